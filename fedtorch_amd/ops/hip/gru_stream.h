// Persistent GRU sequence kernels for 129 <= H <= 256: the streamed-weight
// twins of gru_fwd_k / gru_bwd_k (gru.h; same equations, same operand
// contracts, same work split).
//
// At H = 256 the fp32 image of W_hh is 3*256*256*4 = 786 KB: more than a CU's
// LDS (160 KB, gru.h) and more than its vector registers (512 KB, gru_wide.h),
// so no workgroup can keep it.  It is constant over the T steps and shared by
// all batch tiles, though, so after the first step L2 / Infinity Cache serve
// it.  These kernels therefore read W_hh from global memory in EVERY step,
// straight into MFMA B fragments (a wave is the only consumer of its
// fragments, so they do not pass through LDS):
//
//   gru_fwd_stream_k<NT>  per 16-deep k block j, lane (lr = l&15, lk = l>>4)
//                         of wave w loads W[g][16w + lr][16j + 4lk .. +3] for
//                         the three gates: one 16-byte load each (8 bytes
//                         and a widen for bf16).  The A operand is the
//                         matching ds_read_b128 of h[lr][16j + 4lk .. +3]
//                         from the double-buffered h tile, and the block's
//                         four MFMA k-steps take element e = 0..3 of both:
//                         k-step e multiplies k = 16j + 4lk' + e, lk' = 0..3.
//   gru_bwd_stream_k<NT>  the mirror: dgh[t] double-buffered in LDS at width
//                         3 HP as the A operand, read with one ds_read_b128
//                         per gate and k block; the B fragment is the
//                         transposed one, W[g][16j + 4lk + e][16w + lr], from
//                         W_hh in its natural layout.  Memory runs along the
//                         output column there, so a lane's four k are four
//                         rows apart and are four element loads (a half wave
//                         reads 64 contiguous bytes of each row); a 16-byte
//                         load would need a cross-lane transpose.  Three
//                         accumulators added (a0 + a1) + a2 with a0 seeded by
//                         dh z, as in gru_bwd_reg_k.
//
// The weight stream is software-pipelined one k block ahead of the MFMAs that
// consume it and wraps round: the last block of a step loads block 0 of the
// next step, across the barrier.  The next step's gx (forward) / gates, dout
// and h_prev (backward) are loaded before the MFMAs as well.  One barrier per
// step.
//
// NT = ceil(H/16) in 9..16 waves per workgroup, one workgroup per 16 batch
// rows.  At NT = 16 the 1024-thread workgroup is 4 waves per SIMD, i.e. 128
// unified registers per wave: two weight blocks (24), the accumulators (12),
// the A fragments and the prefetched operands fit that.  Resources of the
// sixteen instantiations: scratch 0, spills 0 (profiles/gru_notes.md).
//
// LDS row strides are HP + 4 (h) and 3 HP + 4 (dgh) floats: multiples of 4, so
// every ds_read_b128 is 16-byte aligned, and 4 x an odd number (HP is a
// multiple of 16).  The 16 lanes lr = 0..15 of one lk read the 4-bank groups
// lr * stride + const; stride / 4 is odd, so any 8 consecutive lr cover the 8
// groups of 32 banks once (and all 16 the 16 groups of 64 banks):
// conflict-free whichever way the hardware splits the 128-bit read.
//
// Pad columns (col >= H) and pad k (>= H) are zeros, and nothing outside w_hh
// is ever read: the weight loads are branch-free, and a lane whose element
// does not exist reads the first element of the block's first row instead
// and selects 0.  Batch pad rows are never loaded and never stored.  The
// 16-byte (8-byte) forward loads are used only where the launcher has checked
// that H is a multiple of 4 and w_hh is 16-byte (8-byte) aligned (w_vec);
// then every four-element group is all inside or all outside a row.
// Otherwise, and always in the backward kernel, the weights are read with
// element loads and nothing beyond element alignment is assumed.
//
// Register budget.  Left alone the compiler lifts everything that does not
// change over the steps out of the T-loop and spills; GRU_STREAM_OPAQUE_*
// below, the live-row count nl and the per-block schedule fence are what
// keeps all sixteen instantiations under 100 registers.
//
// The products are v_mfma_f32_16x16x4_f32 with fp32 accumulation (forward
// seeded with b_hh), so integer data stays exact.  Within a k block the
// summation runs in the permuted order above, which differs from gru.h /
// gru_wide.h; it is fixed by H alone.  No atomics, no host reads, no
// synchronisation between workgroups: deterministic and capture-safe.
#pragma once
#include <hip/hip_runtime.h>
#include "gru.h"

#define GRU_STREAM_MINH 129
#define GRU_STREAM_MAXH 256

// scalar fp32 code only, as in gru_wide.h
#define GRU_STREAM_KERNEL GRU_SCALAR_F32

// W_hh does not change over the steps, so the compiler would lift a step's
// weight addresses, masks and loads out of the T-loop (the gru_wide.h design,
// which does not fit here), and it keeps one strength-reduced 64-bit address
// per row and operand of gx / gates / out / dgx / dgh alive over the loop, some
// 60 registers.  Making the lane's weight offset, its k count, H and its row
// offset opaque once per step keeps all of that in the step that uses it.
#define GRU_STREAM_OPAQUE_V(x) asm volatile("" : "+v"(x))
#define GRU_STREAM_OPAQUE_S(x) asm volatile("" : "+s"(x))

// Header functions without the kernels' target attribute are not inlined into
// them, so the barrier and the bit cast are spelled with builtins here.
__device__ __forceinline__ GRU_STREAM_KERNEL void gru_stream_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ GRU_STREAM_KERNEL float gru_stream_bits(
    unsigned u) {
  return __builtin_bit_cast(float, u);
}

// The weight loads below are a wave-uniform pointer plus the lane's unsigned
// 32-bit byte offset, the form that needs one address register per lane.
// They are branch-free: where an element does not exist the lane reads the
// first element at wg instead (callers pass a wg that is inside w_hh) and
// selects 0.  ES is the element size, 4 (fp32) or 2 (bf16).
template <int ES>
__device__ __forceinline__ GRU_STREAM_KERNEL float gru_stream_ld(const char* p) {
  if constexpr (ES == 2)
    return gru_stream_bits(
        (unsigned)*reinterpret_cast<const unsigned short*>(p) << 16);
  else
    return *reinterpret_cast<const float*>(p);
}

// Forward fragment: the four consecutive elements at wg + off, of which the
// first n exist (n <= 0: none, n >= 4: all).  VEC: n <= 0 or n >= 4, and wg, off are multiples of 4 ES
// bytes: one 16-byte (fp32) / 8-byte (bf16) load.
template <int ES, bool VEC>
__device__ __forceinline__ GRU_STREAM_KERNEL gru_f4 gru_stream_row4(
    const char* __restrict__ wg, unsigned off, int n) {
  gru_f4 v;
  if constexpr (VEC) {
    const bool ok = n >= 4;
    const char* p = wg + (ok ? off : 0u);
    if constexpr (ES == 2) {
      const uint2 u = *reinterpret_cast<const uint2*>(p);
      v[0] = gru_stream_bits(u.x << 16);
      v[1] = gru_stream_bits(u.x & 0xffff0000u);
      v[2] = gru_stream_bits(u.y << 16);
      v[3] = gru_stream_bits(u.y & 0xffff0000u);
    } else {
      v = *reinterpret_cast<const gru_f4*>(p);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = ok ? v[i] : 0.f;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = i < n;
      const float x = gru_stream_ld<ES>(wg + (ok ? off + i * ES : 0u));
      v[i] = ok ? x : 0.f;
    }
  }
  return v;
}

// Backward (transposed) fragment: the elements at wg + i rowb + off, i = 0..3
// (rowb: bytes of one W_hh row), of which the first n exist.
template <int ES>
__device__ __forceinline__ GRU_STREAM_KERNEL gru_f4 gru_stream_col4(
    const char* __restrict__ wg, unsigned rowb, unsigned off, int n) {
  gru_f4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool ok = i < n;
    const float x = gru_stream_ld<ES>(wg + (ok ? off + i * rowb : 0u));
    v[i] = ok ? x : 0.f;
  }
  return v;
}

// --------------------------------------------------------------------------
// forward
// --------------------------------------------------------------------------
// grid ceil(B/16), block 64*NT.  gates [B, T, 4, H] = (r, z, n, q) or null.
// hs: the kernel's LDS, [2][16 * S] floats, 16-byte aligned
template <int NT, int ES, bool VEC>
__device__ __forceinline__ GRU_STREAM_KERNEL void gru_fwd_stream_body(
    float (*__restrict__ hs)[GRU_ROWS * (NT * 16 + 4)],
    const float* __restrict__ gx, const void* __restrict__ w,
    const void* __restrict__ bias, int b_bf16, const float* __restrict__ h0,
    float* __restrict__ out, float* __restrict__ gates, int B, int T, int H) {
  constexpr int HP = NT * 16;
  constexpr int S = HP + 4;             // 4 x odd
  constexpr int NTHR = NT * WAVE;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wid = tid / WAVE;
  const int lr = lane & 15, lk = lane >> 4;
  const long b0 = (long)blockIdx.x * GRU_ROWS;
  const int col = wid * 16 + lr;        // hidden column of this lane
  const bool lcol = col < H;

  for (int i = tid; i < GRU_ROWS * S; i += NTHR) {
    const int m = i / S, k = i - m * S;
    hs[0][i] = (b0 + m < B && k < H) ? h0[(b0 + m) * H + k] : 0.f;
    hs[1][i] = 0.f;
  }

  // row i of this lane is b0 + 4 lk + i; (b*T)*H + col of it is ob + i TH
  const long TH = (long)T * H;
  long ob = (b0 + 4 * lk) * TH + col;
  // rows i < nl exist (and col does); one register, where four lane masks
  // would sit in scalar registers over the whole loop
  const int nl = lcol ? (int)min(max(B - b0 - 4 * lk, 0L), 4L) : 0;
  float hprev[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    hprev[i] = i < nl ? h0[(b0 + 4 * lk + i) * H + col] : 0.f;
  const float br = lcol ? gru_ld1(bias, col, b_bf16) : 0.f;
  const float bz = lcol ? gru_ld1(bias, H + col, b_bf16) : 0.f;
  const float bn = lcol ? gru_ld1(bias, 2 * H + col, b_bf16) : 0.f;

  float xr[4], xz[4], xn[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float* p = gx + (ob + i * TH) * 3 - 2 * col;   // (b*T)*3H + col
    xr[i] = i < nl ? p[0] : 0.f;
    xz[i] = i < nl ? p[H] : 0.f;
    xn[i] = i < nl ? p[2 * H] : 0.f;
  }

  // B fragments W[g][col][16j + 4lk .. +3] of k block j = 0; from here on the
  // stream runs one block ahead of the MFMAs
  const char* wp = reinterpret_cast<const char*>(w);
  unsigned we = (unsigned)(col * H + 4 * lk) * ES;   // used only where lcol
  int krem = lcol ? H - 4 * lk : 0;
  int gb = H * H * ES;                  // bytes of a gate block
  gru_f4 wc[3];
#pragma unroll
  for (int g = 0; g < 3; ++g)
    wc[g] = gru_stream_row4<ES, VEC>(wp + (long)g * gb, we,
                                     krem);
  gru_stream_barrier();

  for (int t = 0; t < T; ++t) {
    const int cur = t & 1;
    GRU_STREAM_OPAQUE_V(we);
    GRU_STREAM_OPAQUE_V(ob);
    GRU_STREAM_OPAQUE_V(krem);
    int kr = krem;
    GRU_STREAM_OPAQUE_S(gb);
    // next step's input projection, in flight during the MFMAs
    float yr[4], yz[4], yn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ld = i < nl && t + 1 < T;
      const float* p = gx + (ob + i * TH + (long)(t + 1) * H) * 3 - 2 * col;
      yr[i] = ld ? p[0] : 0.f;
      yz[i] = ld ? p[H] : 0.f;
      yn[i] = ld ? p[2 * H] : 0.f;
    }
    gru_f4 ar = {br, br, br, br}, az = {bz, bz, bz, bz},
           an = {bn, bn, bn, bn};
    const float* ha = hs[cur] + lr * S + 4 * lk;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      // block j + 1; the last block fetches block 0 for the next step
      const int kn = (j + 1 == NT) ? 0 : 16 * (j + 1);
      // its k count, stepped and opaque: as krem - kn the compiler holds one
      // scalar register per block and element for the constants
      kr = (j + 1 == NT) ? krem : kr - 16;
      GRU_STREAM_OPAQUE_V(kr);
      gru_f4 wn[3];
#pragma unroll
      for (int g = 0; g < 3; ++g)
        wn[g] = gru_stream_row4<ES, VEC>(wp + (long)g * gb + kn * ES, we,
                                         kr);
      const gru_f4 a = *reinterpret_cast<const gru_f4*>(ha + 16 * j);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ar = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], wc[0][e], ar, 0, 0, 0);
        az = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], wc[1][e], az, 0, 0, 0);
        an = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], wc[2][e], an, 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < 3; ++g) wc[g] = wn[g];
      // keep each block's loads with its own MFMAs: moved further ahead they
      // cost 12 registers a block
      __builtin_amdgcn_sched_barrier(0);
    }
    float* hn = hs[cur ^ 1] + (4 * lk) * S + col;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float r = gru_sigmoid(xr[i] + ar[i]);
      const float z = gru_sigmoid(xz[i] + az[i]);
      const float q = an[i];
      const float n = tanhf(xn[i] + r * q);
      float h = (1.f - z) * n + z * hprev[i];
      if (!(i < nl)) h = 0.f;
      hn[i * S] = h;
      hprev[i] = h;
      if (i < nl) {
        const long o = ob + i * TH + (long)t * H;
        out[o] = h;
        if (gates) {
          float* gp = gates + o * 4 - 3 * col;     // ((b*T + t)*4)*H + col
          gp[0] = r;
          gp[H] = z;
          gp[2 * H] = n;
          gp[3 * H] = q;
        }
      }
      xr[i] = yr[i]; xz[i] = yz[i]; xn[i] = yn[i];
    }
    gru_stream_barrier();
  }
}

template <int NT>
__global__ void __launch_bounds__(NT * WAVE) GRU_STREAM_KERNEL
gru_fwd_stream_k(const float* __restrict__ gx, const void* __restrict__ w,
                 int w_bf16, int w_vec, const void* __restrict__ bias,
                 int b_bf16, const float* __restrict__ h0,
                 float* __restrict__ out, float* __restrict__ gates, int B,
                 int T, int H) {
  __shared__ __attribute__((aligned(16))) float
      hs[2][GRU_ROWS * (NT * 16 + 4)];  // [buffer][row][k]
#define GRU_STREAM_FWD(ES, VEC)                                             \
  gru_fwd_stream_body<NT, ES, VEC>(hs, gx, w, bias, b_bf16, h0, out, gates, \
                                   B, T, H)
  if (w_vec) {
    if (w_bf16) GRU_STREAM_FWD(2, true); else GRU_STREAM_FWD(4, true);
  } else {
    if (w_bf16) GRU_STREAM_FWD(2, false); else GRU_STREAM_FWD(4, false);
  }
#undef GRU_STREAM_FWD
}

// --------------------------------------------------------------------------
// backward
// --------------------------------------------------------------------------
// grid ceil(B/16), block 64*NT.  dgx, dgh [B, T, 3H]; dh0 [B, H].
// ds: the kernel's LDS, [2][16 * SA] floats, 16-byte aligned
template <int NT, int ES>
__device__ __forceinline__ GRU_STREAM_KERNEL void gru_bwd_stream_body(
    float (*__restrict__ ds)[GRU_ROWS * (3 * NT * 16 + 4)],
    const float* __restrict__ dout, const float* __restrict__ out,
    const float* __restrict__ gates, const void* __restrict__ w,
    const float* __restrict__ h0, float* __restrict__ dgx,
    float* __restrict__ dgh, float* __restrict__ dh0, int B, int T, int H) {
  constexpr int HP = NT * 16;
  constexpr int SA = 3 * HP + 4;             // 4 x odd
  constexpr int NTHR = NT * WAVE;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wid = tid / WAVE;
  const int lr = lane & 15, lk = lane >> 4;
  const long b0 = (long)blockIdx.x * GRU_ROWS;
  const int col = wid * 16 + lr;
  const bool lcol = col < H;

  for (int i = tid; i < GRU_ROWS * SA; i += NTHR) {
    ds[0][i] = 0.f;
    ds[1][i] = 0.f;
  }

  // row i of this lane is b0 + 4 lk + i; (b*T)*H + col of it is ob + i TH
  const long TH = (long)T * H;
  long ob = (b0 + 4 * lk) * TH + col;
  // rows i < nl exist (and col does); one register, where four lane masks
  // would sit in scalar registers over the whole loop
  const int nl = lcol ? (int)min(max(B - b0 - 4 * lk, 0L), 4L) : 0;

  // operands of step t: gates (r, z, n, q), h_prev and dout
  float cr[4], cz[4], cn[4], cq[4], chp[4], cdo[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long o = ob + i * TH + (long)(T - 1) * H;
    const float* gp = gates + o * 4 - 3 * col;
    cr[i] = i < nl ? gp[0] : 0.f;
    cz[i] = i < nl ? gp[H] : 0.f;
    cn[i] = i < nl ? gp[2 * H] : 0.f;
    cq[i] = i < nl ? gp[3 * H] : 0.f;
    cdo[i] = i < nl ? dout[o] : 0.f;
    chp[i] = !(i < nl) ? 0.f
             : (T > 1 ? out[o - H] : h0[(b0 + 4 * lk + i) * H + col]);
  }
  float dhn[4] = {0.f, 0.f, 0.f, 0.f};

  // B fragments W[g][16j + 4lk + e][col] of k block j = 0
  const char* wp = reinterpret_cast<const char*>(w);
  unsigned we = (unsigned)(4 * lk * H + col) * ES;   // used only where lcol
  int krem = lcol ? H - 4 * lk : 0;
  unsigned rowb = H * ES;               // bytes of a W_hh row
  gru_f4 wc[3];
#pragma unroll
  for (int g = 0; g < 3; ++g)
    wc[g] = gru_stream_col4<ES>(wp + (long)g * H * rowb, rowb, we,
                                krem);
  gru_stream_barrier();

  for (int t = T - 1; t >= 0; --t) {
    const int cur = t & 1;
    GRU_STREAM_OPAQUE_V(we);
    GRU_STREAM_OPAQUE_V(ob);
    GRU_STREAM_OPAQUE_V(krem);
    int kr = krem;
    GRU_STREAM_OPAQUE_S(rowb);
    gru_f4 a0, a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f};
    float* dp = ds[cur] + (4 * lk) * SA + col;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float dh = cdo[i] + dhn[i];
      const float r = cr[i], z = cz[i], n = cn[i];
      const float dn = dh * (1.f - z);
      const float dz = dh * (chp[i] - n);
      float dan = dn * (1.f - n * n);
      float daz = dz * (z * (1.f - z));
      float dar = (dan * cq[i]) * (r * (1.f - r));
      float dhr = dan * r;
      float dhz = dh * z;
      if (i < nl) {
        const long o = (ob + i * TH + (long)t * H) * 3 - 2 * col;
        dgx[o] = dar; dgx[o + H] = daz; dgx[o + 2 * H] = dan;
        dgh[o] = dar; dgh[o + H] = daz; dgh[o + 2 * H] = dhr;
      } else {
        dar = 0.f; daz = 0.f; dhr = 0.f; dhz = 0.f;
      }
      dp[i * SA] = dar;
      dp[i * SA + HP] = daz;
      dp[i * SA + 2 * HP] = dhr;
      a0[i] = dhz;
    }
    gru_stream_barrier();
    // operands of step t-1, in flight during the MFMAs
    float yr[4], yz[4], yn[4], yq[4], yhp[4], ydo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ld = i < nl && t > 0;
      const long o = ob + i * TH + (long)(t - 1) * H;
      const float* gp = gates + o * 4 - 3 * col;
      yr[i] = ld ? gp[0] : 0.f;
      yz[i] = ld ? gp[H] : 0.f;
      yn[i] = ld ? gp[2 * H] : 0.f;
      yq[i] = ld ? gp[3 * H] : 0.f;
      ydo[i] = ld ? dout[o] : 0.f;
      yhp[i] = !ld ? 0.f
               : (t > 1 ? out[o - H] : h0[(b0 + 4 * lk + i) * H + col]);
    }
    const float* da = ds[cur] + lr * SA + 4 * lk;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      // block j + 1; the last block fetches block 0 for the next step
      const int kn = (j + 1 == NT) ? 0 : 16 * (j + 1);
      // its k count, stepped and opaque: as krem - kn the compiler holds one
      // scalar register per block and element for the constants
      kr = (j + 1 == NT) ? krem : kr - 16;
      GRU_STREAM_OPAQUE_V(kr);
      gru_f4 wn[3];
#pragma unroll
      for (int g = 0; g < 3; ++g)
        wn[g] = gru_stream_col4<ES>(wp + ((long)g * H + kn) * rowb, rowb,
                                    we, kr);
      const gru_f4 d0 = *reinterpret_cast<const gru_f4*>(da + 16 * j);
      const gru_f4 d1 = *reinterpret_cast<const gru_f4*>(da + HP + 16 * j);
      const gru_f4 d2 =
          *reinterpret_cast<const gru_f4*>(da + 2 * HP + 16 * j);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(d0[e], wc[0][e], a0, 0, 0,
                                                  0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(d1[e], wc[1][e], a1, 0, 0,
                                                  0);
        a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(d2[e], wc[2][e], a2, 0, 0,
                                                  0);
      }
#pragma unroll
      for (int g = 0; g < 3; ++g) wc[g] = wn[g];
      // keep each block's loads with its own MFMAs: moved further ahead they
      // cost 12 registers a block
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      dhn[i] = (a0[i] + a1[i]) + a2[i];
      cr[i] = yr[i]; cz[i] = yz[i]; cn[i] = yn[i]; cq[i] = yq[i];
      chp[i] = yhp[i]; cdo[i] = ydo[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (i < nl) dh0[(b0 + 4 * lk + i) * H + col] = dhn[i];
}

template <int NT>
__global__ void __launch_bounds__(NT * WAVE) GRU_STREAM_KERNEL
gru_bwd_stream_k(const float* __restrict__ dout,
                 const float* __restrict__ out,
                 const float* __restrict__ gates, const void* __restrict__ w,
                 int w_bf16, const float* __restrict__ h0,
                 float* __restrict__ dgx, float* __restrict__ dgh,
                 float* __restrict__ dh0, int B, int T, int H) {
  __shared__ __attribute__((aligned(16))) float
      ds[2][GRU_ROWS * (3 * NT * 16 + 4)];   // [buffer][row][gate*HP + n]
  if (w_bf16)
    gru_bwd_stream_body<NT, 2>(ds, dout, out, gates, w, h0, dgx, dgh, dh0, B,
                               T, H);
  else
    gru_bwd_stream_body<NT, 4>(ds, dout, out, gates, w, h0, dgx, dgh, dh0, B,
                               T, H);
}
