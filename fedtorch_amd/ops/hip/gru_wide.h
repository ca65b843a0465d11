// Persistent GRU sequence kernels for 65 <= H <= 128: the register-resident
// twins of gru_fwd_k / gru_bwd_k (gru.h; same equations, same operand
// contracts, same work split).
//
// At H = 128 the fp32 LDS image of W_hh that gru.h keeps is 3*128*130*4 =
// 199,680 B, more than a CU's 160 KB.  W_hh is constant over the T steps and
// only ever the MFMA B operand, and a lane's B fragments are the same in every
// step, so here each lane loads its fragments from global memory ONCE, before
// the T-loop, and keeps them in registers:
//
//   gru_fwd_reg_k<NT>  lane (lk = l>>4, lr = l&15) of wave w holds
//                      W[g][col = 16w + lr][k = lk + 4 kk] for g in 0..2 and
//                      kk in 0..HP/4-1: 3 HP / 4 registers (96 at HP = 128).
//                      LDS holds only the double-buffered h tile, 2 x 16 x
//                      (HP + 2) floats.  One ds_read_b32 of A feeds three
//                      MFMAs; one barrier per step.
//   gru_bwd_reg_k<NT>  the mirror: W[g][k = 4 kk + lk][col], again 3 HP / 4
//                      registers; dgh[t] double-buffered in LDS as the A
//                      operand, row stride 3 HP + 2.  Three accumulators added
//                      (a0 + a1) + a2 with a0 seeded by dh z, as in gru_bwd_k.
//
// NT = ceil(H/16) in 5..8 waves per workgroup, one workgroup per 16 batch
// rows.  A 512-thread workgroup is 2 waves per SIMD, so a wave may use up to
// 256 unified VGPR + AGPR; the weight arrays are indexed with compile-time
// constants only (every loop over them is fully unrolled) so that they never
// go to scratch.  Resources of the eight instantiations: scratch 0, spills 0
// (profiles/gru_notes.md).  H > 128 does not fit this budget.
//
// Pad columns (col >= H) and pad k (>= H) hold zero and are never loaded;
// batch pad rows are never loaded and never stored.  w_hh / b_hh are read as
// bf16 or fp32 with element loads.  The products are the same k-ordered
// v_mfma_f32_16x16x4_f32 chains as in gru.h (forward seeded with b_hh), so
// integer data stays exact; no atomics, summation order fixed by H, no host
// reads: deterministic and capture-safe.
//
// The LDS row strides HP + 2 and 3 HP + 2 are 2 or 18 mod 32 for every HP
// here, so the ds_read_b32 A fetches stay conflict-free.
#pragma once
#include <hip/hip_runtime.h>
#include "gru.h"

#define GRU_WIDE_MINH 65
#define GRU_WIDE_MAXH 128

// scalar fp32 code only: the gate math below is four independent elements per
// lane, which the compiler may otherwise pair into packed fp32 operations
// (a device feature: the host pass does not know it)
#define GRU_WIDE_KERNEL GRU_SCALAR_F32

// One lane's B fragments of the three gate blocks: dst[g][kk] =
// w[(g H + row0 + kk rstep) H + col0 + kk cstep] where that element exists,
// else 0.  EL is the weight's element type.
template <int KK, typename EL>
__device__ __forceinline__ GRU_WIDE_KERNEL void gru_wide_frag(
    float (&dst)[3][KK], const void* __restrict__ w, int H, int row0,
    int rstep, int col0, int cstep) {
  const EL* p = reinterpret_cast<const EL*>(w);
#pragma unroll
  for (int g = 0; g < 3; ++g) {
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const int row = row0 + kk * rstep, c = col0 + kk * cstep;
      dst[g][kk] = (row < H && c < H)
                       ? (float)p[((long)g * H + row) * H + c] : 0.f;
    }
  }
}

// --------------------------------------------------------------------------
// forward
// --------------------------------------------------------------------------
// grid ceil(B/16), block 64*NT.  gates [B, T, 4, H] = (r, z, n, q) or null.
// TOK (gru_tok_wide_fwd): gx is the table P [V, 3H] and tok [B, T] selects its
// rows, prefetched as in gru_fwd_k; else tok and V are unused.
template <int NT, bool TOK>
__global__ void __launch_bounds__(NT * WAVE) GRU_WIDE_KERNEL
gru_fwd_reg_k(const float* __restrict__ gx, const void* __restrict__ w,
              int w_bf16, const void* __restrict__ bias, int b_bf16,
              const float* __restrict__ h0, float* __restrict__ out,
              float* __restrict__ gates, int B, int T, int H,
              const long* __restrict__ tok, int V) {
  constexpr int HP = NT * 16;
  constexpr int KK = HP / 4;
  constexpr int S = HP + 2;             // S mod 32 in {2, 18}
  constexpr int NTHR = NT * WAVE;
  __shared__ float hs[2][GRU_ROWS * S];  // [buffer][row][k]
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wid = tid / WAVE;
  const int lr = lane & 15, lk = lane >> 4;
  const long b0 = (long)blockIdx.x * GRU_ROWS;
  const int col = wid * 16 + lr;        // hidden column of this lane
  const bool lcol = col < H;

  // B fragments W[g][col][lk + 4 kk], resident for all T steps
  float wf[3][KK];
  if (w_bf16)
    gru_wide_frag<KK, __hip_bfloat16>(wf, w, H, col, 0, lk, 4);
  else
    gru_wide_frag<KK, float>(wf, w, H, col, 0, lk, 4);

  for (int i = tid; i < GRU_ROWS * S; i += NTHR) {
    const int m = i / S, k = i - m * S;
    hs[0][i] = (b0 + m < B && k < H) ? h0[(b0 + m) * H + k] : 0.f;
    hs[1][i] = 0.f;
  }

  bool live[4];
  long ob[4];                           // (b*T)*H + col
  float hprev[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long b = b0 + 4 * lk + i;
    live[i] = lcol && b < B;
    ob[i] = b * T * (long)H + col;
    hprev[i] = live[i] ? h0[b * H + col] : 0.f;
  }
  const float br = lcol ? gru_ld1(bias, col, b_bf16) : 0.f;
  const float bz = lcol ? gru_ld1(bias, H + col, b_bf16) : 0.f;
  const float bn = lcol ? gru_ld1(bias, 2 * H + col, b_bf16) : 0.f;

  float xr[4], xz[4], xn[4];
  int tk[4];                            // TOK: P offset of step t + 1, or -1
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (TOK) {
      const long ti = (b0 + 4 * lk + i) * T;
      const int o = gru_tok_off(tok, ti, live[i], V, 3 * H);
      tk[i] = gru_tok_off(tok, ti + 1, live[i] && 1 < T, V, 3 * H);
      const float* p = gx + o + col;
      xr[i] = o >= 0 ? p[0] : 0.f;
      xz[i] = o >= 0 ? p[H] : 0.f;
      xn[i] = o >= 0 ? p[2 * H] : 0.f;
    } else {
      const float* p = gx + ob[i] * 3 - 2 * col;   // (b*T + 0)*3H + col
      xr[i] = live[i] ? p[0] : 0.f;
      xz[i] = live[i] ? p[H] : 0.f;
      xn[i] = live[i] ? p[2 * H] : 0.f;
    }
  }
  __syncthreads();

  for (int t = 0; t < T; ++t) {
    const int cur = t & 1;
    // next step's input projection, in flight during the MFMAs
    float yr[4], yz[4], yn[4];
    int tn[4];                          // TOK: P offset of step t + 2, or -1
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (TOK) {
        // tk is -1 beyond the last step and on dead rows
        const float* p = gx + tk[i] + col;
        yr[i] = tk[i] >= 0 ? p[0] : 0.f;
        yz[i] = tk[i] >= 0 ? p[H] : 0.f;
        yn[i] = tk[i] >= 0 ? p[2 * H] : 0.f;
        tn[i] = gru_tok_off(tok, (b0 + 4 * lk + i) * T + t + 2,
                            live[i] && t + 2 < T, V, 3 * H);
      } else {
        const bool ld = live[i] && t + 1 < T;
        const float* p = gx + (ob[i] + (long)(t + 1) * H) * 3 - 2 * col;
        yr[i] = ld ? p[0] : 0.f;
        yz[i] = ld ? p[H] : 0.f;
        yn[i] = ld ? p[2 * H] : 0.f;
      }
    }
    gru_f4 ar = {br, br, br, br}, az = {bz, bz, bz, bz},
           an = {bn, bn, bn, bn};
    const float* ha = hs[cur] + lr * S + lk;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const float a = ha[kk * 4];
      ar = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wf[0][kk], ar, 0, 0, 0);
      az = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wf[1][kk], az, 0, 0, 0);
      an = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wf[2][kk], an, 0, 0, 0);
    }
    float* hn = hs[cur ^ 1] + (4 * lk) * S + col;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float r = gru_sigmoid(xr[i] + ar[i]);
      const float z = gru_sigmoid(xz[i] + az[i]);
      const float q = an[i];
      const float n = tanhf(xn[i] + r * q);
      float h = (1.f - z) * n + z * hprev[i];
      if (!live[i]) h = 0.f;
      hn[i * S] = h;
      hprev[i] = h;
      if (live[i]) {
        const long o = ob[i] + (long)t * H;
        out[o] = h;
        if (gates) {
          float* gp = gates + o * 4 - 3 * col;   // ((b*T + t)*4)*H + col
          gp[0] = r;
          gp[H] = z;
          gp[2 * H] = n;
          gp[3 * H] = q;
        }
      }
      xr[i] = yr[i]; xz[i] = yz[i]; xn[i] = yn[i];
      if constexpr (TOK) tk[i] = tn[i];
    }
    __syncthreads();
  }
}

// --------------------------------------------------------------------------
// backward
// --------------------------------------------------------------------------
// grid ceil(B/16), block 64*NT.  dgx, dgh [B, T, 3H]; dh0 [B, H].
template <int NT>
__global__ void __launch_bounds__(NT * WAVE) GRU_WIDE_KERNEL
gru_bwd_reg_k(const float* __restrict__ dout, const float* __restrict__ out,
              const float* __restrict__ gates, const void* __restrict__ w,
              int w_bf16, const float* __restrict__ h0,
              float* __restrict__ dgx, float* __restrict__ dgh,
              float* __restrict__ dh0, int B, int T, int H) {
  constexpr int HP = NT * 16;
  constexpr int KK = HP / 4;
  constexpr int SA = 3 * HP + 2;             // 2 / 18 mod 32
  constexpr int NTHR = NT * WAVE;
  __shared__ float ds[2][GRU_ROWS * SA];     // [buffer][row][gate*HP + n]
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wid = tid / WAVE;
  const int lr = lane & 15, lk = lane >> 4;
  const long b0 = (long)blockIdx.x * GRU_ROWS;
  const int col = wid * 16 + lr;
  const bool lcol = col < H;

  // B fragments W[g][4 kk + lk][col], resident for all T steps
  float wf[3][KK];
  if (w_bf16)
    gru_wide_frag<KK, __hip_bfloat16>(wf, w, H, lk, 4, col, 0);
  else
    gru_wide_frag<KK, float>(wf, w, H, lk, 4, col, 0);

  for (int i = tid; i < GRU_ROWS * SA; i += NTHR) {
    ds[0][i] = 0.f;
    ds[1][i] = 0.f;
  }

  bool live[4];
  long ob[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long b = b0 + 4 * lk + i;
    live[i] = lcol && b < B;
    ob[i] = b * T * (long)H + col;
  }

  // operands of step t: gates (r, z, n, q), h_prev and dout
  float cr[4], cz[4], cn[4], cq[4], chp[4], cdo[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long o = ob[i] + (long)(T - 1) * H;
    const float* gp = gates + o * 4 - 3 * col;
    cr[i] = live[i] ? gp[0] : 0.f;
    cz[i] = live[i] ? gp[H] : 0.f;
    cn[i] = live[i] ? gp[2 * H] : 0.f;
    cq[i] = live[i] ? gp[3 * H] : 0.f;
    cdo[i] = live[i] ? dout[o] : 0.f;
    chp[i] = !live[i] ? 0.f
             : (T > 1 ? out[o - H] : h0[(b0 + 4 * lk + i) * H + col]);
  }
  float dhn[4] = {0.f, 0.f, 0.f, 0.f};
  __syncthreads();

  for (int t = T - 1; t >= 0; --t) {
    const int cur = t & 1;
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
      if (live[i]) {
        const long o = (ob[i] + (long)t * H) * 3 - 2 * col;
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
    __syncthreads();
    // operands of step t-1, in flight during the MFMAs
    float yr[4], yz[4], yn[4], yq[4], yhp[4], ydo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ld = live[i] && t > 0;
      const long o = ob[i] + (long)(t - 1) * H;
      const float* gp = gates + o * 4 - 3 * col;
      yr[i] = ld ? gp[0] : 0.f;
      yz[i] = ld ? gp[H] : 0.f;
      yn[i] = ld ? gp[2 * H] : 0.f;
      yq[i] = ld ? gp[3 * H] : 0.f;
      ydo[i] = ld ? dout[o] : 0.f;
      yhp[i] = !ld ? 0.f
               : (t > 1 ? out[o - H] : h0[(b0 + 4 * lk + i) * H + col]);
    }
    const float* da = ds[cur] + lr * SA + lk;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(
          da[kk * 4], wf[0][kk], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(
          da[HP + kk * 4], wf[1][kk], a1, 0, 0, 0);
      a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(
          da[2 * HP + kk * 4], wf[2][kk], a2, 0, 0, 0);
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
    if (live[i]) dh0[(b0 + 4 * lk + i) * H + col] = dhn[i];
}
