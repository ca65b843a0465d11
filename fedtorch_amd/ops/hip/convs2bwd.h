// MFMA backward kernels for the 3x3 / stride-2 / pad-1 NHWC bf16
// transition convs (16->32 at 32x32, 32->64 at 16x16) on gfx950.
//
// Forward being differentiated (conv3x3_bn_fwd_k<..., S=2>, Ho = Hi/2):
//   y[n,ho,wo,co] = sum_{dh,dw,ci} x[n, 2ho+dh-1, 2wo+dw-1, ci] * w[co,dh,dw,ci]
//
// ---- conv3x3s2_dgrad_k ---------------------------------------------------
//   dx[n,hi,wi,ci] = sum_co sum_{(dh,dw)} dy[n,ho,wo,co] * w[co,dh,dw,ci]
// over the taps with hi+1-dh, wi+1-dw even.  Input pixels split into four
// (hi&1, wi&1) parity classes with 1 / 2 / 2 / 4 live taps:
//   even coordinate: tap 1 only,        o = i/2
//   odd  coordinate: tap 0, o = (i+1)/2  and  tap 2, o = (i-1)/2
// A zero-inserted s1 dgrad would issue 9 taps for every pixel (4x the
// useful MFMAs); here every 16-pixel M-tile holds pixels of ONE class, so
// its tap set is compile-time.  One workgroup = 256 input pixels (R rows of
// one image: 64 per class = one M-tile per wave per class) x CI_TILE
// channels.  The dy slab is R/2 rows + 1 halo row, Wo cols + 1 halo col
// (the only out-of-range taps are tap 0 on the last odd row/col: they read
// the zeroed halo), pixel slots padded by +8 channels like conv3x3_dgrad_k;
// weights sit as [k/8][CI_TILE][8], k = tap*CO + co, all 9 taps resident:
// stage -> barrier -> MFMAs -> store, no further syncs.
//
// ---- conv3x3s2_wrw_k -----------------------------------------------------
//   dw[co,dh,dw,ci] = sum_{n,ho,wo} dy[n,ho,wo,co] * x[n,2ho+dh-1,2wo+dw-1,ci]
// The convwrw2.h design (GEMM-K = output positions, both operands staged
// TRANSPOSED so every fragment is one ds_read_b128, grid-stride loop over
// supertiles, per-block fp32 partials in quadrant-local layout, no
// atomics, ONE conv3x3_wrw2_final_k: the launcher keeps the stream count
// low, so there are few rows to sum).  New here is the stride-2 column walk: x is staged into column-parity-split planes
//   s_xT[ci][row][ even: Wo | 8 zero pad | odd: Wo ]
// so 8 consecutive wo are contiguous for every dw: dw=1 reads the even
// plane at wo, dw=2 the odd plane at wo, dw=0 the odd plane at wo-1 (the
// aligned odd window shifted by one element through v_alignbit with the
// preceding dword; wo=0 lands in the zero pad = the left conv padding).
// Rows are 2*ho+dh-1: a supertile of SR output rows stages 2*SR+1 input
// rows, the top one zero for ho=0.  Right/bottom padding is never touched
// (Hi, Wi even).
//
// Wave split (COB = CO/16, CIB = CI/16): wave -> co block (wave % COB) and,
// when COB < 4, a k-split (wave / COB) over the supertile's 32-position
// chunks, merged in-block through LDS so a block emits one partial row per
// quadrant; every wave loops all CIB ci blocks off one dy fragment.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"
#include <hip/hip_bf16.h>

// bf16x8 / f32x4 come from convwrw.h (same TU)

template <int CI, int CO, int CI_TILE, int WI>
__global__ void __launch_bounds__(FT_BLOCK) conv3x3s2_dgrad_k(
    const __hip_bfloat16* __restrict__ dy,  // [N, HI/2, WI/2, CO]
    const __hip_bfloat16* __restrict__ w,   // [CO, 3, 3, CI]
    __hip_bfloat16* __restrict__ dx,        // [N, HI, WI, CI]
    int N, int HI) {
  constexpr int R = 256 / WI;             // input rows per workgroup
  constexpr int WO = WI / 2, RO = R / 2;
  constexpr int K8 = 9 * CO / 8;
  constexpr int COP = CO + 8;             // padded pixel slot (elements)
  constexpr int YR = RO + 1, YC = WO + 1; // + zero halo row / col
  constexpr int NSLOT = YR * YC;
  constexpr int SCH = COP / 8;            // 16 B chunks per slot
  constexpr int NT = CI_TILE / 16;
  static_assert(RO * WO == 64, "one 16-pixel M-tile per wave per class");
  static_assert(CO % 32 == 0 && CI_TILE % 16 == 0 && CI % CI_TILE == 0, "");

  __shared__ __attribute__((aligned(16))) __hip_bfloat16 ys[NSLOT * COP];
  __shared__ __attribute__((aligned(16))) __hip_bfloat16
      bw[K8 * CI_TILE * 8];

  const int tid = threadIdx.x;
  const int wave = tid / WAVE, lane = tid & (WAVE - 1);
  const int fm = lane & 15, kg = lane >> 4;

  // grid: [N * (HI/R) * (CI/CI_TILE)]
  const int cib = blockIdx.x % (CI / CI_TILE);
  const int rb = (blockIdx.x / (CI / CI_TILE)) % (HI / R);
  const int n = blockIdx.x / ((CI / CI_TILE) * (HI / R));
  const int ci0 = cib * CI_TILE;
  const int h0 = rb * R;                  // input row base (even)
  const int HO = HI / 2, ho0 = h0 / 2;

  // ---- stage weights: bw[k/8][ci][k%8] = w[co][tap][ci0+ci],
  //      k = tap*CO + co.  16 B global reads along ci, transposing
  //      scalar LDS writes.
  for (int e = tid; e < 9 * CO * (CI_TILE / 8); e += FT_BLOCK) {
    const int kq = e / (CI_TILE / 8);     // co*9 + tap (memory order)
    const int c8 = (e % (CI_TILE / 8)) * 8;
    const int co = kq / 9, tap = kq % 9;
    const uint4 v =
        *reinterpret_cast<const uint4*>(w + (long)kq * CI + ci0 + c8);
    const __hip_bfloat16* vp = reinterpret_cast<const __hip_bfloat16*>(&v);
    const int k = tap * CO + co;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      bw[((long)(k >> 3) * CI_TILE + c8 + i) * 8 + (k & 7)] = vp[i];
  }

  // ---- stage dy slab: every 16 B chunk of every slot written exactly
  //      once (halo row/col, channel pad = 0)
  for (int e = tid; e < NSLOT * SCH; e += FT_BLOCK) {
    const int slot = e / SCH, c8 = (e % SCH) * 8;
    const int row = slot / YC, col = slot % YC;
    const int ho = ho0 + row;
    uint4 v = {0, 0, 0, 0};
    if (c8 < CO && col < WO && ho < HO)
      v = *reinterpret_cast<const uint4*>(
          dy + (((long)n * HO + ho) * WO + col) * CO + c8);
    *reinterpret_cast<uint4*>(&ys[(long)slot * COP + c8]) = v;
  }
  __syncthreads();

  // ---- MFMAs: class cls = (hi&1)*2 + (wi&1); this lane's A pixel of the
  //      wave's M-tile is (r, c) in class coordinates: hi = h0 + 2r + ph
  f32x4 acc[4][NT];
#pragma unroll
  for (int cls = 0; cls < 4; ++cls)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[cls][nt] = {0.f, 0.f, 0.f, 0.f};

  const int pa = wave * 16 + fm;
  const int ra = pa / WO, ca = pa % WO;
#pragma unroll
  for (int cls = 0; cls < 4; ++cls) {
    const int ph = cls >> 1, pw = cls & 1;
#pragma unroll
    for (int th = 0; th <= ph; ++th) {
      const int dh = ph ? 2 * th : 1;     // odd: taps 0, 2; even: tap 1
      const int ro = (ph && dh == 0) ? 1 : 0;
#pragma unroll
      for (int tw = 0; tw <= pw; ++tw) {
        const int dw = pw ? 2 * tw : 1;
        const int cof = (pw && dw == 0) ? 1 : 0;
        const int tap = dh * 3 + dw;
        const int slot = (ra + ro) * YC + ca + cof;
#pragma unroll
        for (int cs = 0; cs < CO / 32; ++cs) {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(
              &ys[(long)slot * COP + cs * 32 + kg * 8]);
          const int k8 = (tap * CO + cs * 32) / 8 + kg;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(
                &bw[((long)k8 * CI_TILE + nt * 16 + fm) * 8]);
            acc[cls][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a, b, acc[cls][nt], 0, 0, 0);
          }
        }
      }
    }
  }

  // ---- store dx: D col = fm (channel), row = kg*4 + reg (pixel) --------
#pragma unroll
  for (int cls = 0; cls < 4; ++cls) {
    const int ph = cls >> 1, pw = cls & 1;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const int p = wave * 16 + kg * 4 + r4;
      const int hi = h0 + 2 * (p / WO) + ph, wi = 2 * (p % WO) + pw;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        dx[(((long)n * HI + hi) * WI + wi) * CI + ci0 + nt * 16 + fm] =
            (__hip_bfloat16)acc[cls][nt][r4];
    }
  }
}


template <int CO, int CI, int WI>
struct S2WrwCfg {
  static constexpr int WO = WI / 2;
  static constexpr int SR = 8;                     // output rows/supertile
  static constexpr int SPOS = SR * WO;             // 128 / 64 positions
  static constexpr int CH = SPOS / 32;             // 32-position k-chunks
  static constexpr int XR = 2 * SR + 1;            // staged input rows
  static constexpr int ODD = WO + 8;               // odd plane offset
  static constexpr int XCP = 2 * WO + 8;           // row stride (elements)
  // plane strides: multiples of 8 elements with stride % 16 == 8 so the 16
  // planes of a fragment read walk distinct banks (convwrw2.h)
  static constexpr int SXR = XR * XCP;
  static constexpr int SX = (SXR % 16 == 8) ? SXR : ((SXR & ~15) + 8 +
                            ((SXR % 16 > 8) ? 16 : 0));
  static constexpr int SD = (SPOS % 16 == 8) ? SPOS : SPOS + 8;
  static constexpr int COB = CO / 16, CIB = CI / 16;
  static constexpr int KS = (COB < 4) ? 4 / COB : 1;  // wave k-splits
  static constexpr int Q = COB * CIB;
  static_assert(COB <= 4 && 4 % COB == 0 && CH % KS == 0, "wave split");
  static_assert(WO % 8 == 0, "8 consecutive wo stay in one output row");
};

template <int CO, int CI, int WI>
__global__ void __launch_bounds__(FT_BLOCK) conv3x3s2_wrw_k(
    const __hip_bfloat16* __restrict__ dy,  // [N, HI/2, WI/2, CO]
    const __hip_bfloat16* __restrict__ x,   // [N, HI, WI, CI]
    float* __restrict__ part,               // [Q * RQ][9*16*16], RQ = grid
    int N, int HI, int RQ) {
  using C = S2WrwCfg<CO, CI, WI>;
  constexpr int WO = C::WO;
  __shared__ __attribute__((aligned(16))) __hip_bfloat16 s_dyT[CO * C::SD];
  __shared__ __attribute__((aligned(16))) __hip_bfloat16 s_xT[CI * C::SX];

  const int tid = threadIdx.x;
  const int wave = tid / WAVE, lane = tid & (WAVE - 1);
  const int fm = lane & 15, kg = lane >> 4;
  const int cob = wave % C::COB, ksp = wave / C::COB;

  // zero once: the odd plane's leading pad (and the plane-stride tail)
  // must read 0 for every supertile; body writes never touch them
  for (int e = tid; e < CI * C::SX / 8; e += FT_BLOCK)
    *reinterpret_cast<uint4*>(&s_xT[(long)e * 8]) = uint4{0, 0, 0, 0};

  f32x4 acc[C::CIB][9];
#pragma unroll
  for (int b = 0; b < C::CIB; ++b)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[b][t] = {0.f, 0.f, 0.f, 0.f};

  const int HO = HI / 2;
  const int tiles_per_img = HO / C::SR;
  const long tiles = (long)N * tiles_per_img;
  __syncthreads();

  for (long tg = blockIdx.x; tg < tiles; tg += gridDim.x) {
    const int n = (int)(tg / tiles_per_img);
    const int ho0 = (int)(tg % tiles_per_img) * C::SR;

    // ---- stage dy transposed: [pos][co] -> s_dyT[co][pos] --------------
    {
      const __hip_bfloat16* dyp = dy + (((long)n * HO + ho0) * WO) * CO;
      constexpr int CHK = C::SPOS * CO / 8;
      for (int e = tid; e < CHK; e += FT_BLOCK) {
        const int pos = e * 8 / CO, c8 = (e * 8) % CO;
        const uint4 v =
            *reinterpret_cast<const uint4*>(dyp + (long)pos * CO + c8);
        const __hip_bfloat16* vp =
            reinterpret_cast<const __hip_bfloat16*>(&v);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          s_dyT[(long)(c8 + j) * C::SD + pos] = vp[j];
      }
    }
    // ---- stage x transposed, columns split by parity ------------------
    {
      constexpr int CHK = C::XR * WI * CI / 8;
      for (int e = tid; e < CHK; e += FT_BLOCK) {
        const int rowe = e * 8 / (WI * CI);
        const int rem = (e * 8) % (WI * CI);
        const int col = rem / CI, c8 = rem % CI;
        const int hh = 2 * ho0 - 1 + rowe;   // < HI always; -1 for ho0 = 0
        uint4 v = {0, 0, 0, 0};
        if (hh >= 0)
          v = *reinterpret_cast<const uint4*>(
              x + (((long)n * HI + hh) * WI + col) * CI + c8);
        const __hip_bfloat16* vp =
            reinterpret_cast<const __hip_bfloat16*>(&v);
        const int off = rowe * C::XCP + (col & 1) * C::ODD + (col >> 1);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          s_xT[(long)(c8 + j) * C::SX + off] = vp[j];
      }
    }
    __syncthreads();

    // ---- MFMAs ----------------------------------------------------------
#pragma unroll
    for (int i = 0; i < C::CH / C::KS; ++i) {
      const int ch = ksp + i * C::KS;
      const int pb = ch * 32 + kg * 8;          // this lane's 8 positions
      const int r0 = pb / WO, w0 = pb % WO;     // w0 % 8 == 0
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(
          &s_dyT[(long)(cob * 16 + fm) * C::SD + pb]);
#pragma unroll
      for (int b = 0; b < C::CIB; ++b) {
#pragma unroll
        for (int dh = 0; dh < 3; ++dh) {
          const __hip_bfloat16* bp =
              &s_xT[(long)(b * 16 + fm) * C::SX + (2 * r0 + dh) * C::XCP + w0];
          typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
          const u32x4 ev = *reinterpret_cast<const u32x4*>(bp);
          const u32x4 od = *reinterpret_cast<const u32x4*>(bp + C::ODD);
          // dword holding odd-plane elements (wo-2, wo-1); wo = 0 reads
          // the zero pad
          const unsigned pv =
              *reinterpret_cast<const unsigned*>(bp + C::ODD - 2);
          u32x4 f0;
          f0.x = __builtin_amdgcn_alignbit(od.x, pv, 16);
          f0.y = __builtin_amdgcn_alignbit(od.y, od.x, 16);
          f0.z = __builtin_amdgcn_alignbit(od.z, od.y, 16);
          f0.w = __builtin_amdgcn_alignbit(od.w, od.z, 16);
          acc[b][dh * 3 + 0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, __builtin_bit_cast(bf16x8, f0), acc[b][dh * 3 + 0], 0, 0, 0);
          acc[b][dh * 3 + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, __builtin_bit_cast(bf16x8, ev), acc[b][dh * 3 + 1], 0, 0, 0);
          acc[b][dh * 3 + 2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, __builtin_bit_cast(bf16x8, od), acc[b][dh * 3 + 2], 0, 0, 0);
        }
      }
    }
    __syncthreads();  // slab consumed; next supertile may overwrite
  }

  // ---- k-split merge: waves (cob, ksp=1) hand their accumulators to
  // (cob, ksp=0) through the consumed x slab, so the block emits ONE row
  // per quadrant (half the partial traffic for the 16->32 conv)
  if constexpr (C::KS > 1) {
    static_assert(C::KS <= 2, "pairwise merge");
    static_assert(C::COB * C::CIB * 36 * WAVE * 4 <= CI * C::SX * 2,
                  "merge buffer fits the x slab");
    float* mb = reinterpret_cast<float*>(s_xT);
    if (ksp == 1) {
#pragma unroll
      for (int b = 0; b < C::CIB; ++b)
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            mb[(((cob * C::CIB + b) * 9 + t) * 4 + r) * WAVE + lane] =
                acc[b][t][r];
    }
    __syncthreads();
    if (ksp == 1) return;
#pragma unroll
    for (int b = 0; b < C::CIB; ++b)
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[b][t][r] +=
              mb[(((cob * C::CIB + b) * 9 + t) * 4 + r) * WAVE + lane];
  }

  // ---- partial rows: quadrant q = cob*CIB + b, one row per block -------
  // D of mfma(a=dy, b=x): col = fm -> ci, row = kg*4 + reg -> co
#pragma unroll
  for (int b = 0; b < C::CIB; ++b) {
    const int q = cob * C::CIB + b;
    float* pr = part + ((long)q * RQ + blockIdx.x) * (9 * 16 * 16);
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        pr[t * 256 + (kg * 4 + r) * 16 + fm] = acc[b][t][r];
  }
}

// The partial rows are summed, cast and scattered into dw by
// conv3x3_wrw2_final_k (convwrw2.h, same partial layout).
