// MFMA 3x3/s1/p1 NHWC bf16 conv weight-gradient, v2 (gfx950).
//
// v1 (convwrw.h) stages 32 positions per wave-private slab and reads
// every MFMA fragment element with a SCALAR ds_read (k = the position
// axis, memory is channel-contiguous): it measured 77/28/33 us per call
// vs MIOpen's 33/25/22 (incl. its SubTensorOp/cast wrappers).  v2 fixes
// the layout, not the schedule:
//
//   * staging TRANSPOSES both operands into LDS — s_dyT[co][pos] and
//     s_xT[ci][pos-with-halo] — so every fragment is ONE contiguous
//     ds_read_b128 (the transpose costs scalar ds_writes, which are
//     cheap and cooperative across the 4 waves);
//   * the 3 tap COLUMN shifts never touch LDS again: each (dh) row is
//     read once as a 16-position aligned window (2x b128) and the
//     dw = 0/1/2 fragments come out of registers (dw=1 via v_alignbit
//     by 16 bits, dw=2 is a free dword shuffle);
//   * one supertile (128 positions; 64 = one image for W=8) is staged
//     cooperatively per workgroup per iteration, single-buffered
//     (stage -> barrier -> MFMAs -> barrier), overlap from several
//     resident workgroups per CU.
//
// Work split.  A workgroup owns COW co blocks x (CIWV*NB) ci blocks of the
// COB x CIB grid of 16x16 output quadrants and stages only those channels
// of dy and x.  Its 4 waves tile COW x CIWV x KS: a wave holds one co block
// against NB ci blocks (one dy fragment feeds NB*9 MFMAs), and KS waves
// share a quadrant by splitting the supertile's 32-position k-chunks; the
// k-split is merged in-block through LDS (fixed order), so a workgroup
// emits ONE partial row per quadrant it owns.  G = quadrants / owned
// workgroups form one supertile STREAM (grid-stride over supertiles):
//   C16: <1,1,1>  KS=4  G=1   block = the single quadrant, 4 k-chunks
//   C32: <2,1,1>  KS=2  G=2   block = both co blocks x one ci block
//   C64: <2,2,1>  KS=1  G=4   block = 2 x 2 quadrants, wave = quadrant
// picked by measurement among the splits the template allows (one block
// per stream with NB = CIB included): profiles/wrw2_notes.md.
//
// Partials are quadrant-local, part[q*RQ + stream][9*16*16] fp32 (RQ =
// streams).  The launcher keeps the stream count low (few, long streams:
// every stream costs one fp32 copy of dw), so ONE conv3x3_wrw2_final_k sums
// a quadrant's rows, casts and scatters into dw[co][kh][kw][ci]
// (channels_last memory order).  No atomics: the result is deterministic.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"
#include <hip/hip_bf16.h>

// bf16x8 / f32x4 from convwrw.h (same TU)

template <int CO, int CI, int W, int COW, int CIWV, int NB>
struct Wrw2Cfg {
  static constexpr int SPOS = (W == 8) ? 64 : 128;   // positions/supertile
  static constexpr int SR = SPOS / W;                // image rows
  static constexpr int CH = SPOS / 32;               // 32-pos k-chunks
  static constexpr int XR = SR + 2;
  static constexpr int XCP = (W + 2 + 7) & ~7;       // padded row stride
  // plane strides: multiples of 8 elements (aligned b128) with
  // (stride/2) % 8 == 4 so 16 consecutive planes hit distinct banks
  static constexpr int SXR = XR * XCP;
  static constexpr int SX = (SXR % 16 == 8) ? SXR : ((SXR & ~15) + 8 +
                            ((SXR % 16 > 8) ? 16 : 0));
  static constexpr int SD = (SPOS % 16 == 8) ? SPOS : SPOS + 8;
  static constexpr int COB = CO / 16, CIB = CI / 16;
  static constexpr int Q = COB * CIB;
  static constexpr int KS = 4 / (COW * CIWV);        // wave k-splits
  static constexpr int BCO = COW * 16;               // staged dy channels
  static constexpr int BCI = CIWV * NB * 16;         // staged x channels
  static constexpr int CIG = CI / BCI;               // ci groups
  static constexpr int G = (CO / BCO) * CIG;         // blocks per stream
  static constexpr int SLOTS = COW * CIWV * NB;      // quadrants per block
  static constexpr int STAGE_B = (BCO * SD + BCI * SX) * 2;
  static constexpr int MERGE_B = (KS > 1) ? SLOTS * 36 * WAVE * 4 : 0;
  static constexpr int LDS_B = STAGE_B > MERGE_B ? STAGE_B : MERGE_B;
  static_assert(COW * CIWV * KS == 4 && CH % KS == 0, "wave split");
  static_assert(CO % BCO == 0 && CI % BCI == 0, "block split");
};

template <int CO, int CI, int W, int COW, int CIWV, int NB>
__global__ void __launch_bounds__(FT_BLOCK) conv3x3_wrw2_k(
    const __hip_bfloat16* __restrict__ dy, const __hip_bfloat16* __restrict__ x,
    float* __restrict__ part, int N, int H, int RQ) {
  using C = Wrw2Cfg<CO, CI, W, COW, CIWV, NB>;
  // one LDS object: the staging slabs, reused by the k-split merge once
  // the last supertile is consumed
  __shared__ __attribute__((aligned(16))) unsigned char smem[C::LDS_B];
  __hip_bfloat16* s_dyT = reinterpret_cast<__hip_bfloat16*>(smem);
  __hip_bfloat16* s_xT = s_dyT + C::BCO * C::SD;

  const int tid = threadIdx.x;
  const int wave = tid / WAVE, lane = tid & (WAVE - 1);
  const int fm = lane & 15, kg = lane >> 4;
  const int cow = wave % COW, ciw = (wave / COW) % CIWV;
  const int ksp = wave / (COW * CIWV);

  const int g = (C::G > 1) ? (int)(blockIdx.x % C::G) : 0;
  const int bstream = blockIdx.x / C::G;
  const int nstreams = gridDim.x / C::G;
  const int co0 = (g / C::CIG) * C::BCO;      // first dy channel staged
  const int ci0 = (g % C::CIG) * C::BCI;      // first x channel staged

  // zero the x halo/padding once: body writes cover cols [1..W] of rows
  // [0..XR); everything else must read as 0 for every supertile
  for (int e = tid; e < C::BCI * C::SX / 8; e += FT_BLOCK)
    *reinterpret_cast<uint4*>(&s_xT[(long)e * 8]) = uint4{0, 0, 0, 0};

  f32x4 acc[NB][9];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[b][t] = {0.f, 0.f, 0.f, 0.f};

  const int tiles_per_img = H / C::SR;
  const long tiles = (long)N * tiles_per_img;
  __syncthreads();

  // Staging is split into a global->register load and a register->LDS
  // transposing store so all of a thread's loads (NDY + NX 16 B chunks) are
  // in flight together.  Issuing the loads of supertile t+1 before t's
  // MFMAs measured no faster (profiles/wrw2_notes.md), so it is not done.
  constexpr int CHK_DY = C::SPOS * C::BCO / 8;
  constexpr int CHK_X = C::XR * W * C::BCI / 8;
  constexpr int NDY = (CHK_DY + FT_BLOCK - 1) / FT_BLOCK;
  constexpr int NX = (CHK_X + FT_BLOCK - 1) / FT_BLOCK;
  uint4 rdy[NDY], rx[NX];

  auto load_tile = [&](long tg) {
    const int n = (int)(tg / tiles_per_img);
    const int h0 = (int)(tg % tiles_per_img) * C::SR;
    const __hip_bfloat16* dyp = dy + (((long)n * H + h0) * W) * CO + co0;
#pragma unroll
    for (int i = 0; i < NDY; ++i) {
      const int e = tid + i * FT_BLOCK;
      const int pos = e * 8 / C::BCO, c8 = (e * 8) % C::BCO;
      if (CHK_DY % FT_BLOCK == 0 || e < CHK_DY)
        rdy[i] = *reinterpret_cast<const uint4*>(dyp + (long)pos * CO + c8);
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int e = tid + i * FT_BLOCK;
      const int rowe = e * 8 / (W * C::BCI);
      const int rem = (e * 8) % (W * C::BCI);
      const int col = rem / C::BCI, c8 = rem % C::BCI;
      const int hh = h0 - 1 + rowe;
      rx[i] = uint4{0, 0, 0, 0};               // rows outside the image
      if ((CHK_X % FT_BLOCK == 0 || e < CHK_X) && hh >= 0 && hh < H)
        rx[i] = *reinterpret_cast<const uint4*>(
            x + (((long)n * H + hh) * W + col) * CI + ci0 + c8);
    }
  };
  // [pos][co0 + c] -> s_dyT[c][pos];  x with halo -> s_xT[c][row*XCP+col+1]
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < NDY; ++i) {
      const int e = tid + i * FT_BLOCK;
      const int pos = e * 8 / C::BCO, c8 = (e * 8) % C::BCO;
      const __hip_bfloat16* vp =
          reinterpret_cast<const __hip_bfloat16*>(&rdy[i]);
      if (CHK_DY % FT_BLOCK == 0 || e < CHK_DY) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          s_dyT[(long)(c8 + j) * C::SD + pos] = vp[j];
      }
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int e = tid + i * FT_BLOCK;
      const int rowe = e * 8 / (W * C::BCI);
      const int rem = (e * 8) % (W * C::BCI);
      const int col = rem / C::BCI, c8 = rem % C::BCI;
      const __hip_bfloat16* vp =
          reinterpret_cast<const __hip_bfloat16*>(&rx[i]);
      if (CHK_X % FT_BLOCK == 0 || e < CHK_X) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          s_xT[(long)(c8 + j) * C::SX + rowe * C::XCP + col + 1] = vp[j];
      }
    }
  };

  for (long tg = bstream; tg < tiles; tg += nstreams) {
    load_tile(tg);
    store_tile();
    __syncthreads();

    // ---- MFMAs ----------------------------------------------------------
#pragma unroll
    for (int i = 0; i < C::CH / C::KS; ++i) {
      const int chunk = ksp + i * C::KS;
      const int pb = chunk * 32 + kg * 8;       // this lane's 8 positions
      const int r0 = pb / W, w0 = pb % W;
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(
          &s_dyT[(long)(cow * 16 + fm) * C::SD + pb]);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int dh = 0; dh < 3; ++dh) {
          // 16-position aligned window of this (ci, row): the dw=0/1/2
          // fragments come out of these 8 dwords without further LDS reads
          const __hip_bfloat16* bp =
              &s_xT[(long)((ciw * NB + b) * 16 + fm) * C::SX +
                    (r0 + dh) * C::XCP + w0];
          typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
          const u32x4 lo = *reinterpret_cast<const u32x4*>(bp);
          const u32x4 hi = *reinterpret_cast<const u32x4*>(bp + 8);
          u32x4 f0 = lo;
          u32x4 f1, f2 = {lo.y, lo.z, lo.w, hi.x};
          f1.x = __builtin_amdgcn_alignbit(lo.y, lo.x, 16);
          f1.y = __builtin_amdgcn_alignbit(lo.z, lo.y, 16);
          f1.z = __builtin_amdgcn_alignbit(lo.w, lo.z, 16);
          f1.w = __builtin_amdgcn_alignbit(hi.x, lo.w, 16);
          acc[b][dh * 3 + 0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, __builtin_bit_cast(bf16x8, f0), acc[b][dh * 3 + 0], 0, 0, 0);
          acc[b][dh * 3 + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, __builtin_bit_cast(bf16x8, f1), acc[b][dh * 3 + 1], 0, 0, 0);
          acc[b][dh * 3 + 2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a, __builtin_bit_cast(bf16x8, f2), acc[b][dh * 3 + 2], 0, 0, 0);
        }
      }
    }
    __syncthreads();  // slab consumed; next supertile may overwrite
  }

  // ---- k-split merge: the KS waves of a quadrant hold k-chunk partials of
  // the SAME outputs; waves ksp = 1..KS-1 hand theirs to ksp = 0 through
  // the consumed slabs, one round each (fixed order), so the block emits
  // ONE row per quadrant
  if constexpr (C::KS > 1) {
    float* mb = reinterpret_cast<float*>(smem);
    const int slot0 = (cow * CIWV + ciw) * NB;
    for (int k = 1; k < C::KS; ++k) {
      if (k > 1) __syncthreads();             // round k-1 read out
      if (ksp == k) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              mb[(((slot0 + b) * 9 + t) * 4 + r) * WAVE + lane] =
                  acc[b][t][r];
      }
      __syncthreads();
      if (ksp == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              acc[b][t][r] +=
                  mb[(((slot0 + b) * 9 + t) * 4 + r) * WAVE + lane];
      }
    }
    if (ksp != 0) return;
  }

  // ---- partial rows: quadrant-local [9][16][16], row = stream ------------
  // D of mfma(a=dy, b=x): col = lane&15 maps the B operand's n index
  // (ci), rows map A's m (co): row = kg*4 + reg.
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int q = (co0 / 16 + cow) * C::CIB + ci0 / 16 + ciw * NB + b;
    float* pr = part + ((long)q * RQ + bstream) * (9 * 16 * 16);
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        pr[t * 256 + (kg * 4 + r) * 16 + fm] = acc[b][t][r];
  }
}

// part[q*RQ + r][9*16*16] fp32 -> dw bf16 [co][kh][kw][ci] in ONE kernel
// (shared with the stride-2 wrw of convs2bwd.h, same partial layout): the
// launchers keep RQ small (few, long supertile streams), so a block of CW
// columns x 256/CW row slices sums a quadrant's rows directly; no stripe
// buffer, no separate cast pass.  CW trades line use (32 columns = one
// 128 B line per row) against blocks in flight (Q * 2304/CW): the small-Q
// shapes take a narrower block to cover the chip.  Fixed summation order.
template <int CW>
__global__ void __launch_bounds__(FT_BLOCK) conv3x3_wrw2_final_k(
    const float* __restrict__ part, int RQ, __hip_bfloat16* __restrict__ dw,
    int CI) {
  constexpr int RS = FT_BLOCK / CW;           // row slices
  constexpr int BPQ = 9 * 256 / CW;           // blocks per quadrant
  __shared__ float lds[RS][CW];
  const int c = threadIdx.x % CW, rs = threadIdx.x / CW;
  const int q = blockIdx.x / BPQ;
  const int lc = (blockIdx.x % BPQ) * CW + c;
  const float* p = part + (long)q * RQ * (9 * 256) + lc;
  float s = 0.f;
#pragma unroll 4
  for (int r = rs; r < RQ; r += RS) s += p[(long)r * (9 * 256)];
  lds[rs][c] = s;
  __syncthreads();
  if (rs == 0) {
    s = 0.f;
#pragma unroll
    for (int i = 0; i < RS; ++i) s += lds[i][c];
    const int tap = lc / 256, mrow = (lc % 256) / 16, ncol = lc % 16;
    const int co = (q / (CI / 16)) * 16 + mrow;
    const int ci = (q % (CI / 16)) * 16 + ncol;
    dw[((long)co * 9 + tap) * CI + ci] = __float2bfloat16(s);
  }
}
