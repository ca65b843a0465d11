// Parameter-gradient reduce of the token-input char-GRU (gru_tok_grads): ONE
// launch produces the three sums over the R = B*T rows that follow gru_bwd /
// gru_wide_bwd when the layer's input is a token id (gru.h, TOK variant):
//
//   dW_hh[c][k] = sum_r dgh[r][c] * h_prev[r][k]          [3H, H]
//   db_hh[c]    = sum_r dgh[r][c]                         [3H]
//   dP[v][c]    = sum_{r : tok[r] == v} dgx[r][c]         [V, 3H]
//
// with r = b*T + t and h_prev[r] = h0[b] at t == 0, else out[b, t-1] -- the
// row before r in `out`; it is addressed here, never concatenated.
//
// Work split.  Every 16x16 output tile is one workgroup, and a workgroup owns
// its tile for ALL of K = R, so there are no partial buffers, no second launch
// and no atomics.  Two roles by block index, both on v_mfma_f32_16x16x4_f32
// (lane l holds A[row l&15][k l>>4], B[k l>>4][col l&15] and
// C[row 4*(l>>4)+i][col l&15]):
//
//   dW role  ceil(3H/16) x ceil(H/16) blocks.  A = dgh read transposed (lane
//            reads dgh[r0 + lk][c0 + lr]: 16 consecutive floats per k), B =
//            h_prev[r0 + lk][n0 + lr].  The blocks of hidden tile 0 also run
//            the same A against B = 1: every column of that accumulator is
//            db_hh, column 0 is stored.
//   dP role  ceil(V/16) x ceil(3H/16) blocks.  A is the one-hot
//            (tok[r0 + lk] == v0 + lr) ? 1 : 0 built in registers from the
//            token load, B = dgx[r0 + lk][c0 + lr].  A 1/0 multiplier in an
//            fp32 FMA chain adds a selected term exactly and an unselected one
//            as +0, so the segmented sum is an ordered fp32 sum without
//            sorting.  A token outside [0, V) matches no row and contributes
//            nothing; a vocabulary row no token selects is exact zeros.
//            Caveat: 0 * inf is NaN, so an infinite (or NaN) dgx[r][c] makes
//            column c of EVERY row of its tile NaN, not only row tok[r].
//
// K split.  The NW waves of a workgroup take the 4-row k-steps round robin
// (wave w: steps w, w + NW, ...; four steps' loads are issued before their
// four MFMAs), then waves 1.. leave their accumulators in LDS and wave 0 adds
// them in wave order and stores.  The summation order is fixed by the shapes
// and NW, so two runs are bit-identical.  No host reads: capture-safe.
//
// Bounds: rows >= R, columns >= 3H / H / V are never loaded (their operand is
// 0) and never stored; every element of the three outputs is written.
#pragma once
#include <hip/hip_runtime.h>
#include "gru.h"

#define GRU_TOK_MAXW 16   // waves per workgroup
#define GRU_TOK_U 4       // k-steps in flight per wave

// ROLE 0: dW_hh (+ db_hh when WITH_DB), ROLE 1: dP.  Accumulates this wave's
// k-steps of tile (row0, col0) into acc (and accb).
template <int ROLE, bool WITH_DB>
__device__ __forceinline__ GRU_SCALAR_F32 void gru_tok_acc(
    gru_f4& acc, gru_f4& accb, const float* __restrict__ am,
    const float* __restrict__ out, const float* __restrict__ h0,
    const long* __restrict__ tok, long R, int T, int H, int arow, bool a_ok,
    int bcol, bool b_ok, int wid, int nw, int lk) {
  const int H3 = 3 * H;
  const long nsteps = (R + 3) >> 2;
  for (long s = wid; s < nsteps; s += (long)GRU_TOK_U * nw) {
    float a[GRU_TOK_U], b[GRU_TOK_U];
#pragma unroll
    for (int u = 0; u < GRU_TOK_U; ++u) {
      const long r = 4 * (s + (long)u * nw) + lk;
      const bool in = r < R;
      if (ROLE == 0) {
        a[u] = (in && a_ok) ? am[r * H3 + arow] : 0.f;
        float hv = 0.f;
        if (in && b_ok) {
          const long bb = r / T;
          hv = (r == bb * T) ? h0[bb * H + bcol] : out[(r - 1) * H + bcol];
        }
        b[u] = hv;
      } else {
        a[u] = (in && a_ok && tok[r] == (long)arow) ? 1.f : 0.f;
        b[u] = (in && b_ok) ? am[r * H3 + bcol] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < GRU_TOK_U; ++u) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u], acc, 0, 0, 0);
      if (WITH_DB)
        accb = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], 1.f, accb, 0, 0, 0);
    }
  }
}

// grid ceil(3H/16)*ceil(H/16) + ceil(V/16)*ceil(3H/16), block 64*NW with
// 1 <= NW <= GRU_TOK_MAXW.  dgx, dgh [R, 3H]; out [R, H]; h0 [B, H]; tok [R].
__global__ void __launch_bounds__(GRU_TOK_MAXW * WAVE) GRU_SCALAR_F32
gru_tok_grads_k(const float* __restrict__ dgx, const float* __restrict__ dgh,
                const float* __restrict__ out, const float* __restrict__ h0,
                const long* __restrict__ tok, float* __restrict__ dP,
                float* __restrict__ dW, float* __restrict__ db, long R, int T,
                int H, int V) {
  __shared__ float red[GRU_TOK_MAXW - 1][2][4][WAVE];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wid = tid / WAVE;
  const int nw = blockDim.x / WAVE;
  const int lr = lane & 15, lk = lane >> 4;
  const int H3 = 3 * H;
  const int MT = (H3 + 15) / 16, NTH = (H + 15) / 16;
  const int bid = blockIdx.x;
  const bool role_w = bid < MT * NTH;   // block-uniform

  gru_f4 acc = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
  int row0, col0;                       // tile origin in its output
  bool with_db = false;
  if (role_w) {
    row0 = (bid / NTH) * 16;
    col0 = (bid % NTH) * 16;
    with_db = col0 == 0;
    const int c = row0 + lr, n = col0 + lr;
    if (with_db)
      gru_tok_acc<0, true>(acc, accb, dgh, out, h0, tok, R, T, H, c, c < H3,
                           n, n < H, wid, nw, lk);
    else
      gru_tok_acc<0, false>(acc, accb, dgh, out, h0, tok, R, T, H, c, c < H3,
                            n, n < H, wid, nw, lk);
  } else {
    const int id = bid - MT * NTH;
    row0 = (id / MT) * 16;
    col0 = (id % MT) * 16;
    const int v = row0 + lr, c = col0 + lr;
    gru_tok_acc<1, false>(acc, accb, dgx, out, h0, tok, R, T, H, v, v < V, c,
                          c < H3, wid, nw, lk);
  }

  // merge over the waves, in wave order
  if (wid > 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      red[wid - 1][0][i][lane] = acc[i];
      red[wid - 1][1][i][lane] = accb[i];
    }
  }
  __syncthreads();
  if (wid > 0) return;
  for (int w = 0; w + 1 < nw; ++w) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[i] += red[w][0][i][lane];
      accb[i] += red[w][1][i][lane];
    }
  }

  const int nrow = role_w ? H3 : V, ncol = role_w ? H : H3;
  float* dst = role_w ? dW : dP;
  const int cc = col0 + lr;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rr = row0 + 4 * lk + i;
    if (rr < nrow) {
      if (cc < ncol) dst[(long)rr * ncol + cc] = acc[i];
      if (with_db && lr == 0) db[rr] = accb[i];
    }
  }
}
