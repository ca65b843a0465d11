// Local SGD steps of packed LeNet-style CNN clients, batched per layer: every
// kernel's grid has a client dimension, the weights are read from (and
// updated in) the [C, N] replica arena -- the scheme of mlpround.h, whose
// round-begin / snapshot kernel (mlp_rows_k), row helper, 32x32 tiles, head
// kernel and SGD update (mlp_sgd / mlp_update<false>) are used as they are.
//
// The model (components/models/cnn.py): conv 5x5 / stride 1 / no padding +
// bias, ReLU, max-pool 2/2, twice; then fc1 + ReLU and fc2, mean softmax
// cross-entropy.  S1 = (S - 4) / 2, S2 = (S1 - 4) / 2, O2 = S1 - 4.
//
//   for each client c with steps[c] > 0 (others: nothing read or written):
//     replicas[c] <- server                                  mlp_rows_k(0)
//     for s in 0 .. steps[c]-1, rows r = idx[c, s, :] >= 0, n = #rows:
//       [snap[c] <- replicas[c]  if s + 1 == k_cut]          mlp_rows_k(1)
//       p1 = pool(relu(conv(x,  W1) + b1)), argmax           cnn_conv1_fwd_k
//       p2 = pool(relu(conv(p1, W2) + b2)), argmax           cnn_conv2_fwd_k
//       a  = relu(flat(p2) Wf1^T + bf1)                      cnn_fc1_fwd_k
//       logits = a Wf2^T + bf2 ; loss[c, s] ; dlogits / n    mlp_head_k<true>
//       da = dl Wf2 ; SGD on Wf2, bf2 ; dz1 = da [a > 0] ;   cnn_fc_bwd_k<true>
//         SGD on bf1
//       dp2 = dz1 Wf1 ; SGD on Wf1                           cnn_fc_bwd_k<false>
//       dp1 = dgrad(dz2, W2), dz2 = dp2 through the argmax   cnn_conv2_dgrad_k
//       dW2 = wrw(dz2, p1), db2 ; SGD on W2, b2              cnn_conv2_wrw_k
//       dW1 = wrw(dz1c, x), db1 ; SGD on W1, b1              cnn_conv1_wrw_k
//     mom_init[c] <- 1 (with momentum)                       mlp_rows_k(2)
//
// 9 launches per step, 256 threads each.  Every kernel takes the step s and
// returns at once, uniformly, for a client with s >= steps[c].
//
// A pooled element keeps one byte: the position 2 dy + dx of the FIRST
// maximum of its window in (row, column) scan order, or 4 when that maximum
// is <= 0 (the ReLU mask z > 0 passes nothing).  dz of a conv output is the
// pooled gradient at that position and zero at the other three.
//
// conv2's three products are implicit GEMMs on v_mfma_f32_16x16x4_f32 (lane l
// of a wave holds A[row l&15][k l>>4], B[k l>>4][col l&15] and the
// accumulator elements C[row 4 (l>>4) + i][col l&15]); bit-for-bit a
// k-ordered fmaf chain:
//   forward  M = 4 S2^2 conv pixels of one sample, ordered (window, position)
//            so that the four accumulators of a lane are one pool window;
//            N = 16 output channels of the block; K = 25 C1 in the arena's own
//            element order (either weight order: a table maps k to the LDS
//            offset of its tap), the block's filter slab [K, 16] in LDS.
//   dgrad    M = S1^2 pixels of one sample, N = 16 input channels, K = 25 C2
//            in chunks of 8 output channels: dz2 of the chunk zero-padded by
//            4 in LDS, the filter chunk [200, 16] beside it.
//   wrw      M = C2 (one 16-row tile per wave), N = 64 of the 25 C1 filter
//            elements per block, K = the O2^2 pixels of a sample, the samples
//            in order; dz2 dense in LDS (odd row stride), p1 of the sample
//            beside it.  The update runs from the accumulators.
// Pad rows / columns / k are zeros in LDS (or clamped to a valid address and
// discarded); nothing is read out of range.  conv1 (K = 25 Cin <= 100) and
// its weight gradient (one term per pool window) are scalar; the fc layers
// use the 32x32 scalar tiles of mlpround.h (at most 64 rows: they are bound
// by the weight and momentum traffic, not by arithmetic).
//
// The weight of a conv sits in the arena as [co][ci][kh][kw] or, nhwc, as
// [co][kh][kw][ci]; element (co, j) of either is at w + co * 25 Cg + j and
// cnn_tap() decodes j.
//
// No atomics; every summation order is fixed by the shapes, so two runs are
// bit-identical.  No host reads: capture-safe.  Padding samples (idx < 0 or
// >= M) are never dereferenced, their workspace rows are never read, and
// they are excluded from n.  Only parameter elements of the rows of online
// clients are written (replicas: the whole row first).
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"
#include "mlpround.h"

#define CNNROUND_THREADS 256
#define CNNROUND_MAXB MLPROUND_MAXB
#define CNNROUND_MAXK MLPROUND_MAXK
#define CNNROUND_MAXCIN 4
#define CNNROUND_MAXS 32
#define CNNROUND_MAXC1 24
#define CNNROUND_MAXC2 64
#define CNNROUND_MAXH 4096
#define CNN_DG_CO 8             // output channels of a dgrad chunk
#define CNN_WRW_NT 4            // 16-column tiles of a wrw block

typedef float cnn_f4 __attribute__((ext_vector_type(4)));

struct CnnLayout {
  int Cin, S, C1, C2, H, K;
  int S1, S2, O2, F2;           // F2 = C2 S2^2: the features of fc1
  int w1, b1, nhwc1, w2, b2, nhwc2, fw1, fb1, fw2, fb2;   // arena offsets
  // workspace offsets (floats, per client; m.lay.ws_stride is the stride)
  int p1, p2, act, dl, dz1, dp2, dp1;
  // byte workspace offsets (per client)
  int am1, am2;
  long wsb_stride;
};

struct CnnRoundArgs {
  MlpRoundArgs m;               // operands, SGD, and the head's MlpLayout
  CnnLayout lay;
  unsigned char* wsb;           // [C, wsb_stride]: the argmax bytes
};

// element j of a filter's 25 Cg arena elements: channel ci and tap t = 5 kh +
// kw
__device__ __forceinline__ void cnn_tap(int nhwc, int j, int Cg, int& ci,
                                        int& t) {
  if (nhwc) { t = j / Cg; ci = j - t * Cg; }
  else { ci = j / 25; t = j - ci * 25; }
}

// ReLU + 2x2 max-pool of a window in scan order: the pooled value and the
// byte of the header comment
__device__ __forceinline__ float cnn_pool(float z0, float z1, float z2,
                                          float z3, unsigned char& code) {
  float m = z0;
  int k = 0;
  if (z1 > m) { m = z1; k = 1; }
  if (z2 > m) { m = z2; k = 2; }
  if (z3 > m) { m = z3; k = 3; }
  if (!(m > 0.f)) { m = 0.f; k = 4; }
  code = (unsigned char)k;
  return m;
}

// the row of sample b of (client, step), -1 for padding
__device__ __forceinline__ int cnn_row(const MlpRoundArgs& a, int c, int s,
                                       int b) {
  const int r = a.idx[((long)c * a.T + s) * a.B + b];
  return r >= a.M ? -1 : r;
}

// conv1 + bias + ReLU + pool of sample blockIdx.y.  grid = (C, B).
__global__ void __launch_bounds__(CNNROUND_THREADS)
cnn_conv1_fwd_k(const CnnRoundArgs a, int s) {
  __shared__ float img[CNNROUND_MAXCIN * CNNROUND_MAXS * CNNROUND_MAXS];
  __shared__ float Wf[CNNROUND_MAXC1 * 25 * CNNROUND_MAXCIN];
  const int c = blockIdx.x, b = blockIdx.y;
  if (s >= mlp_nsteps(a.m, c)) return;
  const int r = cnn_row(a.m, c, s, b);
  if (r < 0) return;
  const CnnLayout& L = a.lay;
  const int tid = threadIdx.x;
  const int Cin = L.Cin, S = L.S, C1 = L.C1, S1 = L.S1, nt = 25 * Cin;
  const float* P = a.m.replicas + (long)c * a.m.N;
  const float* x = a.m.X + (long)r * Cin * S * S;
  for (int e = tid; e < Cin * S * S; e += CNNROUND_THREADS) img[e] = x[e];
  for (int e = tid; e < C1 * nt; e += CNNROUND_THREADS) {
    const int co = e / nt;
    int ci, t;
    cnn_tap(L.nhwc1, e - co * nt, Cin, ci, t);
    Wf[co * nt + ci * 25 + t] = P[L.w1 + e];
  }
  __syncthreads();
  const int nw = S1 * S1;
  float* p1 = a.m.ws + (long)c * a.m.lay.ws_stride + L.p1 + (long)b * C1 * nw;
  unsigned char* am = a.wsb + (long)c * L.wsb_stride + L.am1 + (long)b * C1 * nw;
  for (int e = tid; e < C1 * nw; e += CNNROUND_THREADS) {
    const int co = e / nw, win = e - co * nw;
    const int ph = win / S1, pw = win - ph * S1;
    float z0 = 0.f, z1 = 0.f, z2 = 0.f, z3 = 0.f;
    for (int ci = 0; ci < Cin; ++ci) {
      const float* ip = img + ci * S * S + 2 * ph * S + 2 * pw;
      const float* wp = Wf + co * nt + ci * 25;
      float pt[6][6];
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) pt[i][j] = ip[i * S + j];
#pragma unroll
      for (int kh = 0; kh < 5; ++kh)
#pragma unroll
        for (int kw = 0; kw < 5; ++kw) {
          const float w = wp[kh * 5 + kw];
          z0 = fmaf(pt[kh][kw], w, z0);
          z1 = fmaf(pt[kh][kw + 1], w, z1);
          z2 = fmaf(pt[kh + 1][kw], w, z2);
          z3 = fmaf(pt[kh + 1][kw + 1], w, z3);
        }
    }
    const float bias = P[L.b1 + co];
    unsigned char code;
    p1[e] = cnn_pool(z0 + bias, z1 + bias, z2 + bias, z3 + bias, code);
    am[e] = code;
  }
}

// conv2 + bias + ReLU + pool: the block's 16 output channels, samples
// blockIdx.z, + gridDim.z, ...  grid = (C, ceil(C2 / 16), Z); dynamic LDS:
// Wt [Kp][16], Ps [C1 S1^2], koff [Kp], Kp = 25 C1 rounded up to 4.
__global__ void __launch_bounds__(CNNROUND_THREADS)
cnn_conv2_fwd_k(const CnnRoundArgs a, int s) {
  extern __shared__ float cnn_smem[];
  const int c = blockIdx.x;
  if (s >= mlp_nsteps(a.m, c)) return;
  const CnnLayout& L = a.lay;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int C1 = L.C1, C2 = L.C2, S1 = L.S1, S2 = L.S2;
  const int K2 = 25 * C1, Kp = (K2 + 3) & ~3, np1 = C1 * S1 * S1;
  float* Wt = cnn_smem;
  float* Ps = Wt + Kp * 16;
  int* koff = (int*)(Ps + np1);
  const int co0 = blockIdx.y * 16;
  const float* P = a.m.replicas + (long)c * a.m.N;
  const float* W = P + L.w2;
  for (int e = tid; e < Kp * 16; e += CNNROUND_THREADS) {
    const int col = e / Kp, k = e - col * Kp;
    float v = 0.f;
    if (k < K2 && co0 + col < C2) v = W[(long)(co0 + col) * K2 + k];
    Wt[k * 16 + col] = v;
  }
  for (int k = tid; k < Kp; k += CNNROUND_THREADS) {
    int o = 0;                  // k >= K2: any valid tap, its Wt row is zero
    if (k < K2) {
      int ci, t;
      cnn_tap(L.nhwc2, k, C1, ci, t);
      o = ci * S1 * S1 + (t / 5) * S1 + t % 5;
    }
    koff[k] = o;
  }
  const int nwin = S2 * S2, ntile = (nwin + 3) / 4;
  const bool cok = co0 + lr < C2;
  const float bias = cok ? P[L.b2 + co0 + lr] : 0.f;
  float* ws = a.m.ws + (long)c * a.m.lay.ws_stride;
  unsigned char* wsb = a.wsb + (long)c * L.wsb_stride;
  for (int b = blockIdx.z; b < a.m.B; b += gridDim.z) {
    const int r = cnn_row(a.m, c, s, b);
    __syncthreads();            // the last sample's reads of Ps
    if (r >= 0) {
      const float* p1 = ws + L.p1 + (long)b * np1;
      for (int e = tid; e < np1; e += CNNROUND_THREADS) Ps[e] = p1[e];
    }
    __syncthreads();
    if (r < 0) continue;
    for (int mt = w; mt < ntile; mt += 4) {
      // row lr of the tile: window 4 mt + lr / 4, position lr % 4
      const int win = min(mt * 4 + (lr >> 2), nwin - 1), q = lr & 3;
      const int ph = win / S2, pw = win - ph * S2;
      const float* ap = Ps + (2 * ph + (q >> 1)) * S1 + 2 * pw + (q & 1);
      cnn_f4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int k = lk; k < Kp; k += 4)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[koff[k]],
                                                   Wt[k * 16 + lr], acc, 0,
                                                   0, 0);
      // the lane's accumulators: the window 4 mt + lk of channel co0 + lr
      const int wi = mt * 4 + lk;
      if (wi < nwin && cok) {
        unsigned char code;
        const float v = cnn_pool(acc[0] + bias, acc[1] + bias, acc[2] + bias,
                                 acc[3] + bias, code);
        const long o = (long)b * L.F2 + (co0 + lr) * nwin + wi;
        ws[L.p2 + o] = v;
        wsb[L.am2 + o] = code;
      }
    }
  }
}

// fc1 + bias + ReLU for the tile blockIdx.y of its output columns.
// grid = (C, ceil(H / 32)).
__global__ void __launch_bounds__(CNNROUND_THREADS)
cnn_fc1_fwd_k(const CnnRoundArgs a, int s) {
  __shared__ float As[MLPROUND_MAXB * MLP_LD];
  __shared__ float Ws[MLP_TN * MLP_LD];
  __shared__ int rid[MLPROUND_MAXB];
  const int c = blockIdx.x;
  if (s >= mlp_nsteps(a.m, c)) return;
  const CnnLayout& L = a.lay;
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int j0 = blockIdx.y * MLP_TN;
  mlp_rows(a.m, c, s, rid);
  const float* P = a.m.replicas + (long)c * a.m.N;
  float* ws = a.m.ws + (long)c * a.m.lay.ws_stride;
  float acc[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) acc[m] = 0.f;
  for (int k0 = 0; k0 < L.F2; k0 += MLP_TN) {
    mlp_load_a<false>(As, ws + L.p2, L.F2, k0, L.F2, rid);
    mlp_load_w<false>(Ws, P + L.fw1, j0, L.H, k0, L.F2);
    __syncthreads();
    mlp_fma_tile(acc, As, Ws);
    __syncthreads();
  }
  const int col = j0 + tx;
  if (col >= L.H) return;
  const float bias = P[L.fb1 + col];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int b = ty + 8 * m;
    if (b >= a.m.B) break;
    ws[L.act + (long)b * L.H + col] =
        rid[b] >= 0 ? fmaxf(acc[m] + bias, 0.f) : 0.f;
  }
}

// backward through a boundary of the fc stack, for the tile blockIdx.y of the
// columns below it (mlp_bwd_k without BatchNorm):
//   TOP   fc2 | fc1: M = Wf2 [K, H]; da = dl M ; SGD on M[:, tile] ;
//         dz1 = da [a > 0] ; SGD on bf1[tile] ; block 0: SGD on bf2.
//   !TOP  fc1 | p2:  M = Wf1 [H, F2]; dp2 = dz1 M ; SGD on M[:, tile].
// The block owns the column slab of M, so dgrad sees pre-update weights.
template <bool TOP>
__global__ void __launch_bounds__(CNNROUND_THREADS)
cnn_fc_bwd_k(const CnnRoundArgs a, int s) {
  __shared__ float As[MLPROUND_MAXB * MLP_LD];   // dz_M chunk, later dz1
  __shared__ float Ws[MLP_TN * MLP_LD];          // M chunk (pre-update)
  __shared__ float At[MLPROUND_MAXB * MLP_LD];   // the tile of a / p2
  __shared__ int rid[MLPROUND_MAXB];
  const int c = blockIdx.x;
  if (s >= mlp_nsteps(a.m, c)) return;
  const CnnLayout& L = a.lay;
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int j0 = blockIdx.y * MLP_TN;
  mlp_rows(a.m, c, s, rid);
  const MlpSgd u = mlp_sgd<false>(a.m, c, s);
  const MlpCorr k0 = {0.f, 0.f};
  float* ws = a.m.ws + (long)c * a.m.lay.ws_stride;
  const int ncol = TOP ? L.H : L.F2, nO = TOP ? L.K : L.H;
  const int m_off = TOP ? L.fw2 : L.fw1;
  const float* dzM = ws + (TOP ? L.dl : L.dz1);
  const int col = j0 + tx;
  const bool cin = col < ncol;

  mlp_load_a<false>(At, ws + (TOP ? L.act : L.p2), ncol, j0, ncol, rid);
  float acc[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) acc[m] = 0.f;
  for (int o0 = 0; o0 < nO; o0 += MLP_TN) {
    mlp_load_a<false>(As, dzM, nO, o0, nO, rid);
    mlp_load_w<true>(Ws, u.p + m_off, j0, ncol, o0, nO);
    __syncthreads();
    mlp_fma_tile(acc, As, Ws);
    // weight gradient of M[o0 + oo][col], oo = ty + 8 q, rows in order
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < a.m.B; ++b) {
      const float av = At[b * MLP_LD + tx];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        g[q] = fmaf(As[b * MLP_LD + ty + 8 * q], av, g[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int oo = ty + 8 * q;
      if (cin && o0 + oo < nO)
        mlp_update<false>(u, m_off + (o0 + oo) * ncol + col,
                          Ws[tx * MLP_LD + oo], g[q], k0);
    }
    __syncthreads();
  }
  if (!TOP) {
    float* dp2 = ws + L.dp2;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int b = ty + 8 * m;
      if (b < a.m.B && cin) dp2[(long)b * ncol + col] = acc[m];
    }
    return;
  }
  float* dz1 = ws + L.dz1;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int b = ty + 8 * m;
    const float v = At[b * MLP_LD + tx] > 0.f ? acc[m] : 0.f;
    As[b * MLP_LD + tx] = v;
    if (b < a.m.B && cin) dz1[(long)b * ncol + col] = v;
  }
  __syncthreads();
  if (tid < MLP_TN && j0 + tid < ncol) {     // dbf1 = sum of dz1 over the rows
    const int e = L.fb1 + j0 + tid;
    float sb = 0.f;
    for (int b = 0; b < a.m.B; ++b) sb += As[b * MLP_LD + tid];
    mlp_update<false>(u, e, u.p[e], sb, k0);
  }
  if (blockIdx.y == 0) {                     // dbf2 = sum of dl over the rows
    for (int k = tid; k < L.K; k += CNNROUND_THREADS) {
      float sb = 0.f;
      for (int b = 0; b < a.m.B; ++b)
        if (rid[b] >= 0) sb += dzM[(long)b * L.K + k];
      mlp_update<false>(u, L.fb2 + k, u.p[L.fb2 + k], sb, k0);
    }
  }
}

// the four conv-output gradients of pool window (ph, pw) of a channel: v at
// the argmax position, zero at the others, into a dense map of row stride ld
__device__ __forceinline__ void cnn_put_window(float* d, int ld, int ph,
                                               int pw, int code, float v) {
  float* q = d + 2 * ph * ld + 2 * pw;
  q[0] = code == 0 ? v : 0.f;
  q[1] = code == 1 ? v : 0.f;
  q[ld] = code == 2 ? v : 0.f;
  q[ld + 1] = code == 3 ? v : 0.f;
}

// conv2 dgrad of sample blockIdx.z for the block's 16 input channels:
// dp1[b, ci, y, x] = sum_{co, kh, kw} dz2[b, co, y - kh, x - kw] W2[co, ci,
// kh, kw].  grid = (C, ceil(C1 / 16), B); dynamic LDS: Dz [8][(S1 + 4)^2],
// Wc [200][16], koff [200].
__global__ void __launch_bounds__(CNNROUND_THREADS)
cnn_conv2_dgrad_k(const CnnRoundArgs a, int s) {
  extern __shared__ float cnn_smem[];
  const int c = blockIdx.x, b = blockIdx.z;
  if (s >= mlp_nsteps(a.m, c)) return;
  if (cnn_row(a.m, c, s, b) < 0) return;
  const CnnLayout& L = a.lay;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int C1 = L.C1, C2 = L.C2, S1 = L.S1, S2 = L.S2;
  const int K2 = 25 * C1, P2 = S1 + 4, PP = P2 * P2;
  const int KC = 25 * CNN_DG_CO;
  float* Dz = cnn_smem;
  float* Wc = Dz + CNN_DG_CO * PP;
  int* koff = (int*)(Wc + KC * 16);
  const int ci0 = blockIdx.y * 16;
  const float* W = a.m.replicas + (long)c * a.m.N + L.w2;
  const float* ws = a.m.ws + (long)c * a.m.lay.ws_stride;
  const float* dp2 = ws + L.dp2 + (long)b * L.F2;
  const unsigned char* am =
      a.wsb + (long)c * L.wsb_stride + L.am2 + (long)b * L.F2;
  for (int k = tid; k < KC; k += CNNROUND_THREADS) {
    const int col = k / 25, t = k - col * 25;
    koff[k] = col * PP - (t / 5) * P2 - t % 5;
  }
  // the border of 4 stays zero; the interior is rewritten per chunk
  for (int e = tid; e < CNN_DG_CO * PP; e += CNNROUND_THREADS) Dz[e] = 0.f;
  const int np = S1 * S1, ntile = (np + 15) / 16, nwin = S2 * S2;
  int pix[4];
  cnn_f4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = min((w + 4 * j) * 16 + lr, np - 1);
    const int y = m / S1;
    pix[j] = (y + 4) * P2 + (m - y * S1) + 4;
    acc[j] = cnn_f4{0.f, 0.f, 0.f, 0.f};
  }
  for (int cc = 0; cc < C2; cc += CNN_DG_CO) {
    __syncthreads();            // the last chunk's reads; first: the zeros
    for (int e = tid; e < CNN_DG_CO * nwin; e += CNNROUND_THREADS) {
      const int col = e / nwin, win = e - col * nwin;
      const int ph = win / S2, pw = win - ph * S2;
      int code = 4;
      float v = 0.f;
      if (cc + col < C2) {
        code = am[(cc + col) * nwin + win];
        v = dp2[(cc + col) * nwin + win];
      }
      cnn_put_window(Dz + col * PP + 4 * P2 + 4, P2, ph, pw, code, v);
    }
    for (int e = tid; e < KC * 16; e += CNNROUND_THREADS) {
      int col, t, cl;           // lanes along the arena's contiguous index
      if (L.nhwc2) {
        cl = e & 15;
        col = (e >> 4) / 25;
        t = (e >> 4) - col * 25;
      } else {
        const int q = e / 25;
        t = e - q * 25;
        cl = q & 15;
        col = q >> 4;
      }
      const int co = cc + col, ci = ci0 + cl;
      float v = 0.f;
      if (co < C2 && ci < C1)
        v = W[(long)co * K2 + (L.nhwc2 ? t * C1 + ci : ci * 25 + t)];
      Wc[(col * 25 + t) * 16 + cl] = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (w + 4 * j >= ntile) continue;          // uniform in the wave
      const float* ap = Dz + pix[j];
      for (int k = lk; k < KC; k += 4)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            ap[koff[k]], Wc[k * 16 + lr], acc[j], 0, 0, 0);
    }
  }
  float* dp1 = a.m.ws + (long)c * a.m.lay.ws_stride + L.dp1 +
               (long)b * C1 * np;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = (w + 4 * j) * 16 + 4 * lk + i;
      if (m < np && ci0 + lr < C1) dp1[(ci0 + lr) * np + m] = acc[j][i];
    }
}

// conv2 weight and bias gradient and their update: wave w owns output
// channels 16 w .. 16 w + 15, the block the filter elements 64 blockIdx.y ..
// + 63 of every channel; the samples are summed in order.  Block 0 also
// updates b2.  grid = (C, ceil(25 C1 / 64)); dynamic LDS: Dz [64][O2^2 | 1],
// Ps [C1 S1^2], coff [64], ptab [O2^2], red [256].
__global__ void __launch_bounds__(CNNROUND_THREADS)
cnn_conv2_wrw_k(const CnnRoundArgs a, int s) {
  extern __shared__ float cnn_smem[];
  __shared__ int rid[MLPROUND_MAXB];
  const int c = blockIdx.x;
  if (s >= mlp_nsteps(a.m, c)) return;
  const CnnLayout& L = a.lay;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int C1 = L.C1, C2 = L.C2, S1 = L.S1, S2 = L.S2, O2 = L.O2;
  const int K2 = 25 * C1, npx = O2 * O2, LDA = npx | 1, np1 = C1 * S1 * S1;
  const int NC = 16 * CNN_WRW_NT;
  float* Dz = cnn_smem;
  float* Ps = Dz + CNNROUND_MAXC2 * LDA;
  int* coff = (int*)(Ps + np1);
  int* ptab = coff + NC;
  float* red = (float*)(ptab + npx);
  const int n0 = blockIdx.y * NC;
  mlp_rows(a.m, c, s, rid);
  const MlpSgd u = mlp_sgd<false>(a.m, c, s);
  const MlpCorr k0 = {0.f, 0.f};
  const float* ws = a.m.ws + (long)c * a.m.lay.ws_stride;
  const unsigned char* wsb = a.wsb + (long)c * L.wsb_stride;
  for (int j = tid; j < NC; j += CNNROUND_THREADS) {
    int o = 0;                  // n >= 25 C1: a valid tap, the column is dropped
    if (n0 + j < K2) {
      int ci, t;
      cnn_tap(L.nhwc2, n0 + j, C1, ci, t);
      o = ci * S1 * S1 + (t / 5) * S1 + t % 5;
    }
    coff[j] = o;
  }
  for (int k = tid; k < npx; k += CNNROUND_THREADS)
    ptab[k] = (k / O2) * S1 + k % O2;
  // rows of channels >= C2 stay zero
  for (int e = tid; e < CNNROUND_MAXC2 * LDA; e += CNNROUND_THREADS)
    Dz[e] = 0.f;
  __syncthreads();
  int cf[CNN_WRW_NT];
  cnn_f4 acc[CNN_WRW_NT];
#pragma unroll
  for (int j = 0; j < CNN_WRW_NT; ++j) {
    cf[j] = coff[16 * j + lr];
    acc[j] = cnn_f4{0.f, 0.f, 0.f, 0.f};
  }
  const int nwin = S2 * S2;
  for (int b = 0; b < a.m.B; ++b) {
    if (rid[b] < 0) continue;
    __syncthreads();            // the last sample's reads
    const float* p1 = ws + L.p1 + (long)b * np1;
    for (int e = tid; e < np1; e += CNNROUND_THREADS) Ps[e] = p1[e];
    const float* dp2 = ws + L.dp2 + (long)b * L.F2;
    const unsigned char* am = wsb + L.am2 + (long)b * L.F2;
    for (int e = tid; e < C2 * nwin; e += CNNROUND_THREADS) {
      const int co = e / nwin, win = e - co * nwin;
      const int ph = win / S2, pw = win - ph * S2;
      cnn_put_window(Dz + co * LDA, O2, ph, pw, am[e], dp2[e]);
    }
    __syncthreads();
    const float* ap = Dz + (16 * w + lr) * LDA;
    for (int k = lk; k < npx; k += 4) {
      const float av = ap[k];
      const float* bp = Ps + ptab[k];
#pragma unroll
      for (int j = 0; j < CNN_WRW_NT; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bp[cf[j]], acc[j],
                                                      0, 0, 0);
    }
  }
#pragma unroll
  for (int j = 0; j < CNN_WRW_NT; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = 16 * w + 4 * lk + i, n = n0 + 16 * j + lr;
      if (co < C2 && n < K2) {
        const int e = L.w2 + co * K2 + n;
        mlp_update<false>(u, e, u.p[e], acc[j][i], k0);
      }
    }
  if (blockIdx.y != 0) return;
  // db2[co]: wave q sums the samples q, q + 4, ..., the four parts in order
  {
    const int co = tid & 63, q = tid >> 6;
    float sb = 0.f;
    if (co < C2)
      for (int b = q; b < a.m.B; b += 4) {
        if (rid[b] < 0) continue;
        const float* dp2 = ws + L.dp2 + (long)b * L.F2 + co * nwin;
        const unsigned char* am = wsb + L.am2 + (long)b * L.F2 + co * nwin;
        for (int i = 0; i < nwin; ++i)
          if (am[i] < 4) sb += dp2[i];
      }
    red[tid] = sb;
  }
  __syncthreads();
  if (tid < C2) {
    const float sb = ((red[tid] + red[64 + tid]) + red[128 + tid]) +
                     red[192 + tid];
    mlp_update<false>(u, L.b2 + tid, u.p[L.b2 + tid], sb, k0);
  }
}

// conv1 weight and bias gradient of output channel blockIdx.y and their
// update.  dz1c has one non-zero per pool window, so the sum runs over the
// windows: thread (t, sl) sums filter element t (t = 25 Cin: the bias) over
// the windows sl, sl + SL, ... of every sample, the SL parts in order.
// grid = (C, C1).
__global__ void __launch_bounds__(CNNROUND_THREADS)
cnn_conv1_wrw_k(const CnnRoundArgs a, int s) {
  __shared__ float img[CNNROUND_MAXCIN * CNNROUND_MAXS * CNNROUND_MAXS];
  __shared__ float gs[(CNNROUND_MAXS / 2) * (CNNROUND_MAXS / 2)];
  __shared__ int off[(CNNROUND_MAXS / 2) * (CNNROUND_MAXS / 2)];
  __shared__ float part[CNNROUND_THREADS];
  __shared__ int rid[MLPROUND_MAXB];
  const int c = blockIdx.x, co = blockIdx.y;
  if (s >= mlp_nsteps(a.m, c)) return;
  const CnnLayout& L = a.lay;
  const int tid = threadIdx.x;
  const int Cin = L.Cin, S = L.S, C1 = L.C1, S1 = L.S1, nt = 25 * Cin;
  const int ntp = nt + 1 <= 32 ? 32 : 128, SL = CNNROUND_THREADS / ntp;
  const int t = tid % ntp, sl = tid / ntp;
  mlp_rows(a.m, c, s, rid);
  const MlpSgd u = mlp_sgd<false>(a.m, c, s);
  const MlpCorr k0 = {0.f, 0.f};
  int xo = 0;
  if (t < nt) {
    int ci, tt;
    cnn_tap(L.nhwc1, t, Cin, ci, tt);
    xo = ci * S * S + (tt / 5) * S + tt % 5;
  }
  const int nw = S1 * S1, nimg = Cin * S * S;
  const float* ws = a.m.ws + (long)c * a.m.lay.ws_stride;
  const unsigned char* wsb = a.wsb + (long)c * L.wsb_stride;
  float acc = 0.f;
  for (int b = 0; b < a.m.B; ++b) {
    const int r = rid[b];
    if (r < 0) continue;
    __syncthreads();            // the last sample's reads
    const float* x = a.m.X + (long)r * nimg;
    for (int e = tid; e < nimg; e += CNNROUND_THREADS) img[e] = x[e];
    const long o = ((long)b * C1 + co) * nw;
    for (int win = tid; win < nw; win += CNNROUND_THREADS) {
      const int code = wsb[L.am1 + o + win];
      const int ph = win / S1, pw = win - ph * S1;
      gs[win] = code < 4 ? ws[L.dp1 + o + win] : 0.f;
      off[win] = (2 * ph + ((code >> 1) & 1)) * S + 2 * pw + (code & 1);
    }
    __syncthreads();
    if (t < nt) {
      for (int win = sl; win < nw; win += SL)
        acc = fmaf(gs[win], img[xo + off[win]], acc);
    } else if (t == nt) {
      for (int win = sl; win < nw; win += SL) acc += gs[win];
    }
  }
  __syncthreads();
  part[tid] = acc;
  __syncthreads();
  if (tid <= nt) {
    float g = 0.f;
    for (int q = 0; q < SL; ++q) g += part[q * ntp + tid];
    const int e = tid < nt ? L.w1 + co * nt + tid : L.b1 + co;
    mlp_update<false>(u, e, u.p[e], g, k0);
  }
}
