// Local SGD steps of packed MLP clients, batched per layer: every kernel's
// grid has a client dimension, the weights are read from (and updated in)
// the [C, N] replica arena, BatchNorm statistics are per client.
//
// The model: L blocks of Linear(in, H) + bias, BatchNorm1d over the batch
// (biased variance, affine, never running statistics), ReLU; then the head
// fc = Linear(H, K, bias=False) and mean softmax cross-entropy.
//
//   for each client c with steps[c] > 0 (others: nothing read or written):
//     replicas[c] <- server                                  mlp_rows_k(0)
//     for s in 0 .. steps[c]-1, rows r = idx[c, s, :] >= 0, n = #rows:
//       [snap[c] <- replicas[c]  if s + 1 == k_cut]          mlp_rows_k(1)
//       a_0 = X[r]
//       z_i = a_i W_i^T + b_i ; mu, var over the n rows      mlp_fwd_layer_k
//       xh = (z - mu) / sqrt(var + eps) ; a_{i+1} = max(g xh + beta, 0)
//       logits = a_L Wfc^T ; loss[c, s] ; dlogits / n        mlp_head_k
//       for i = L-1 .. 0, M = the matrix above layer i:      mlp_bwd_k<false>
//         da = dz_M M ; dM = dz_M^T a ; SGD on M ; BN backward -> dz_i ;
//         SGD on g_i, beta_i, b_i
//       dW_0 = dz_0^T x ; SGD on W_0                         mlp_bwd_k<true>
//       every SGD update with fused_sgd_step's gradient corrections:
//         d = g ; [delta] d -= delta[c] ; [control pair] d += c - c_c[c] ;
//         [prox_mu] d += mu (p - server) ; then wd, momentum, p -= lr d
//     mom_init[c] <- 1 (with momentum)                       mlp_rows_k(2)
//
// 2L + 2 launches per step, grid = (C, column tiles), 256 threads.  Every
// kernel takes the step s and returns at once, uniformly, for a client with
// s >= steps[c].
//
// Tiles: a block owns MLP_TN = 32 columns and all (<= 64) rows of them, so
// the BatchNorm sums (forward statistics, backward sums) are block-local.
// Thread (tx = tid % 32, ty = tid / 32) holds column tx of rows ty + 8 m,
// m < 8.  Products run over 32-deep chunks staged in LDS with row stride 33
// (odd: the column-indexed reads are conflict-free, the row-indexed ones are
// broadcasts).
//
// mlp_bwd_k owns a column slab M[:, tile] of the matrix above: per 32-row
// chunk of M it stages the chunk (pre-update), adds its share to da, forms
// the chunk's weight gradient from the staged dz_M and a, and updates the
// chunk in place from the staged values.  No other block touches that slab
// in the launch, so dgrad always sees pre-update weights.
//
// No atomics; every summation order is fixed by the shapes, so two runs are
// bit-identical.  No host reads: capture-safe.  Padding samples (idx < 0 or
// >= M) are never dereferenced: their rows are zero in every staged tile,
// in xh, a and dz, and they are excluded from n.  Only parameter elements of
// the rows of online clients are written (replicas: the whole row first).
//
// A gradient correction is constant over the round and is read where it is
// used: lanes run along the contiguous arena index at every update site, so
// its loads coalesce like the momentum's, and they are issued ahead of the
// sums that precede the update.  The backward kernels exist twice
// (template <bool CORR>): without a correction the launcher runs code that
// knows none.  Only parameter elements of the correction rows of clients
// with steps > 0 are read, and none past the client's last step.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"

#define MLPROUND_THREADS 256
#define MLPROUND_MAXB 64
#define MLPROUND_MAXK 128
#define MLPROUND_MAXL 8
#define MLP_TN 32               // columns of a tile, and depth of a chunk
#define MLP_LD 33               // LDS row stride of a tile
// gradient corrections of a round (MlpRoundArgs.corr, the same in all blocks)
#define MLPROUND_DELTA 1
#define MLPROUND_CTRL 2
#define MLPROUND_PROX 4

struct MlpLayout {
  int L;
  int w[MLPROUND_MAXL], b[MLPROUND_MAXL], g[MLPROUND_MAXL],
      be[MLPROUND_MAXL];                       // arena offsets per block
  int in[MLPROUND_MAXL], out[MLPROUND_MAXL];
  int fc, H, K;                                // the head: offset, [K, H]
  // workspace offsets (floats, per client)
  int xh[MLPROUND_MAXL], act[MLPROUND_MAXL], rstd[MLPROUND_MAXL];
  int dz[MLPROUND_MAXL + 1];                   // dz[L]: dlogits / n
  long ws_stride;
};

struct MlpRoundArgs {
  const float* X;        // [M, F]
  const int* Y;          // [M]
  const int* idx;        // [C, T, B]
  const int* steps;      // [C]
  const float* lr;       // [C, T]
  const float* server;   // [N]
  float* replicas;       // [C, N]
  float* in_mom;         // [C, N] or null
  int* mom_init;         // [C]
  float* snap;           // [C, N] or null
  float* loss;           // [C, T]
  float* ws;             // [C, ws_stride]
  const float* corr_rows;  // [C, N] or null: delta (d -= delta[c]) or, with
  const float* ctrl_s;     // ctrl_s [N], the client controls (d += c - c_c[c])
  int M, B, T, N;
  int k_cut, use_mom, nesterov, wd_numel;
  float wd, mom, omd, eps;
  float prox_mu;         // != 0: d += prox_mu (p - server)
  int corr;              // MLPROUND_DELTA | _CTRL | _PROX, 0: no correction
  MlpLayout lay;
};

// the SGD state of a (client, step): lr and the first-use momentum rule
struct MlpSgd {
  float lr, mom, omd, wd, mom_n;
  int use_mom, nesterov, wd_numel;
  float* p;              // the client's replica row
  float* m;              // its momentum row
  // the correction (set and used by the CORR kernels only)
  const float* cr;       // the client's correction row
  const float* cs;       // the server control
  const float* srv;      // the server
  float prox_mu;
  int corr;
};

template <bool CORR>
__device__ __forceinline__ MlpSgd mlp_sgd(const MlpRoundArgs& a, int c,
                                          int s) {
  MlpSgd u;
  const bool first = a.use_mom && s == 0 && a.mom_init[c] == 0;
  u.lr = a.lr[(long)c * a.T + s];
  u.mom = first ? 0.f : a.mom;        // first use: buf = 0 * buf + 1 * d
  u.omd = first ? 1.f : a.omd;
  u.mom_n = a.mom;
  u.wd = a.wd;
  u.use_mom = a.use_mom;
  u.nesterov = a.nesterov;
  u.wd_numel = a.wd_numel;
  u.p = a.replicas + (long)c * a.N;
  u.m = a.use_mom ? a.in_mom + (long)c * a.N : nullptr;
  if (CORR) {
    u.cr = a.corr_rows ? a.corr_rows + (long)c * a.N : nullptr;
    u.cs = a.ctrl_s;
    u.srv = a.server;
    u.prox_mu = a.prox_mu;
    u.corr = a.corr;
  }
  return u;
}

// the correction of arena element e: cv = delta or c - c_c (the difference
// first, as fused_sgd_step forms it), sv = the server's value for the
// proximal term.  Loaded ahead of the update that uses it.
struct MlpCorr {
  float cv, sv;
};

template <bool CORR>
__device__ __forceinline__ MlpCorr mlp_corr_load(const MlpSgd& u, int e) {
  MlpCorr k = {0.f, 0.f};
  if (CORR) {
    if (u.corr & MLPROUND_DELTA) k.cv = u.cr[e];
    else if (u.corr & MLPROUND_CTRL) k.cv = u.cs[e] - u.cr[e];
    if (u.corr & MLPROUND_PROX) k.sv = u.srv[e];
  }
  return k;
}

// the local branch of fused_sgd_step on arena element e, p its value
template <bool CORR>
__device__ __forceinline__ void mlp_update(const MlpSgd& u, int e, float p,
                                           float g, const MlpCorr& k) {
  if (CORR) {
    if (u.corr & MLPROUND_DELTA) g -= k.cv;
    else if (u.corr & MLPROUND_CTRL) g += k.cv;
    if (u.corr & MLPROUND_PROX) g = fmaf(u.prox_mu, p - k.sv, g);
  }
  float d = e < u.wd_numel ? fmaf(u.wd, p, g) : g;
  if (u.use_mom) {
    const float bu = fmaf(u.mom, u.m[e], u.omd * d);
    u.m[e] = bu;
    d = u.nesterov ? fmaf(u.mom_n, bu, d) : bu;
  }
  u.p[e] = fmaf(-u.lr, d, p);
}

// rows of the step into LDS (-1: padding, also for b >= B); returns n
__device__ __forceinline__ int mlp_rows(const MlpRoundArgs& a, int c, int s,
                                        int* rid) {
  const int tid = threadIdx.x;
  if (tid < MLPROUND_MAXB) {
    int r = -1;
    if (tid < a.B) {
      r = a.idx[((long)c * a.T + s) * a.B + tid];
      if (r >= a.M) r = -1;
    }
    rid[tid] = r;
  }
  __syncthreads();
  int n = 0;
  for (int b = 0; b < a.B; ++b) n += rid[b] >= 0;
  return n;
}

// As[b][kk] = A[row(b)][k0 + kk], zero for padding rows and past nK.
// GATHER: row(b) = rid[b] (the data matrix), else b (a workspace matrix).
template <bool GATHER>
__device__ __forceinline__ void mlp_load_a(float* As, const float* A, int lda,
                                           int k0, int nK, const int* rid) {
  const int kk = threadIdx.x & 31, b0 = threadIdx.x >> 5;
  const bool kin = k0 + kk < nK;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int b = b0 + 8 * m;
    const int r = rid[b];
    float v = 0.f;
    if (r >= 0 && kin) v = A[(long)(GATHER ? r : b) * lda + k0 + kk];
    As[b * MLP_LD + kk] = v;
  }
}

// Ws[col][kk] = W[j0 + col][k0 + kk] of a row-major [ncols, nK] matrix
// (TRANS: of a row-major [nK, ncols] one), zero outside.  Lanes run along the
// contiguous dimension of W either way.
template <bool TRANS>
__device__ __forceinline__ void mlp_load_w(float* Ws, const float* W, int j0,
                                           int ncols, int k0, int nK) {
  const int lo = threadIdx.x & 31, hi0 = threadIdx.x >> 5;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int hi = hi0 + 8 * m;
    const int col = TRANS ? lo : hi, kk = TRANS ? hi : lo;
    float v = 0.f;
    if (j0 + col < ncols && k0 + kk < nK)
      v = TRANS ? W[(long)(k0 + kk) * ncols + j0 + col]
                : W[(long)(j0 + col) * nK + k0 + kk];
    Ws[col * MLP_LD + kk] = v;
  }
}

// acc[m] += sum_kk As[ty + 8 m][kk] Ws[tx][kk], kk ascending
__device__ __forceinline__ void mlp_fma_tile(float (&acc)[8], const float* As,
                                             const float* Ws) {
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll 8
  for (int kk = 0; kk < MLP_TN; ++kk) {
    const float w = Ws[tx * MLP_LD + kk];
#pragma unroll
    for (int m = 0; m < 8; ++m)
      acc[m] = fmaf(As[(ty + 8 * m) * MLP_LD + kk], w, acc[m]);
  }
}

__device__ __forceinline__ int mlp_nsteps(const MlpRoundArgs& a, int c) {
  return min(a.steps[c], a.T);
}

// mode 0: replicas[c] <- server ; 1: snap[c] <- replicas[c] for clients that
// reach step k_cut ; 2: mom_init[c] <- 1.  grid = (C, row blocks).
__global__ void __launch_bounds__(MLPROUND_THREADS)
mlp_rows_k(const MlpRoundArgs a, int mode) {
  const int c = blockIdx.x;
  const int ns = mlp_nsteps(a, c);
  if (ns <= 0) return;
  if (mode == 2) {
    if (blockIdx.y == 0 && threadIdx.x == 0) a.mom_init[c] = 1;
    return;
  }
  if (mode == 1 && a.k_cut > ns) return;
  const float* src = mode == 0 ? a.server : a.replicas + (long)c * a.N;
  float* dst = (mode == 0 ? a.replicas : a.snap) + (long)c * a.N;
  for (int i = blockIdx.y * MLPROUND_THREADS + threadIdx.x; i < a.N;
       i += gridDim.y * MLPROUND_THREADS)
    dst[i] = src[i];
}

// forward of block li for the tile blockIdx.y of its output columns
template <bool GATHER>
__global__ void __launch_bounds__(MLPROUND_THREADS)
mlp_fwd_layer_k(const MlpRoundArgs a, int s, int li) {
  __shared__ float As[MLPROUND_MAXB * MLP_LD];
  __shared__ float Ws[MLP_TN * MLP_LD];
  __shared__ float st[2 * MLP_TN];
  __shared__ int rid[MLPROUND_MAXB];
  const int c = blockIdx.x;
  if (s >= mlp_nsteps(a, c)) return;
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int j0 = blockIdx.y * MLP_TN;
  const int n = mlp_rows(a, c, s, rid);
  const int in = a.lay.in[li], out = a.lay.out[li];
  const float* P = a.replicas + (long)c * a.N;
  float* ws = a.ws + (long)c * a.lay.ws_stride;
  const float* A = GATHER ? a.X : ws + a.lay.act[li - 1];
  const float* W = P + a.lay.w[li];

  float acc[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) acc[m] = 0.f;
  for (int k0 = 0; k0 < in; k0 += MLP_TN) {
    mlp_load_a<GATHER>(As, A, in, k0, in, rid);
    mlp_load_w<false>(Ws, W, j0, out, k0, in);
    __syncthreads();
    mlp_fma_tile(acc, As, Ws);
    __syncthreads();
  }
  const int col = j0 + tx;
  const bool cin = col < out;
  const float bias = cin ? P[a.lay.b[li] + col] : 0.f;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    acc[m] += bias;
    As[(ty + 8 * m) * MLP_LD + tx] = acc[m];      // z of the tile
  }
  __syncthreads();
  if (tid < MLP_TN) {           // statistics of column tid, rows in order
    const float inv = n > 0 ? 1.f / (float)n : 0.f;
    float sum = 0.f;
    for (int b = 0; b < a.B; ++b)
      if (rid[b] >= 0) sum += As[b * MLP_LD + tid];
    const float mu = sum * inv;
    float sq = 0.f;
    for (int b = 0; b < a.B; ++b)
      if (rid[b] >= 0) {
        const float d = As[b * MLP_LD + tid] - mu;
        sq = fmaf(d, d, sq);
      }
    const float rs = 1.f / sqrtf(sq * inv + a.eps);
    st[tid] = mu;
    st[MLP_TN + tid] = rs;
    if (j0 + tid < out) ws[a.lay.rstd[li] + j0 + tid] = rs;
  }
  __syncthreads();
  if (!cin) return;
  const float mu = st[tx], rs = st[MLP_TN + tx];
  const float g = P[a.lay.g[li] + col], be = P[a.lay.be[li] + col];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int b = ty + 8 * m;
    if (b >= a.B) break;
    const bool ok = rid[b] >= 0;
    const float xh = ok ? (acc[m] - mu) * rs : 0.f;
    const float y = fmaf(g, xh, be);
    ws[a.lay.xh[li] + (long)b * out + col] = xh;
    ws[a.lay.act[li] + (long)b * out + col] = ok ? fmaxf(y, 0.f) : 0.f;
  }
}

// head: logits, softmax cross-entropy, loss[c, s], dlogits / n.  One block
// per client; the logits [B, K] are staged in LDS with row stride K | 1.
// BIAS: the head has a bias at arena offset b_off (the CNN of cnnround.h).
template <bool BIAS>
__global__ void __launch_bounds__(MLPROUND_THREADS)
mlp_head_k(const MlpRoundArgs a, int s, int b_off) {
  __shared__ float As[MLPROUND_MAXB * MLP_LD];
  __shared__ float Ws[MLP_TN * MLP_LD];
  __shared__ float Ls[MLPROUND_MAXB * (MLPROUND_MAXK + 1)];
  __shared__ float lrow[MLPROUND_MAXB];
  __shared__ int rid[MLPROUND_MAXB];
  const int c = blockIdx.x;
  if (s >= mlp_nsteps(a, c)) return;
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int n = mlp_rows(a, c, s, rid);
  const int H = a.lay.H, K = a.lay.K, KS = K | 1, L = a.lay.L;
  float* ws = a.ws + (long)c * a.lay.ws_stride;
  const float* A = ws + a.lay.act[L - 1];
  const float* W = a.replicas + (long)c * a.N + a.lay.fc;

  for (int j0 = 0; j0 < K; j0 += MLP_TN) {
    float acc[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) acc[m] = 0.f;
    for (int k0 = 0; k0 < H; k0 += MLP_TN) {
      mlp_load_a<false>(As, A, H, k0, H, rid);
      mlp_load_w<false>(Ws, W, j0, K, k0, H);
      __syncthreads();
      mlp_fma_tile(acc, As, Ws);
      __syncthreads();
    }
    if (j0 + tx < K) {
      const float bias = BIAS ? W[b_off - a.lay.fc + j0 + tx] : 0.f;
#pragma unroll
      for (int m = 0; m < 8; ++m)
        Ls[(ty + 8 * m) * KS + j0 + tx] = BIAS ? acc[m] + bias : acc[m];
    }
  }
  __syncthreads();
  const float inv = n > 0 ? 1.f / (float)n : 0.f;
  if (tid < a.B) {
    float* z = Ls + tid * KS;
    const int r = rid[tid];
    float l = 0.f;
    if (r < 0) {
      for (int k = 0; k < K; ++k) z[k] = 0.f;
    } else {
      const int y = a.Y[r];
      const bool yok = y >= 0 && y < K;
      float mx = z[0];
      for (int k = 1; k < K; ++k) mx = fmaxf(mx, z[k]);
      const float zy = yok ? z[y] : 0.f;
      float sum = 0.f;
      for (int k = 0; k < K; ++k) {
        const float e = expf(z[k] - mx);
        z[k] = e;
        sum += e;
      }
      l = (logf(sum) + mx) - zy;
      const float rs = 1.f / sum;
      for (int k = 0; k < K; ++k) z[k] *= rs;
      if (yok) z[y] -= 1.f;
      for (int k = 0; k < K; ++k) z[k] *= inv;
    }
    lrow[tid] = l;
  }
  __syncthreads();
  if (tid == 0) {                              // fixed-order mean of the rows
    float t = 0.f;
    for (int b = 0; b < a.B; ++b) t += lrow[b];
    a.loss[(long)c * a.T + s] = t * inv;
  }
  float* dl = ws + a.lay.dz[L];
  for (int e = tid; e < a.B * K; e += MLPROUND_THREADS) {
    const int b = e / K;
    dl[e] = Ls[b * KS + (e - b * K)];
  }
}

// backward through the boundary above block li (FIRST: below block 0).
//   !FIRST  tile of block li's output columns; M = W_{li+1} or the head
//           [nO, ncol]; a = a_{li+1} (block li's activation); da, SGD on
//           M[:, tile], BN backward, SGD on g, beta, b, dz_li[:, tile].
//   FIRST   tile of the input features; M = W_0 [nO, ncol = F]; a = x
//           re-gathered; SGD on W_0[:, tile] only.
// CORR: the SGD updates take the round's gradient correction.
template <bool FIRST, bool CORR>
__global__ void __launch_bounds__(MLPROUND_THREADS)
mlp_bwd_k(const MlpRoundArgs a, int s, int li) {
  __shared__ float As[MLPROUND_MAXB * MLP_LD];   // dz_M chunk, later dy
  __shared__ float Ws[MLP_TN * MLP_LD];          // M chunk (pre-update)
  __shared__ float At[MLPROUND_MAXB * MLP_LD];   // a tile
  __shared__ float Xs[MLPROUND_MAXB * MLP_LD];   // xh tile
  __shared__ float st[3 * MLP_TN];
  __shared__ int rid[MLPROUND_MAXB];
  const int c = blockIdx.x;
  if (s >= mlp_nsteps(a, c)) return;
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int j0 = blockIdx.y * MLP_TN;
  const int n = mlp_rows(a, c, s, rid);
  const int L = a.lay.L;
  const MlpSgd u = mlp_sgd<CORR>(a, c, s);
  float* ws = a.ws + (long)c * a.lay.ws_stride;
  const int ncol = FIRST ? a.lay.in[0] : a.lay.out[li];
  const bool head = !FIRST && li == L - 1;
  const int nO = FIRST ? a.lay.out[0] : (head ? a.lay.K : a.lay.out[li + 1]);
  const int m_off = FIRST ? a.lay.w[0] : (head ? a.lay.fc : a.lay.w[li + 1]);
  const float* dzM = ws + a.lay.dz[FIRST ? 0 : li + 1];
  const int col = j0 + tx;
  const bool cin = col < ncol;

  // the a tile: At[b][jc] (k0 = j0 as the "chunk")
  if (FIRST) mlp_load_a<true>(At, a.X, ncol, j0, ncol, rid);
  else mlp_load_a<false>(At, ws + a.lay.act[li], ncol, j0, ncol, rid);

  float acc[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) acc[m] = 0.f;
  for (int o0 = 0; o0 < nO; o0 += MLP_TN) {
    mlp_load_a<false>(As, dzM, nO, o0, nO, rid);
    mlp_load_w<true>(Ws, u.p + m_off, j0, ncol, o0, nO);
    // the correction of the chunk's elements: issued here, used after the
    // rows
    MlpCorr kc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int oo = ty + 8 * q;
      kc[q] = MlpCorr{0.f, 0.f};
      if (cin && o0 + oo < nO)
        kc[q] = mlp_corr_load<CORR>(u, m_off + (o0 + oo) * ncol + col);
    }
    __syncthreads();
    if (!FIRST) mlp_fma_tile(acc, As, Ws);
    // weight gradient of M[o0 + oo][col], oo = ty + 8 q, rows in order
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < a.B; ++b) {
      const float av = At[b * MLP_LD + tx];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        g[q] = fmaf(As[b * MLP_LD + ty + 8 * q], av, g[q]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int oo = ty + 8 * q;
      if (cin && o0 + oo < nO)
        mlp_update<CORR>(u, m_off + (o0 + oo) * ncol + col,
                         Ws[tx * MLP_LD + oo], g[q], kc[q]);
    }
    __syncthreads();
  }
  if (FIRST) return;

  // ReLU mask and BatchNorm backward of the tile's columns
  const int out = ncol;
  mlp_load_a<false>(Xs, ws + a.lay.xh[li], out, j0, out, rid);
  float dy[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int b = ty + 8 * m;
    dy[m] = At[b * MLP_LD + tx] > 0.f ? acc[m] : 0.f;
    As[b * MLP_LD + tx] = dy[m];
  }
  __syncthreads();
  const float nf = (float)n;
  if (tid < MLP_TN) {
    // the corrections of gamma and beta: issued ahead of the sums
    MlpCorr kg = {0.f, 0.f}, kb = {0.f, 0.f};
    if (j0 + tid < out) {
      kg = mlp_corr_load<CORR>(u, a.lay.g[li] + j0 + tid);
      kb = mlp_corr_load<CORR>(u, a.lay.be[li] + j0 + tid);
    }
    float s1 = 0.f, s2 = 0.f;
    for (int b = 0; b < a.B; ++b) {
      const float d = As[b * MLP_LD + tid];
      s1 += d;
      s2 = fmaf(d, Xs[b * MLP_LD + tid], s2);
    }
    st[tid] = s1;
    st[MLP_TN + tid] = s2;
    float coef = 0.f;
    const int cj = j0 + tid;
    if (cj < out) {
      const float gam = u.p[a.lay.g[li] + cj];
      coef = gam * ws[a.lay.rstd[li] + cj] * (n > 0 ? 1.f / nf : 0.f);
      mlp_update<CORR>(u, a.lay.g[li] + cj, gam, s2, kg);
      mlp_update<CORR>(u, a.lay.be[li] + cj, u.p[a.lay.be[li] + cj], s1, kb);
    }
    st[2 * MLP_TN + tid] = coef;
  }
  __syncthreads();
  {
    const float s1 = st[tx], s2 = st[MLP_TN + tx], coef = st[2 * MLP_TN + tx];
    float* dz = ws + a.lay.dz[li];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int b = ty + 8 * m;
      const float xh = Xs[b * MLP_LD + tx];
      const float v = rid[b] >= 0
          ? coef * (fmaf(nf, dy[m], -s1) - xh * s2) : 0.f;
      if (b < a.B && cin) dz[(long)b * out + col] = v;
      dy[m] = v;
    }
  }
  __syncthreads();                       // the sums have read dy from As
#pragma unroll
  for (int m = 0; m < 8; ++m) As[(ty + 8 * m) * MLP_LD + tx] = dy[m];
  __syncthreads();
  if (tid < MLP_TN && j0 + tid < out) {  // db = sum of dz over the rows
    const int e = a.lay.b[li] + j0 + tid;
    const MlpCorr kc = mlp_corr_load<CORR>(u, e);
    float sb = 0.f;
    for (int b = 0; b < a.B; ++b) sb += As[b * MLP_LD + tid];
    mlp_update<CORR>(u, e, u.p[e], sb, kc);
  }
}
