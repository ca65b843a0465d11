// Local SGD steps of packed char-GRU clients, batched per layer: every grid
// has a client dimension, the weights are read from (and updated in) the
// [C, N] replica arena, activations live in a per-client workspace.
//
// The model (components/models/rnn.py, one layer, gate order r, z, n):
// encoder E [V, H], GRU W_ih / W_hh [3H, H], b_ih / b_hh [3H], decoder
// W_d [K, H], b_d [K]; a data row is one window of T tokens and T targets.
//
//   for each client c with steps[c] > 0 (others: nothing read or written):
//     replicas[c] <- server                                  mlp_rows_k(0)
//     for s in 0 .. steps[c]-1, rows idx[c, s, :n] (the valid prefix):
//       [snap[c] <- replicas[c]  if s + 1 == k_cut]          mlp_rows_k(1)
//       P = E W_ih^T + b_ih                        [V, 3H]   rnn_table_k
//       h0 = hidden[c, :n] if hid_rows[c] == n else 0
//       gx[b, t] = P[tok[b, t]] (0 outside [0, V)) ; the GRU over T steps ;
//       hidden[c, :n] <- h_T                                 rnn_gru_fwd_k
//       logits = out W_d^T + b_d ; CE per row ; dlogits / (n T)
//                                                            rnn_dec_k
//       dW_d = dlogits^T out, db_d | dout = dlogits W_d      rnn_dec_bwd_k
//       the sequence backward: dgx, dgh                      rnn_gru_bwd_k
//       dP (one-hot A operand), dW_hh, db_hh                 rnn_grads_k
//       dE = dP W_ih, dW_ih = dP^T E, db_ih = colsum dP      rnn_table_bwd_k
//       SGD on the seven tensors ; hid_rows[c] <- n ;
//       loss[c, s] = sum of the tile partials / (n T)        rnn_update_k
//     mom_init[c] <- 1 (with momentum)                       mlp_rows_k(2)
//
// Eight launches per step.  Every kernel takes the step s and returns at
// once, uniformly, for a client with s >= steps[c].  The update is a launch
// of its own, so every gradient kernel reads pre-update weights; hid_rows[c]
// is read by all batch tiles of the forward launch and written by the last.
//
// All products are v_mfma_f32_16x16x4_f32 (lane l holds A[row l&15][k l>>4],
// B[k l>>4][col l&15] and C[row 4*(l>>4)+i][col l&15]): a k-ordered fp32 fmaf
// chain.  The sequence kernels are those of gru.h with the client axis: W_hh
// in LDS, h / dgh double-buffered as the A operand, one barrier per step,
// tokens prefetched two steps ahead.  The reduce kernels are those of
// gru_tok.h: a workgroup owns its output tile for all of K = n T, its waves
// take the 4-row k-steps round robin and are merged in wave order.
//
// No atomics; every summation order is fixed by the shapes and n, so two runs
// are bit-identical.  No host reads: capture-safe.  n is the length of the
// valid prefix of idx[c, s, :] (0 <= row < M); nothing past it is addressed.
// Rows >= n T and columns >= H / 3H / V / K are never loaded (their operand is
// 0) and never stored.  A target outside [0, K) selects no logit.
// Scalar fp32 code only (GRU_SCALAR_F32).
//
// Limits (checked by the launcher): 1 <= H <= 64, 1 <= V, K <= 128,
// 1 <= B <= 64, T >= 1, the per-client workspace below 2^30 floats.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "gru.h"
#include "mlpround.h"

#define RNNROUND_MAXH 64
#define RNNROUND_MAXV 128      // vocabulary V and classes K
#define RNNROUND_MAXB 64
#define RNNROUND_THREADS 256   // one-tile-per-wave kernels and the update
#define RNN_NW 8               // waves of a reduce workgroup
#define RNN_U 4                // k-steps in flight per wave
#define RNN_LG (RNNROUND_MAXV + 1)   // LDS row stride of the logits tile
#define RNN_NTENS 7

struct RnnLayout {
  int V, H, K;
  // arena offsets, in the order of `off`: encoder, w_ih, w_hh, b_ih, b_hh,
  // decoder weight, decoder bias; start[q] = elements before tensor q
  int off[RNN_NTENS];
  int start[RNN_NTENS + 1];
  // workspace offsets (floats, per client)
  int P, h0, out, gates, dl, dout, dgx, dgh, dP, lossp, grad;
  long ws_stride;
};
enum { RNN_ENC, RNN_WIH, RNN_WHH, RNN_BIH, RNN_BHH, RNN_DW, RNN_DB };

struct RnnRoundArgs {
  MlpRoundArgs m;        // X, Y unused; T = steps, lay unused
  const int* tok;        // [M, Tq]
  const int* tgt;        // [M, Tq]
  float* hidden;         // [C, B, H]
  int* hid_rows;         // [C]
  int* tokw;             // [C, B * Tq]: the step's tokens, -1 outside [0, V)
  int Tq;                // window length
  RnnLayout lay;
};

// n of step s: the length of the valid prefix of idx[c, s, :].  Every lane
// of a (converged) wave gets it.
__device__ __forceinline__ int rnn_nrows(const RnnRoundArgs& a, int c,
                                         int s) {
  const int lane = threadIdx.x & (WAVE - 1);
  int r = -1;
  if (lane < a.m.B) {
    r = a.m.idx[((long)c * a.m.T + s) * a.m.B + lane];
    if (r >= a.m.M) r = -1;
  }
  const unsigned long long ok = __ballot(r >= 0);
  return ok == ~0ull ? WAVE : __ffsll((long long)~ok) - 1;
}

// token i of `tok` if it is loaded and inside [0, V), else -1; `st`: keep it
__device__ __forceinline__ int rnn_tok(const int* __restrict__ tok, long i,
                                       bool ld, int V, int* __restrict__ keep,
                                       long ki, bool st) {
  if (!ld) return -1;
  int v = tok[i];
  if (v < 0 || v >= V) v = -1;
  if (st) keep[ki] = v;
  return v;
}

// --------------------------------------------------------------------------
// 1. the input-gate table P[c] = E W_ih^T + b_ih
// --------------------------------------------------------------------------
// grid (ceil(tiles / 4), C), one 16x16 tile of [V, 3H] per wave, K = H.
__global__ void __launch_bounds__(RNNROUND_THREADS) GRU_SCALAR_F32
rnn_table_k(const RnnRoundArgs a, int s) {
  const int c = blockIdx.y;
  if (s >= mlp_nsteps(a.m, c)) return;
  const RnnLayout& L = a.lay;
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  const int lr = lane & 15, lk = lane >> 4;
  const int H = L.H, H3 = 3 * H, NT3 = (H3 + 15) / 16;
  const int tile = blockIdx.x * (RNNROUND_THREADS / WAVE) + wid;
  if (tile >= ((L.V + 15) / 16) * NT3) return;
  const int v0 = (tile / NT3) * 16, j0 = (tile % NT3) * 16;
  const float* Pm = a.m.replicas + (long)c * a.m.N;
  const float* E = Pm + L.off[RNN_ENC];
  const float* W = Pm + L.off[RNN_WIH];
  const int v = v0 + lr, j = j0 + lr;
  const bool vok = v < L.V, jok = j < H3;
  const float bj = jok ? Pm[L.off[RNN_BIH] + j] : 0.f;
  gru_f4 acc = {bj, bj, bj, bj};
  for (int k0 = 0; k0 < H; k0 += 4) {
    const int k = k0 + lk;
    const float av = (vok && k < H) ? E[v * H + k] : 0.f;
    const float bv = (jok && k < H) ? W[j * H + k] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
  }
  float* P = a.m.ws + (long)c * L.ws_stride + L.P;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int vv = v0 + 4 * lk + i;
    if (vv < L.V && jok) P[vv * H3 + j] = acc[i];
  }
}

// --------------------------------------------------------------------------
// 2. the sequence forward (gru_tok_fwd_k of gru.h with the client axis)
// --------------------------------------------------------------------------
// grid (ceil(B/16), C), block 64*NT, NT = ceil(H/16).  Writes out [n, T, H],
// gates [n, T, 4, H] = (r, z, n, q), h0 [n, H] (the state the step started
// from), tokw and hidden[c] -- rows of its own tile only.
template <int NT>
__global__ void __launch_bounds__(NT * WAVE) GRU_SCALAR_F32
rnn_gru_fwd_k(const RnnRoundArgs a, int s) {
  constexpr int HP = NT * 16;
  constexpr int S = HP + 2;             // S mod 32 in {2, 18}
  constexpr int NTHR = NT * WAVE;
  __shared__ float Ws[3 * HP * S];      // [gate][n][k]
  __shared__ float hs[2][GRU_ROWS * S];  // [buffer][row][k]
  const int c = blockIdx.y;
  if (s >= mlp_nsteps(a.m, c)) return;
  const int n = rnn_nrows(a, c, s);
  const int b0 = blockIdx.x * GRU_ROWS;
  if (b0 >= n) return;
  const RnnLayout& L = a.lay;
  const int H = L.H, H3 = 3 * H, T = a.Tq, V = L.V;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wid = tid / WAVE;
  const int lr = lane & 15, lk = lane >> 4;
  const float* Pm = a.m.replicas + (long)c * a.m.N;
  const float* w = Pm + L.off[RNN_WHH];
  const float* bias = Pm + L.off[RNN_BHH];
  float* ws = a.m.ws + (long)c * L.ws_stride;
  const float* P = ws + L.P;
  float* out = ws + L.out;
  float* gates = ws + L.gates;
  float* hid = a.hidden + (long)c * a.m.B * H;
  int* tokw = a.tokw + (long)c * a.m.B * T;
  const bool keep = a.hid_rows[c] == n;   // else init_hidden: zeros

  for (int i = tid; i < 3 * HP * S; i += NTHR) {
    const int g = i / (HP * S), rem = i - g * (HP * S);
    const int nn = rem / S, k = rem - nn * S;
    Ws[i] = (nn < H && k < H) ? w[(g * H + nn) * H + k] : 0.f;
  }
  for (int i = tid; i < GRU_ROWS * S; i += NTHR) {
    const int m = i / S, k = i - m * S;
    hs[0][i] = (keep && b0 + m < n && k < H) ? hid[(b0 + m) * H + k] : 0.f;
    hs[1][i] = 0.f;
  }

  const int col = wid * 16 + lr;        // hidden column of this lane
  const bool lcol = col < H;
  bool live[4];
  int ob[4];                            // (b*T)*H + col
  long tb[4];                           // the row's first token in a.tok
  float hprev[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int b = b0 + 4 * lk + i;
    live[i] = lcol && b < n;
    ob[i] = b * T * H + col;
    hprev[i] = (live[i] && keep) ? hid[b * H + col] : 0.f;
    if (live[i]) ws[L.h0 + b * H + col] = hprev[i];
    tb[i] = live[i]
        ? (long)a.m.idx[((long)c * a.m.T + s) * a.m.B + b] * T : 0;
  }
  const float br = lcol ? bias[col] : 0.f;
  const float bz = lcol ? bias[H + col] : 0.f;
  const float bn = lcol ? bias[2 * H + col] : 0.f;

  const bool st = col == 0;             // this lane keeps its rows' tokens
  float xr[4], xz[4], xn[4];
  int tk[4];                            // token of step t + 1, or -1
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long kb = (long)(b0 + 4 * lk + i) * T;
    const int v = rnn_tok(a.tok, tb[i], live[i], V, tokw, kb, st);
    tk[i] = rnn_tok(a.tok, tb[i] + 1, live[i] && 1 < T, V, tokw, kb + 1, st);
    const float* p = P + v * H3 + col;
    xr[i] = v >= 0 ? p[0] : 0.f;
    xz[i] = v >= 0 ? p[H] : 0.f;
    xn[i] = v >= 0 ? p[2 * H] : 0.f;
  }
  __syncthreads();

  const float* wr = Ws + (0 * HP + col) * S + lk;
  const float* wz = Ws + (1 * HP + col) * S + lk;
  const float* wn = Ws + (2 * HP + col) * S + lk;
  for (int t = 0; t < T; ++t) {
    const int cur = t & 1;
    // next step's table rows, in flight during the MFMAs
    float yr[4], yz[4], yn[4];
    int tn[4];                          // token of step t + 2, or -1
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float* p = P + tk[i] * H3 + col;
      yr[i] = tk[i] >= 0 ? p[0] : 0.f;
      yz[i] = tk[i] >= 0 ? p[H] : 0.f;
      yn[i] = tk[i] >= 0 ? p[2 * H] : 0.f;
      tn[i] = rnn_tok(a.tok, tb[i] + t + 2, live[i] && t + 2 < T, V, tokw,
                      (long)(b0 + 4 * lk + i) * T + t + 2, st);
    }
    gru_f4 ar = {br, br, br, br}, az = {bz, bz, bz, bz},
           an = {bn, bn, bn, bn};
    const float* ha = hs[cur] + lr * S + lk;
#pragma unroll
    for (int kk = 0; kk < HP / 4; ++kk) {
      const float av = ha[kk * 4];
      ar = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wr[kk * 4], ar, 0, 0, 0);
      az = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wz[kk * 4], az, 0, 0, 0);
      an = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wn[kk * 4], an, 0, 0, 0);
    }
    float* hn = hs[cur ^ 1] + (4 * lk) * S + col;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float r = gru_sigmoid(xr[i] + ar[i]);
      const float z = gru_sigmoid(xz[i] + az[i]);
      const float q = an[i];
      const float nv = tanhf(xn[i] + r * q);
      float h = (1.f - z) * nv + z * hprev[i];
      if (!live[i]) h = 0.f;
      hn[i * S] = h;
      hprev[i] = h;
      if (live[i]) {
        const int o = ob[i] + t * H;
        out[o] = h;
        float* gp = gates + o * 4 - 3 * col;   // ((b*T + t)*4)*H + col
        gp[0] = r;
        gp[H] = z;
        gp[2 * H] = nv;
        gp[3 * H] = q;
      }
      xr[i] = yr[i]; xz[i] = yz[i]; xn[i] = yn[i];
      tk[i] = tn[i];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (live[i]) hid[(b0 + 4 * lk + i) * H + col] = hprev[i];
}

// --------------------------------------------------------------------------
// 3. decoder forward, softmax cross-entropy, dlogits / (n T)
// --------------------------------------------------------------------------
// grid (ceil(B*T/16), C), 4 waves: one tile of 16 (b, t) rows.  Wave w forms
// the logits of class tiles w, w + 4 into LDS; then it owns rows 4w .. 4w+3:
// lanes run along the classes, maximum and sum by butterfly (every lane gets
// the same bits).  lossp[tile] = the tile's row losses added in row order.
__global__ void __launch_bounds__(RNNROUND_THREADS) GRU_SCALAR_F32
rnn_dec_k(const RnnRoundArgs a, int s) {
  __shared__ float lg[16 * RNN_LG];
  __shared__ float rl[16];
  const int c = blockIdx.y;
  if (s >= mlp_nsteps(a.m, c)) return;
  const int n = rnn_nrows(a, c, s);
  const RnnLayout& L = a.lay;
  const int H = L.H, K = L.K, T = a.Tq;
  const int R = n * T, r0 = blockIdx.x * 16;
  if (r0 >= R) return;
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  const int lr = lane & 15, lk = lane >> 4;
  const float* Pm = a.m.replicas + (long)c * a.m.N;
  const float* Wd = Pm + L.off[RNN_DW];
  float* ws = a.m.ws + (long)c * L.ws_stride;
  const float* out = ws + L.out;
  float* dl = ws + L.dl;

  const int ra = r0 + lr;
  const bool rok = ra < R;
  for (int ct = wid; ct < (K + 15) / 16; ct += RNNROUND_THREADS / WAVE) {
    const int k = ct * 16 + lr;
    const bool kok = k < K;
    const float bk = kok ? Pm[L.off[RNN_DB] + k] : 0.f;
    gru_f4 acc = {bk, bk, bk, bk};
    for (int j0 = 0; j0 < H; j0 += 4) {
      const int j = j0 + lk;
      const float av = (rok && j < H) ? out[ra * H + j] : 0.f;
      const float bv = (kok && j < H) ? Wd[k * H + j] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
    }
    if (kok) {
#pragma unroll
      for (int i = 0; i < 4; ++i) lg[(4 * lk + i) * RNN_LG + k] = acc[i];
    }
  }
  __syncthreads();

  const float inv = 1.f / (float)R;
  for (int i = 0; i < 4; ++i) {
    const int row = 4 * wid + i, r = r0 + row;   // wave-uniform
    if (r >= R) {
      if (lane == 0) rl[row] = 0.f;
      continue;
    }
    const int b = r / T, t = r - b * T;
    const long dr = a.m.idx[((long)c * a.m.T + s) * a.m.B + b];
    const int y = a.tgt[dr * T + t];
    const float* x = lg + row * RNN_LG;
    const bool in0 = lane < K, in1 = lane + WAVE < K;
    const float x0 = in0 ? x[lane] : -INFINITY;
    const float x1 = in1 ? x[lane + WAVE] : -INFINITY;
    float mx = fmaxf(x0, x1);
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1)
      mx = fmaxf(mx, __shfl_xor(mx, o, WAVE));
    const float e0 = in0 ? expf(x0 - mx) : 0.f;
    const float e1 = in1 ? expf(x1 - mx) : 0.f;
    float sum = e0 + e1;
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, WAVE);
    const float rs = 1.f / sum;
    if (in0) dl[r * K + lane] = (e0 * rs - (lane == y ? 1.f : 0.f)) * inv;
    if (in1)
      dl[r * K + lane + WAVE] =
          (e1 * rs - (lane + WAVE == y ? 1.f : 0.f)) * inv;
    if (lane == 0)
      rl[row] = (mx + logf(sum)) - ((y >= 0 && y < K) ? x[y] : 0.f);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float sum = 0.f;
    for (int i = 0; i < 16; ++i) sum += rl[i];
    ws[L.lossp + blockIdx.x] = sum;
  }
}

// --------------------------------------------------------------------------
// the K-split reduce of gru_tok.h over the R = n T rows of a client
// --------------------------------------------------------------------------
// ROLE 0: A = am[r][arow], B = h_prev[r][bcol] (h0 / out, addressed)
// ROLE 1: A = (tokw[r] == arow), B = bm[r][bcol]
// ROLE 2: A = am[r][arow], B = bm[r][bcol]
template <int ROLE, bool WITH_DB>
__device__ __forceinline__ GRU_SCALAR_F32 void rnn_acc(
    gru_f4& acc, gru_f4& accb, const float* __restrict__ am, int lda,
    const float* __restrict__ bm, int ldb, const float* __restrict__ h0,
    const int* __restrict__ tokw, int R, int T, int arow, bool a_ok, int bcol,
    bool b_ok, int wid, int nw, int lk) {
  const int nsteps = (R + 3) >> 2;
  for (int q = wid; q < nsteps; q += RNN_U * nw) {
    float av[RNN_U], bv[RNN_U];
#pragma unroll
    for (int u = 0; u < RNN_U; ++u) {
      const int r = 4 * (q + u * nw) + lk;
      const bool in = r < R;
      if (ROLE == 1)
        av[u] = (in && a_ok && tokw[r] == arow) ? 1.f : 0.f;
      else
        av[u] = (in && a_ok) ? am[r * lda + arow] : 0.f;
      if (ROLE == 0) {
        float hv = 0.f;
        if (in && b_ok) {
          const int bb = r / T;
          hv = (r == bb * T) ? h0[bb * ldb + bcol] : bm[(r - 1) * ldb + bcol];
        }
        bv[u] = hv;
      } else {
        bv[u] = (in && b_ok) ? bm[r * ldb + bcol] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < RNN_U; ++u) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
      if (WITH_DB)
        accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], 1.f, accb, 0, 0,
                                                    0);
    }
  }
}

// merge the waves' accumulators in wave order; wave 0 stores the tile
// (row0, col0) of dst [nrow, ncol] and, with db, column 0 of accb
__device__ __forceinline__ GRU_SCALAR_F32 void rnn_merge_store(
    gru_f4 acc, gru_f4 accb, float (*red)[2][4][WAVE], float* dst, int nrow,
    int ncol, int row0, int col0, float* db) {
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  const int lr = lane & 15, lk = lane >> 4;
  if (wid > 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      red[wid - 1][0][i][lane] = acc[i];
      red[wid - 1][1][i][lane] = accb[i];
    }
  }
  __syncthreads();
  if (wid > 0) return;
  for (int w = 0; w + 1 < RNN_NW; ++w) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[i] += red[w][0][i][lane];
      accb[i] += red[w][1][i][lane];
    }
  }
  const int cc = col0 + lr;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rr = row0 + 4 * lk + i;
    if (rr < nrow) {
      if (cc < ncol) dst[rr * ncol + cc] = acc[i];
      if (db && lr == 0) db[rr] = accb[i];
    }
  }
}

// --------------------------------------------------------------------------
// 4. decoder backward: dW_d, db_d | dout
// --------------------------------------------------------------------------
// grid (ceil(K/16) ceil(H/16) + ceil(ceil(B*T/16) ceil(H/16) / RNN_NW), C),
// block 64 RNN_NW.  The first blocks own one tile of dW_d each (those of
// hidden tile 0 also db_d); in the others every wave owns one 16x16 tile of
// dout = dlogits W_d, K = classes.
__global__ void __launch_bounds__(RNN_NW * WAVE) GRU_SCALAR_F32
rnn_dec_bwd_k(const RnnRoundArgs a, int s) {
  __shared__ float red[RNN_NW - 1][2][4][WAVE];
  const int c = blockIdx.y;
  if (s >= mlp_nsteps(a.m, c)) return;
  const int n = rnn_nrows(a, c, s);
  const RnnLayout& L = a.lay;
  const int H = L.H, K = L.K, T = a.Tq, R = n * T;
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  const int lr = lane & 15, lk = lane >> 4;
  const int NHT = (H + 15) / 16, nW = ((K + 15) / 16) * NHT;
  const int bid = blockIdx.x;
  float* ws = a.m.ws + (long)c * L.ws_stride;
  const float* dl = ws + L.dl;
  const float* out = ws + L.out;
  if (bid < nW) {                       // block-uniform
    const int row0 = (bid / NHT) * 16, col0 = (bid % NHT) * 16;
    const int k = row0 + lr, j = col0 + lr;
    gru_f4 acc = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
    if (col0 == 0)
      rnn_acc<2, true>(acc, accb, dl, K, out, H, nullptr, nullptr, R, T, k,
                       k < K, j, j < H, wid, RNN_NW, lk);
    else
      rnn_acc<2, false>(acc, accb, dl, K, out, H, nullptr, nullptr, R, T, k,
                        k < K, j, j < H, wid, RNN_NW, lk);
    rnn_merge_store(acc, accb, red, ws + L.grad + L.off[RNN_DW], K, H, row0,
                    col0, col0 == 0 ? ws + L.grad + L.off[RNN_DB] : nullptr);
    return;
  }
  const int tile = (bid - nW) * RNN_NW + wid;
  if (tile >= ((R + 15) / 16) * NHT) return;
  const int r0 = (tile / NHT) * 16, j0 = (tile % NHT) * 16;
  const float* Wd = a.m.replicas + (long)c * a.m.N + L.off[RNN_DW];
  const int r = r0 + lr, j = j0 + lr;
  gru_f4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int k = k0 + lk;
    const float av = (r < R && k < K) ? dl[r * K + k] : 0.f;
    const float bv = (j < H && k < K) ? Wd[k * H + j] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
  }
  float* dout = ws + L.dout;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rr = r0 + 4 * lk + i;
    if (rr < R && j < H) dout[rr * H + j] = acc[i];
  }
}

// --------------------------------------------------------------------------
// 5. the sequence backward (gru_bwd_k of gru.h with the client axis)
// --------------------------------------------------------------------------
// grid (ceil(B/16), C), block 64*NT.  dgx, dgh [n, T, 3H].  The state is
// detached between steps: no dh0.
template <int NT>
__global__ void __launch_bounds__(NT * WAVE) GRU_SCALAR_F32
rnn_gru_bwd_k(const RnnRoundArgs a, int s) {
  constexpr int HP = NT * 16;
  constexpr int SB = (NT == 1) ? 16 : (NT == 4) ? 80 : 48;  // = 16 mod 32
  constexpr int SA = 3 * HP + 2;                            // 2 / 18 mod 32
  constexpr int NTHR = NT * WAVE;
  __shared__ float Ws[3 * HP * SB];          // [gate*HP + n][j]
  __shared__ float ds[2][GRU_ROWS * SA];     // [buffer][row][gate*HP + n]
  const int c = blockIdx.y;
  if (s >= mlp_nsteps(a.m, c)) return;
  const int n = rnn_nrows(a, c, s);
  const int b0 = blockIdx.x * GRU_ROWS;
  if (b0 >= n) return;
  const RnnLayout& L = a.lay;
  const int H = L.H, T = a.Tq;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wid = tid / WAVE;
  const int lr = lane & 15, lk = lane >> 4;
  const float* w = a.m.replicas + (long)c * a.m.N + L.off[RNN_WHH];
  float* ws = a.m.ws + (long)c * L.ws_stride;
  const float* dout = ws + L.dout;
  const float* out = ws + L.out;
  const float* gates = ws + L.gates;
  const float* h0 = ws + L.h0;
  float* dgx = ws + L.dgx;
  float* dgh = ws + L.dgh;

  for (int i = tid; i < 3 * HP * SB; i += NTHR) {
    const int row = i / SB, j = i - row * SB;
    const int g = row / HP, nn = row - g * HP;
    Ws[i] = (nn < H && j < H) ? w[(g * H + nn) * H + j] : 0.f;
  }
  for (int i = tid; i < GRU_ROWS * SA; i += NTHR) {
    ds[0][i] = 0.f;
    ds[1][i] = 0.f;
  }

  const int col = wid * 16 + lr;
  const bool lcol = col < H;
  bool live[4];
  int ob[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int b = b0 + 4 * lk + i;
    live[i] = lcol && b < n;
    ob[i] = b * T * H + col;
  }

  // operands of step t: gates (r, z, n, q), h_prev and dout
  float cr[4], cz[4], cn[4], cq[4], chp[4], cdo[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = ob[i] + (T - 1) * H;
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

  const float* wb = Ws + lk * SB + col;
  for (int t = T - 1; t >= 0; --t) {
    const int cur = t & 1;
    gru_f4 a0, a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f};
    float* dp = ds[cur] + (4 * lk) * SA + col;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float dh = cdo[i] + dhn[i];
      const float r = cr[i], z = cz[i], nv = cn[i];
      const float dn = dh * (1.f - z);
      const float dz = dh * (chp[i] - nv);
      float dan = dn * (1.f - nv * nv);
      float daz = dz * (z * (1.f - z));
      float dar = (dan * cq[i]) * (r * (1.f - r));
      float dhr = dan * r;
      float dhz = dh * z;
      if (live[i]) {
        const int o = (ob[i] + t * H) * 3 - 2 * col;
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
      const int o = ob[i] + (t - 1) * H;
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
    for (int kk = 0; kk < HP / 4; ++kk) {
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(
          da[kk * 4], wb[(kk * 4) * SB], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(
          da[HP + kk * 4], wb[(HP + kk * 4) * SB], a1, 0, 0, 0);
      a2 = __builtin_amdgcn_mfma_f32_16x16x4f32(
          da[2 * HP + kk * 4], wb[(2 * HP + kk * 4) * SB], a2, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      dhn[i] = (a0[i] + a1[i]) + a2[i];
      cr[i] = yr[i]; cz[i] = yz[i]; cn[i] = yn[i]; cq[i] = yq[i];
      chp[i] = yhp[i]; cdo[i] = ydo[i];
    }
  }
}

// --------------------------------------------------------------------------
// 6. dP (one-hot A operand), dW_hh, db_hh
// --------------------------------------------------------------------------
// grid (ceil(3H/16) ceil(H/16) + ceil(V/16) ceil(3H/16), C), block 64 RNN_NW:
// gru_tok_grads_k of gru_tok.h with the client axis.  A vocabulary row that
// no token selects is exact zeros.
__global__ void __launch_bounds__(RNN_NW * WAVE) GRU_SCALAR_F32
rnn_grads_k(const RnnRoundArgs a, int s) {
  __shared__ float red[RNN_NW - 1][2][4][WAVE];
  const int c = blockIdx.y;
  if (s >= mlp_nsteps(a.m, c)) return;
  const int n = rnn_nrows(a, c, s);
  const RnnLayout& L = a.lay;
  const int H = L.H, H3 = 3 * H, V = L.V, T = a.Tq, R = n * T;
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  const int lr = lane & 15, lk = lane >> 4;
  const int MT = (H3 + 15) / 16, NHT = (H + 15) / 16;
  const int bid = blockIdx.x;
  float* ws = a.m.ws + (long)c * L.ws_stride;
  const int* tokw = a.tokw + (long)c * a.m.B * T;
  gru_f4 acc = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
  if (bid < MT * NHT) {                 // block-uniform
    const int row0 = (bid / NHT) * 16, col0 = (bid % NHT) * 16;
    const int g = row0 + lr, j = col0 + lr;
    if (col0 == 0)
      rnn_acc<0, true>(acc, accb, ws + L.dgh, H3, ws + L.out, H, ws + L.h0,
                       tokw, R, T, g, g < H3, j, j < H, wid, RNN_NW, lk);
    else
      rnn_acc<0, false>(acc, accb, ws + L.dgh, H3, ws + L.out, H, ws + L.h0,
                        tokw, R, T, g, g < H3, j, j < H, wid, RNN_NW, lk);
    rnn_merge_store(acc, accb, red, ws + L.grad + L.off[RNN_WHH], H3, H, row0,
                    col0, col0 == 0 ? ws + L.grad + L.off[RNN_BHH] : nullptr);
  } else {
    const int id = bid - MT * NHT;
    const int row0 = (id / MT) * 16, col0 = (id % MT) * 16;
    const int v = row0 + lr, g = col0 + lr;
    rnn_acc<1, false>(acc, accb, nullptr, 0, ws + L.dgx, H3, nullptr, tokw, R,
                      T, v, v < V, g, g < H3, wid, RNN_NW, lk);
    rnn_merge_store(acc, accb, red, ws + L.dP, V, H3, row0, col0, nullptr);
  }
}

// --------------------------------------------------------------------------
// 7. backward of the table: dE = dP W_ih, dW_ih = dP^T E, db_ih = colsum dP
// --------------------------------------------------------------------------
// grid (ceil(tiles / 4), C), one 16x16 tile per wave: first the tiles of dE
// [V, H] (K = 3H), then those of dW_ih [3H, H] (K = V); the latter's hidden
// tile 0 also runs A against B = 1 for db_ih.  Pre-update E and W_ih.
__global__ void __launch_bounds__(RNNROUND_THREADS) GRU_SCALAR_F32
rnn_table_bwd_k(const RnnRoundArgs a, int s) {
  const int c = blockIdx.y;
  if (s >= mlp_nsteps(a.m, c)) return;
  const RnnLayout& L = a.lay;
  const int H = L.H, H3 = 3 * H, V = L.V;
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  const int lr = lane & 15, lk = lane >> 4;
  const int NHT = (H + 15) / 16, nE = ((V + 15) / 16) * NHT,
            nW = ((H3 + 15) / 16) * NHT;
  int tile = blockIdx.x * (RNNROUND_THREADS / WAVE) + wid;
  if (tile >= nE + nW) return;
  const float* Pm = a.m.replicas + (long)c * a.m.N;
  const float* E = Pm + L.off[RNN_ENC];
  const float* W = Pm + L.off[RNN_WIH];
  float* ws = a.m.ws + (long)c * L.ws_stride;
  const float* dP = ws + L.dP;
  float* grad = ws + L.grad;
  gru_f4 acc = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
  if (tile < nE) {                      // wave-uniform
    const int v0 = (tile / NHT) * 16, k0 = (tile % NHT) * 16;
    const int v = v0 + lr, k = k0 + lr;
    for (int j0 = 0; j0 < H3; j0 += 4) {
      const int j = j0 + lk;
      const float av = (v < V && j < H3) ? dP[v * H3 + j] : 0.f;
      const float bv = (k < H && j < H3) ? W[j * H + k] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int vv = v0 + 4 * lk + i;
      if (vv < V && k < H) grad[L.off[RNN_ENC] + vv * H + k] = acc[i];
    }
    return;
  }
  tile -= nE;
  const int j0 = (tile / NHT) * 16, k0 = (tile % NHT) * 16;
  const int j = j0 + lr, k = k0 + lr;
  const bool with_db = k0 == 0;
  for (int v0 = 0; v0 < V; v0 += 4) {
    const int v = v0 + lk;
    const float av = (j < H3 && v < V) ? dP[v * H3 + j] : 0.f;
    const float bv = (k < H && v < V) ? E[v * H + k] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
    if (with_db)
      accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av, 1.f, accb, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int jj = j0 + 4 * lk + i;
    if (jj < H3) {
      if (k < H) grad[L.off[RNN_WIH] + jj * H + k] = acc[i];
      if (with_db && lr == 0) grad[L.off[RNN_BIH] + jj] = accb[i];
    }
  }
}

// --------------------------------------------------------------------------
// 8. the SGD update of the seven tensors, hid_rows and the step's loss
// --------------------------------------------------------------------------
// grid (chunks, C).  Element i of the seven tensors laid end to end is arena
// element off[q] + i - start[q]; its gradient sits at the same arena index of
// the client's gradient workspace.  Pad gaps of the arena are not touched.
__global__ void __launch_bounds__(RNNROUND_THREADS) GRU_SCALAR_F32
rnn_update_k(const RnnRoundArgs a, int s) {
  const int c = blockIdx.y;
  if (s >= mlp_nsteps(a.m, c)) return;
  const RnnLayout& L = a.lay;
  float* ws = a.m.ws + (long)c * L.ws_stride;
  const float* grad = ws + L.grad;
  const MlpSgd u = mlp_sgd<false>(a.m, c, s);
  const MlpCorr none = {0.f, 0.f};
  for (int i = blockIdx.x * RNNROUND_THREADS + threadIdx.x;
       i < L.start[RNN_NTENS]; i += gridDim.x * RNNROUND_THREADS) {
    int q = 0;
#pragma unroll
    for (int t = 1; t < RNN_NTENS; ++t) q += i >= L.start[t];
    const int e = L.off[q] + i - L.start[q];
    mlp_update<false>(u, e, u.p[e], grad[e], none);
  }
  if (blockIdx.x == 0 && threadIdx.x < WAVE) {
    const int n = rnn_nrows(a, c, s);
    if (threadIdx.x == 0) {
      const int R = n * a.Tq;
      float sum = 0.f;
      for (int t = 0; t < (R + 15) / 16; ++t) sum += ws[L.lossp + t];
      a.m.loss[(long)c * a.m.T + s] = R > 0 ? sum * (1.f / (float)R) : 0.f;
      a.hid_rows[c] = n;
    }
  }
}
