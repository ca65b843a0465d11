// A whole federated round of local SGD for packed LINEAR models (logistic
// regression / least squares) in ONE launch: one workgroup of 256 threads per
// virtual client, the client's weight [K, F], bias [K] and momentum buffer
// resident in LDS as fp32 over all of the round's steps.
//
//   for each client c with steps[c] > 0 (others: nothing read or written):
//     W, b <- server[w_off ..], server[b_off ..]
//     for s in 0 .. steps[c]-1, over the rows r = idx[c, s, :] >= 0:
//       [snapshot]  snap[c] <- parameters, if s + 1 == k_cut
//       logits = x W^T + b
//       loss[c, s] = mean CE(logits, y)   (loss_kind 0)
//                  = mean (logits - y)^2  (loss_kind 1, K == 1)
//       dW = dlogits^T x,  db = sum_rows dlogits
//       d = g ; [delta] d -= delta[c] ; [control pair] d += c - c_c[c] ;
//       [prox_mu] d += mu (p - server)   -- fused_sgd_step's corrections
//       d += wd p ; first use: buf = d, else buf = m buf + (1 - damp) d
//       d = nesterov ? d + m buf : buf ; p -= lr[c, s] d
//     replicas[c] <- parameters (pad gaps copied from server)
//     in_mom[c]   <- buf, mom_init[c] <- 1            (with momentum only)
//
// LDS image: P[f][k] with row stride KS = K | 1 (odd), f = 0 .. F, where row
// F is the bias -- the bias is the weight of a constant feature 1.  Lanes
// that differ in f touch banks (f KS + k) mod 32: all distinct within a half
// wave because KS is odd, so the ds_read_b32 / ds_write_b32 of both products
// are conflict-free, and k is an immediate offset.  The momentum image has
// the same shape.
//
// Phases of a step (three barriers):
//   forward   wave w takes rows w, w+4, ...; lanes stride over f, read x
//             coalesced from global and P[f][.] from LDS, keep K
//             accumulators, finish with a wave64 shuffle reduce; lane 0 adds
//             the bias and stores logits[row][k].
//   loss      thread t takes row t: softmax / squared error, the row's loss
//             and dlogits[row][k] (already divided by the row count) to LDS.
//   backward  thread t owns features f = t, t+256, ... (f = F: the bias):
//             loops over the rows IN ORDER, re-reads x[row][f] (an L2 hit),
//             takes dlogits as an LDS broadcast and applies the SGD update
//             to its own P[f][.] in LDS.  A gradient correction is constant
//             over the round and only its owner thread needs it, so it stays
//             in global memory: the K values of the feature (elements
//             k F + f, coalesced across threads for each k; the bias takes
//             b_off + k) are loaded ahead of the row loop, whose B re-reads
//             of x cover their latency.  The LDS image is the same with and
//             without a correction.
//
// No atomics; every summation order is fixed by (F, K, B), so two runs are
// bit-identical.  No host reads, no synchronisation: capture-safe.  Padding
// samples (idx < 0) are never dereferenced; a row id >= M is treated as
// padding as well, so the kernel cannot read outside X whatever idx holds
// (the launcher rejects such idx when it may read it).  The loads of a
// padding sample are redirected to row 0 of X and their value discarded.
//
// Limits (checked by the launcher): 1 <= K <= 16, F >= 1, and
//   (1 + momentum) (F + 1) (K | 1) + B (K + 2)  <=  LINROUND_LDS_FLOATS
// floats of LDS: the kernel declares 159 KiB statically, which a single
// workgroup can get on gfx950 (one workgroup per CU).  K is a template
// parameter (16 instantiations), so the k loops unroll without guards.
// A correction adds no limit: it is never staged in LDS.  Its rows are only
// read for clients with steps > 0, and only at weight and bias elements.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "common.h"

#define LINROUND_THREADS 256
#define LINROUND_MAXK 16
#define LINROUND_LDS_FLOATS 40704  // floats: 159 KiB of the CU's 160 KiB
// gradient corrections of a round (LinRoundArgs.corr, the same in all blocks)
#define LINROUND_DELTA 1
#define LINROUND_CTRL 2
#define LINROUND_PROX 4

// wave64 sum in a fixed order, the total lands in lane 0
__device__ __forceinline__ float linround_wave_sum(float v) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1)
    v += __shfl_down(v, off, WAVE);
  return v;
}

struct LinRoundArgs {
  const float* X;        // [M, F]
  const void* Y;         // [M] int32 class ids or fp32 targets
  const int* idx;        // [C, T, B]
  const int* steps;      // [C]
  const float* lr;       // [C, T]
  const float* server;   // [N]
  float* replicas;       // [C, N]
  float* in_mom;         // [C, N] or null
  int* mom_init;         // [C]
  float* snap;           // [C, N] or null
  float* loss;           // [C, T]
  const float* corr_rows;  // [C, N] or null: delta (d -= delta[c]) or, with
  const float* ctrl_s;     // ctrl_s [N], the client controls (d += c - c_c[c])
  int M, F, B, T;
  int N, w_off, b_off;   // the arena and the offsets of weight and bias
  int k_cut, use_mom, nesterov;
  float wd, mom, omd;    // omd = 1 - dampening
  float prox_mu;         // != 0: d += prox_mu (p - server)
  int corr;              // LINROUND_DELTA | _CTRL | _PROX, 0: no correction
};

// LDS element of arena element i, or -1 for a pad gap
template <int K>
__device__ __forceinline__ int linround_slot(int i, int w_off, int b_off,
                                             int F) {
  constexpr int KS = K | 1;
  const int iw = i - w_off, ib = i - b_off;
  if (iw >= 0 && iw < K * F) {
    const int k = iw / F;
    return (iw - k * F) * KS + k;
  }
  if (ib >= 0 && ib < K) return F * KS + ib;
  return -1;
}

// LOSS 0: softmax cross-entropy, 1: squared error (K == 1)
template <int K, int LOSS>
__global__ void __launch_bounds__(LINROUND_THREADS)
linear_round_k(const LinRoundArgs a) {
  constexpr int KS = K | 1;
  __shared__ float sm[LINROUND_LDS_FLOATS];
  const int c = blockIdx.x;
  const int ns = min(a.steps[c], a.T);       // never past idx / lr / loss
  if (ns <= 0) return;                       // offline: untouched (uniform)
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wid = tid / WAVE;
  const int F = a.F, B = a.B;
  const int np = (F + 1) * KS;
  float* Ps = sm;                            // parameters [F + 1][KS]
  float* Ms = sm + np;                       // momentum   [F + 1][KS]
  float* zs = sm + (a.use_mom ? 2 * np : np);  // logits / dlogits [B][K]
  float* ls = zs + B * K;                    // per-row loss [B]
  int* is = reinterpret_cast<int*>(ls + B);  // row ids of the step [B]

  // per-thread bases of the arena rows (element tid): the copies below step
  // through them in strides of the block, o = i - tid
  const float* srv = a.server + tid;
  float* rep = a.replicas + (long)c * a.N + tid;
  float* mo = a.use_mom ? a.in_mom + (long)c * a.N + tid : nullptr;
  float* sp = a.snap ? a.snap + (long)c * a.N + tid : nullptr;
  float* lo = a.loss + (long)c * a.T + tid;   // used by thread 0 alone
  int* mi = a.mom_init + c + tid;            // likewise
  // the correction's rows likewise: the kernel has no scalar register to
  // spare, and a per-thread base lives in a vector register
  const float* cr = a.corr ? a.corr_rows + (long)c * a.N + tid : nullptr;
  const float* cs = a.corr ? a.ctrl_s + tid : nullptr;
  const int ow = a.w_off - tid, ob = a.b_off - tid;  // arena offsets likewise
  const bool had_mom = a.use_mom && a.mom_init[c] != 0;

  // parameters (and momentum) in; pad gaps of the arena pass through
  for (int o = 0; o + tid < a.N; o += LINROUND_THREADS) {
    const int j = linround_slot<K>(o + tid, a.w_off, a.b_off, F);
    const float v = srv[o];
    if (j < 0) {
      rep[o] = v;
    } else {
      Ps[j] = v;
      if (a.use_mom) Ms[j] = had_mom ? mo[o] : 0.f;
    }
  }
  __syncthreads();

  for (int s = 0; s < ns; ++s) {
    const int* ids = a.idx + ((long)c * a.T + s) * B;
    const float lr = a.lr[(long)c * a.T + s];
    // first use of the buffer: buf = 0 * 0 + 1 * d
    const bool first = a.use_mom && !had_mom && s == 0;
    const float mom = first ? 0.f : a.mom, omd = first ? 1.f : a.omd;

    if (sp && s + 1 == a.k_cut) {
      for (int o = 0; o + tid < a.N; o += LINROUND_THREADS) {
        const int j = linround_slot<K>(o + tid, a.w_off, a.b_off, F);
        sp[o] = j < 0 ? srv[o] : Ps[j];
      }
    }

    // ---- forward: one wave per row ------------------------------------
    for (int b = wid; b < B; b += LINROUND_THREADS / WAVE) {
      int r = ids[b];
      if (r >= a.M) r = -1;
      if (lane == 0) is[b] = r;
      const float* xr = a.X + (long)(r < 0 ? 0 : r) * F;
      float acc[K];
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = 0.f;
      for (int f = lane; f < F; f += WAVE) {
        const float xv = xr[f];
        const float* pf = Ps + f * KS;
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = fmaf(xv, pf[k], acc[k]);
      }
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float t = linround_wave_sum(acc[k]);
        if (lane == 0) zs[b * K + k] = r < 0 ? 0.f : t + Ps[F * KS + k];
      }
    }
    __syncthreads();

    // ---- loss and dlogits: one thread per row -------------------------
    int nv = 0;
    for (int b = 0; b < B; ++b) nv += is[b] >= 0;
    const float inv = nv > 0 ? 1.f / (float)nv : 0.f;
    for (int b = tid; b < B; b += LINROUND_THREADS) {
      const int r = is[b];
      float* z = zs + b * K;
      float lrow = 0.f;
      if (r < 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) z[k] = 0.f;
      } else if (LOSS == 0) {
        const int y = reinterpret_cast<const int*>(a.Y)[r];
        const bool yok = y >= 0 && y < K;
        float mx = z[0];
#pragma unroll
        for (int k = 1; k < K; ++k) mx = fmaxf(mx, z[k]);
        float e[K], sum = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          e[k] = expf(z[k] - mx);
          sum += e[k];
        }
        lrow = (logf(sum) + mx) - (yok ? z[y] : 0.f);
        const float rs = 1.f / sum;
#pragma unroll
        for (int k = 0; k < K; ++k) z[k] = e[k] * rs;
        if (yok) z[y] -= 1.f;
#pragma unroll
        for (int k = 0; k < K; ++k) z[k] *= inv;
      } else {
        const float d = z[0] - reinterpret_cast<const float*>(a.Y)[r];
        lrow = d * d;
        z[0] = (2.f * d) * inv;
      }
      ls[b] = lrow;
    }
    __syncthreads();

    if (tid == 0) {                          // fixed-order mean of the rows
      float t = 0.f;
      for (int b = 0; b < B; ++b) t += ls[b];
      lo[s] = t * inv;
    }

    // ---- backward + SGD: one thread per feature (f == F: the bias) -----
    // Two copies of the phase, chosen by the block-uniform a.corr: without a
    // correction the code, and so the arithmetic and the registers of the
    // row loop, are the ones of a kernel that knows no correction.
    auto backward = [&](auto with_corr) {
      constexpr bool CORR = decltype(with_corr)::value;
      for (int f = tid; f <= F; f += LINROUND_THREADS) {
        const bool isb = f == F;
        const float* xc = a.X + (isb ? 0 : f);
        float g[K];
#pragma unroll
        for (int k = 0; k < K; ++k) g[k] = 0.f;
        // the correction of this feature: issued here, used after the rows
        float cv[K], sv[K];
        if (CORR) {
          // element of (f, k) relative to the per-thread bases: o0 + k es
          const int o0 = isb ? ob : ow + f;
          const int es = isb ? 1 : F;
#pragma unroll
          for (int k = 0; k < K; ++k) cv[k] = sv[k] = 0.f;
          if (a.corr & LINROUND_DELTA) {
#pragma unroll
            for (int k = 0; k < K; ++k) cv[k] = cr[o0 + k * es];
          } else if (a.corr & LINROUND_CTRL) {
#pragma unroll
            for (int k = 0; k < K; ++k)
              cv[k] = cs[o0 + k * es] - cr[o0 + k * es];
          }
          if (a.corr & LINROUND_PROX) {
#pragma unroll
            for (int k = 0; k < K; ++k) sv[k] = srv[o0 + k * es];
          }
        }
        for (int b = 0; b < B; ++b) {
          const int r = is[b];
          const float t = xc[(long)(r < 0 ? 0 : r) * F];
          const float xv = r < 0 ? 0.f : (isb ? 1.f : t);
          const float* zb = zs + b * K;
#pragma unroll
          for (int k = 0; k < K; ++k) g[k] = fmaf(zb[k], xv, g[k]);
        }
        float* pf = Ps + f * KS;
        float* mf = Ms + f * KS;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float p = pf[k];
          float d = g[k];
          if (CORR) {
            if (a.corr & LINROUND_DELTA) d -= cv[k];
            else if (a.corr & LINROUND_CTRL) d += cv[k];
            if (a.corr & LINROUND_PROX) d = fmaf(a.prox_mu, p - sv[k], d);
          }
          d = fmaf(a.wd, p, d);
          if (a.use_mom) {
            const float bu = fmaf(mom, mf[k], omd * d);
            mf[k] = bu;
            d = a.nesterov ? fmaf(a.mom, bu, d) : bu;
          }
          pf[k] = fmaf(-lr, d, p);
        }
      }
    };
    if (a.corr) backward(std::true_type());
    else backward(std::false_type());
    __syncthreads();
  }

  // parameters (and momentum) out
  for (int o = 0; o + tid < a.N; o += LINROUND_THREADS) {
    const int j = linround_slot<K>(o + tid, a.w_off, a.b_off, F);
    if (j >= 0) {
      rep[o] = Ps[j];
      if (a.use_mom) mo[o] = Ms[j];
    }
  }
  if (a.use_mom && tid == 0) mi[0] = 1;
}
