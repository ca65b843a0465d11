// The two sequence kernels of the packed char-GRU round (rnnround.h) for
// 65 <= H <= 128: rnn_gru_fwd_k / rnn_gru_bwd_k with the work split of
// gru_fwd_reg_k<NT, true> / gru_bwd_reg_k<NT> (gru_wide.h).
//
// At H = 128 the fp32 LDS image of W_hh that rnnround.h keeps is 199,680 B,
// more than a CU has.  W_hh[c] is constant over the T steps of a local step
// and only ever the MFMA B operand, so every lane loads its own B fragments
// from replicas[c] + off[RNN_WHH] once, before the T-loop, and keeps them in
// registers:
//
//   rnn_gru_fwd_reg_k<NT>  lane (lk = l>>4, lr = l&15) of wave w holds
//                          W[g][col = 16w + lr][k = lk + 4 kk], g in 0..2,
//                          kk in 0..HP/4-1: 3 HP / 4 registers.  LDS holds
//                          only the double-buffered h tile, 2 x 16 x (HP + 2)
//                          floats.  One ds_read_b32 of A feeds three MFMAs;
//                          one barrier per step.
//   rnn_gru_bwd_reg_k<NT>  the mirror: W[g][k = 4 kk + lk][col]; dgh[t]
//                          double-buffered in LDS as the A operand, row
//                          stride 3 HP + 2.  Accumulators added (a0 + a1) +
//                          a2 with a0 seeded by dh z; no dh0 (the state is
//                          detached between steps).
//
// grid (ceil(B/16), C), block 64 NT, NT = ceil(H/16) in 5..8.  A block returns
// at once, uniformly, for s >= steps[c] and for a batch tile past n.  The
// other six kernels of the step take their tile counts from H and are those
// of rnnround.h.  Everything a kernel of rnnround.h promises holds here: the
// hidden rule (hidden[c, :n] if hid_rows[c] == n, else zeros), tokens through
// idx[c, s, b] and prefetched two steps ahead, a token outside [0, V) reads
// gx = 0 and is kept as -1 in tokw, accumulators seeded with b_hh; rows >= n
// and columns >= H are never loaded (their operand is 0) and never stored; no
// atomics, the k-ordered v_mfma_f32_16x16x4_f32 chains fix the summation
// order by H, no host reads.
//
// A 512-thread workgroup is 2 waves per SIMD, so a wave may use up to 256
// VGPR; the weight arrays are indexed with compile-time constants only (every
// loop over them is fully unrolled) so that they never go to scratch.  The
// per-row address state is 32-bit: the launcher bounds M T below 2^31 and the
// workspace below 2^30 floats.  Resources of the eight instantiations:
// scratch 0, spills 0 (profiles/packed_rnn_notes.md).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "gru_wide.h"
#include "rnnround.h"

#define RNNROUND_WIDE_MINH GRU_WIDE_MINH
#define RNNROUND_WIDE_MAXH GRU_WIDE_MAXH

// --------------------------------------------------------------------------
// the sequence forward
// --------------------------------------------------------------------------
// Writes out [n, T, H], gates [n, T, 4, H] = (r, z, n, q), h0 [n, H] (the
// state the step started from), tokw and hidden[c] -- rows of its own tile
// only.
template <int NT>
__global__ void __launch_bounds__(NT * WAVE) GRU_SCALAR_F32
rnn_gru_fwd_reg_k(const RnnRoundArgs a, int s) {
  constexpr int HP = NT * 16;
  constexpr int KK = HP / 4;
  constexpr int S = HP + 2;             // S mod 32 in {2, 18}
  constexpr int NTHR = NT * WAVE;
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
  const float* bias = Pm + L.off[RNN_BHH];
  float* ws = a.m.ws + (long)c * L.ws_stride;
  const float* P = ws + L.P;
  float* out = ws + L.out;
  float* gates = ws + L.gates;
  float* hid = a.hidden + (long)c * a.m.B * H;
  int* tokw = a.tokw + (long)c * a.m.B * T;
  const bool keep = a.hid_rows[c] == n;   // else init_hidden: zeros
  const int col = wid * 16 + lr;        // hidden column of this lane
  const bool lcol = col < H;

  // B fragments W[g][col][lk + 4 kk], resident for all T steps
  float wf[3][KK];
  gru_wide_frag<KK, float>(wf, Pm + L.off[RNN_WHH], H, col, 0, lk, 4);

  for (int i = tid; i < GRU_ROWS * S; i += NTHR) {
    const int m = i / S, k = i - m * S;
    hs[0][i] = (keep && b0 + m < n && k < H) ? hid[(b0 + m) * H + k] : 0.f;
    hs[1][i] = 0.f;
  }

  bool live[4];
  int ob[4];                            // (b*T)*H + col
  int tb[4];                            // the row's first token in a.tok
  float hprev[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int b = b0 + 4 * lk + i;
    live[i] = lcol && b < n;
    ob[i] = b * T * H + col;
    hprev[i] = (live[i] && keep) ? hid[b * H + col] : 0.f;
    if (live[i]) ws[L.h0 + b * H + col] = hprev[i];
    tb[i] = live[i] ? a.m.idx[((long)c * a.m.T + s) * a.m.B + b] * T : 0;
  }
  const float br = lcol ? bias[col] : 0.f;
  const float bz = lcol ? bias[H + col] : 0.f;
  const float bn = lcol ? bias[2 * H + col] : 0.f;

  const bool st = col == 0;             // this lane keeps its rows' tokens
  const int kb = (b0 + 4 * lk) * T;     // tokw index of this lane's row 0
  float xr[4], xz[4], xn[4];
  int tk[4];                            // token of step t + 1, or -1
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = rnn_tok(a.tok, tb[i], live[i], V, tokw, kb + i * T, st);
    tk[i] = rnn_tok(a.tok, (long)tb[i] + 1, live[i] && 1 < T, V, tokw,
                    kb + i * T + 1, st);
    const float* p = P + v * H3 + col;
    xr[i] = v >= 0 ? p[0] : 0.f;
    xz[i] = v >= 0 ? p[H] : 0.f;
    xn[i] = v >= 0 ? p[2 * H] : 0.f;
  }
  __syncthreads();

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
      tn[i] = rnn_tok(a.tok, (long)tb[i] + t + 2, live[i] && t + 2 < T, V,
                      tokw, kb + i * T + t + 2, st);
    }
    gru_f4 ar = {br, br, br, br}, az = {bz, bz, bz, bz},
           an = {bn, bn, bn, bn};
    const float* ha = hs[cur] + lr * S + lk;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const float av = ha[kk * 4];
      ar = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wf[0][kk], ar, 0, 0, 0);
      az = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wf[1][kk], az, 0, 0, 0);
      an = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wf[2][kk], an, 0, 0, 0);
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
// the sequence backward
// --------------------------------------------------------------------------
// dgx, dgh [n, T, 3H], rows of its own tile only.
template <int NT>
__global__ void __launch_bounds__(NT * WAVE) GRU_SCALAR_F32
rnn_gru_bwd_reg_k(const RnnRoundArgs a, int s) {
  constexpr int HP = NT * 16;
  constexpr int KK = HP / 4;
  constexpr int SA = 3 * HP + 2;             // 2 / 18 mod 32
  constexpr int NTHR = NT * WAVE;
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
  float* ws = a.m.ws + (long)c * L.ws_stride;
  const float* dout = ws + L.dout;
  const float* out = ws + L.out;
  const float* gates = ws + L.gates;
  const float* h0 = ws + L.h0;
  float* dgx = ws + L.dgx;
  float* dgh = ws + L.dgh;
  const int col = wid * 16 + lr;
  const bool lcol = col < H;

  // B fragments W[g][4 kk + lk][col], resident for all T steps
  float wf[3][KK];
  gru_wide_frag<KK, float>(
      wf, a.m.replicas + (long)c * a.m.N + L.off[RNN_WHH], H, lk, 4, col, 0);

  for (int i = tid; i < GRU_ROWS * SA; i += NTHR) {
    ds[0][i] = 0.f;
    ds[1][i] = 0.f;
  }

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
}
