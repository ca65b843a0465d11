// Persistent single-layer GRU sequence kernels for gfx950 (PyTorch gate order
// r, z, n; weight_hh [3H, H]).  The input projection gx = x W_ih^T + b_ih of
// all T steps is computed beforehand by one library GEMM; these kernels run
// the sequential part, all T steps inside ONE launch:
//
//   r = sigmoid(gx_r + W_hr h + b_hr)      z = sigmoid(gx_z + W_hz h + b_hz)
//   q = W_hn h + b_hn                      n = tanh(gx_n + r * q)
//   h' = (1 - z) * n + z * h
//
//   gru_fwd_k<NT>  one workgroup per 16 batch rows, NT = ceil(H/16) waves.
//                  W_hh sits in LDS as fp32, padded to HP = 16*NT in both
//                  dimensions with the pad ZERO-filled; h is double-buffered
//                  in LDS as the MFMA A operand.  Wave w owns the r, z and n
//                  accumulator tiles of hidden columns [16w, 16w+16), so the
//                  gate math and the h_prev it needs are lane-local and
//                  h_prev stays in registers over the steps.  One barrier
//                  per step.
//   gru_bwd_k<NT>  the mirror over the same batch tiles, t = T-1 .. 0:
//                    dh   = dout[:, t] + dh_next
//                    da_n = dh (1 - z) (1 - n^2)
//                    da_z = dh (h_prev - n) z (1 - z)
//                    da_r = da_n q r (1 - r)
//                    dgx[t] = (da_r, da_z, da_n)
//                    dgh[t] = (da_r, da_z, da_n r)
//                    dh_next = dh z + dgh[t] . W_hh        (K = 3 HP)
//                  dgh[t] is double-buffered in LDS as the A operand, W_hh
//                  is the B operand in its natural [k][n] layout.
//
// The products are v_mfma_f32_16x16x4_f32: bit-for-bit a k-ordered fp32 fmaf
// chain, so small-integer data gives exact results.  Lane l of a wave holds
// A[row l&15][k l>>4], B[k l>>4][col l&15] and the four accumulator elements
// C[row 4*(l>>4)+i][col l&15].
//
// No atomics; every summation order is fixed by H alone, so two runs are
// bit-identical.  No host reads, no synchronisation: both are capture-safe.
// w_hh / b_hh are read as bf16 or fp32 (independently) with element loads --
// nothing beyond the natural element alignment is assumed.  Batch pad rows
// (b >= B) and pad columns (>= H) are never loaded and never stored; they
// carry zeros through the LDS operands.
//
// Limits (checked by the launchers): 1 <= H <= 64, T >= 1, B >= 1.
// LDS row strides are chosen so that the ds_read_b32 operand fetches (banks
// = dword address mod 32 within each half wave) are conflict-free.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"
#include <hip/hip_bf16.h>

#define GRU_MAXH 64
#define GRU_ROWS 16

typedef float gru_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float gru_ld1(const void* p, long i, int bf16) {
  return bf16 ? __bfloat162float(
                    reinterpret_cast<const __hip_bfloat16*>(p)[i])
              : reinterpret_cast<const float*>(p)[i];
}
__device__ __forceinline__ float gru_sigmoid(float a) {
  return 1.f / (1.f + expf(-a));
}

// --------------------------------------------------------------------------
// forward
// --------------------------------------------------------------------------
// grid ceil(B/16), block 64*NT.  gates [B, T, 4, H] = (r, z, n, q) or null.
template <int NT>
__global__ void __launch_bounds__(NT * WAVE)
gru_fwd_k(const float* __restrict__ gx, const void* __restrict__ w,
          int w_bf16, const void* __restrict__ bias, int b_bf16,
          const float* __restrict__ h0, float* __restrict__ out,
          float* __restrict__ gates, int B, int T, int H) {
  constexpr int HP = NT * 16;
  constexpr int S = HP + 2;             // S mod 32 in {2, 18}
  constexpr int NTHR = NT * WAVE;
  __shared__ float Ws[3 * HP * S];      // [gate][n][k]
  __shared__ float hs[2][GRU_ROWS * S];  // [buffer][row][k]
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wid = tid / WAVE;
  const int lr = lane & 15, lk = lane >> 4;
  const long b0 = (long)blockIdx.x * GRU_ROWS;

  for (int i = tid; i < 3 * HP * S; i += NTHR) {
    const int g = i / (HP * S), rem = i - g * (HP * S);
    const int n = rem / S, k = rem - n * S;
    Ws[i] = (n < H && k < H) ? gru_ld1(w, ((long)g * H + n) * H + k, w_bf16)
                             : 0.f;
  }
  for (int i = tid; i < GRU_ROWS * S; i += NTHR) {
    const int m = i / S, k = i - m * S;
    hs[0][i] = (b0 + m < B && k < H) ? h0[(b0 + m) * H + k] : 0.f;
    hs[1][i] = 0.f;
  }

  const int col = wid * 16 + lr;        // hidden column of this lane
  const bool lcol = col < H;
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
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float* p = gx + ob[i] * 3 - 2 * col;   // (b*T + 0)*3H + col
    xr[i] = live[i] ? p[0] : 0.f;
    xz[i] = live[i] ? p[H] : 0.f;
    xn[i] = live[i] ? p[2 * H] : 0.f;
  }
  __syncthreads();

  const float* wr = Ws + (0 * HP + col) * S + lk;
  const float* wz = Ws + (1 * HP + col) * S + lk;
  const float* wn = Ws + (2 * HP + col) * S + lk;
  for (int t = 0; t < T; ++t) {
    const int cur = t & 1;
    // next step's input projection, in flight during the MFMAs
    float yr[4], yz[4], yn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ld = live[i] && t + 1 < T;
      const float* p = gx + (ob[i] + (long)(t + 1) * H) * 3 - 2 * col;
      yr[i] = ld ? p[0] : 0.f;
      yz[i] = ld ? p[H] : 0.f;
      yn[i] = ld ? p[2 * H] : 0.f;
    }
    gru_f4 ar = {br, br, br, br}, az = {bz, bz, bz, bz},
           an = {bn, bn, bn, bn};
    const float* ha = hs[cur] + lr * S + lk;
#pragma unroll
    for (int kk = 0; kk < HP / 4; ++kk) {
      const float a = ha[kk * 4];
      ar = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wr[kk * 4], ar, 0, 0, 0);
      az = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wz[kk * 4], az, 0, 0, 0);
      an = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wn[kk * 4], an, 0, 0, 0);
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
    }
    __syncthreads();
  }
}

// --------------------------------------------------------------------------
// backward
// --------------------------------------------------------------------------
// grid ceil(B/16), block 64*NT.  dgx, dgh [B, T, 3H]; dh0 [B, H].
template <int NT>
__global__ void __launch_bounds__(NT * WAVE)
gru_bwd_k(const float* __restrict__ dout, const float* __restrict__ out,
          const float* __restrict__ gates, const void* __restrict__ w,
          int w_bf16, const float* __restrict__ h0, float* __restrict__ dgx,
          float* __restrict__ dgh, float* __restrict__ dh0, int B, int T,
          int H) {
  constexpr int HP = NT * 16;
  constexpr int SB = (NT == 1) ? 16 : (NT == 4) ? 80 : 48;  // = 16 mod 32
  constexpr int SA = 3 * HP + 2;                            // 2 / 18 mod 32
  constexpr int NTHR = NT * WAVE;
  __shared__ float Ws[3 * HP * SB];          // [gate*HP + n][j]
  __shared__ float ds[2][GRU_ROWS * SA];     // [buffer][row][gate*HP + n]
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wid = tid / WAVE;
  const int lr = lane & 15, lk = lane >> 4;
  const long b0 = (long)blockIdx.x * GRU_ROWS;

  for (int i = tid; i < 3 * HP * SB; i += NTHR) {
    const int row = i / SB, j = i - row * SB;
    const int g = row / HP, n = row - g * HP;
    Ws[i] = (n < H && j < H) ? gru_ld1(w, ((long)g * H + n) * H + j, w_bf16)
                             : 0.f;
  }
  for (int i = tid; i < GRU_ROWS * SA; i += NTHR) {
    ds[0][i] = 0.f;
    ds[1][i] = 0.f;
  }

  const int col = wid * 16 + lr;
  const bool lcol = col < H;
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

  const float* wb = Ws + lk * SB + col;
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
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (live[i]) dh0[(b0 + 4 * lk + i) * H + col] = dhn[i];
}
