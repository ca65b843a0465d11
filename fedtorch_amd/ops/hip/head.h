// Classifier tail for gfx950: global average pool + FC head (fwd/bwd) and
// the on-device loss / top-k accumulator of the validation pass.
//
//   head_fwd_k     one workgroup per sample: pool the NHWC map into LDS with
//                  16-byte loads along C, then one wave per output class
//                  (lanes over C, wave64 shuffle reduce).
//   head_dx_k      one workgroup per sample: g[c] = sum_k dl[n,k] w[k,c] / HW
//                  into LDS, then broadcast over the pixels with 16-byte
//                  stores.
//   head_dwdb_k    one workgroup per (class, 64-channel tile): the 4 waves
//                  take 4 contiguous slices of N, their partials are summed
//                  through LDS in wave order.
//   ce_topk_k      ONE workgroup, one wave per sample in turn; thread 0 adds
//                  the batch's (loss_sum, top1, top5, n) into the fp64
//                  accumulator, so stream order serialises the batches.
//
// No atomics anywhere and every summation order is fixed by the launch
// geometry (which depends on the shapes alone): two runs are bit-identical.
// All accumulation is fp32; x / weight / bias are read in their own dtype
// (bf16 or fp32, independently), so neither the autocast case (fp32 fc) nor
// the bf16 twin arena needs a cast kernel.
//
// Limits (checked by the launchers): C % 8 == 0, 8 <= C <= 1024,
// 1 <= K <= 1024; x, weight and dx are 16-byte aligned.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"
#include <hip/hip_bf16.h>

#define HEAD_MAXC 1024
#define HEAD_MAXK 1024
#define HEAD_CE_BLOCK 1024

// 8 consecutive elements of a bf16 / fp32 row as fp32 (16 / 2x16 bytes)
__device__ __forceinline__ void head_ld8(const float* __restrict__ p,
                                         float* v) {
  const float4 a = reinterpret_cast<const float4*>(p)[0];
  const float4 b = reinterpret_cast<const float4*>(p)[1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void head_ld8(const __hip_bfloat16* __restrict__ p,
                                         float* v) {
  struct alignas(16) V8 { __hip_bfloat16 d[8]; };
  const V8 a = *reinterpret_cast<const V8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = __bfloat162float(a.d[j]);
}
__device__ __forceinline__ void head_st8(float* __restrict__ p,
                                         const float* v) {
  reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ void head_st8(__hip_bfloat16* __restrict__ p,
                                         const float* v) {
  struct alignas(16) V8 { __hip_bfloat16 d[8]; };
  V8 a;
#pragma unroll
  for (int j = 0; j < 8; ++j) a.d[j] = __float2bfloat16(v[j]);  // RNE
  *reinterpret_cast<V8*>(p) = a;
}
__device__ __forceinline__ float head_ld1(const void* p, long i, int bf16) {
  return bf16 ? __bfloat162float(
                    reinterpret_cast<const __hip_bfloat16*>(p)[i])
              : reinterpret_cast<const float*>(p)[i];
}
__device__ __forceinline__ void head_st1(void* p, long i, int bf16, float v) {
  if (bf16)
    reinterpret_cast<__hip_bfloat16*>(p)[i] = __float2bfloat16(v);
  else
    reinterpret_cast<float*>(p)[i] = v;
}

__device__ __forceinline__ int head_wave_sum_i(int v) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1)
    v += __shfl_down(v, off, WAVE);
  return v;
}

// --------------------------------------------------------------------------
// forward: pooled[n,c] = sum_hw x[n,hw,c] / HW ; logits = pooled @ w^T + b
// --------------------------------------------------------------------------
// grid N, block FT_BLOCK.  Pool: the C/8 16-byte chunks of a pixel go to
// consecutive threads, G = 256 / (C/8) thread groups stride over the pixels;
// the G partial rows (G*C <= 2048 floats) are summed per channel in group
// order.  FC: wave w takes classes w, w+4, ...; lane l takes channel chunks
// l and l+64.
template <typename TX, typename TW>
__global__ void __launch_bounds__(FT_BLOCK)
head_fwd_k(const TX* __restrict__ x, const TW* __restrict__ w,
           const void* __restrict__ bias, int bias_bf16,
           float* __restrict__ logits, float* __restrict__ pooled,
           int C, int HW, int K) {
  __shared__ __attribute__((aligned(16))) float part[FT_BLOCK * 8];
  __shared__ __attribute__((aligned(16))) float pl[HEAD_MAXC];
  const int tid = threadIdx.x;
  const long n = blockIdx.x;
  const int nchunk = C >> 3;            // 1..128
  const int G = FT_BLOCK / nchunk;      // 2..256
  if (tid < G * nchunk) {
    const int ch = tid % nchunk, g = tid / nchunk;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const TX* xp = x + n * (long)HW * C + ch * 8;
    for (int p = g; p < HW; p += G) {
      float v[8];
      head_ld8(xp + (long)p * C, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += v[j];
    }
    head_st8(part + g * C + ch * 8, acc);
  }
  __syncthreads();
  const int Gu = G < HW ? G : HW;       // groups that saw a pixel
  for (int c = tid; c < C; c += FT_BLOCK) {
    float s = 0.f;
    for (int g = 0; g < Gu; ++g) s += part[g * C + c];
    s = s / (float)HW;
    pl[c] = s;
    pooled[n * C + c] = s;
  }
  __syncthreads();
  const int lane = tid & (WAVE - 1), wid = tid / WAVE;
  for (int k = wid; k < K; k += FT_BLOCK / WAVE) {
    float s = 0.f;
    const TW* wp = w + (long)k * C;
    for (int ch = lane; ch < nchunk; ch += WAVE) {
      float wv[8];
      head_ld8(wp + ch * 8, wv);
      const float4 a = reinterpret_cast<const float4*>(pl + ch * 8)[0];
      const float4 b = reinterpret_cast<const float4*>(pl + ch * 8)[1];
      s = fmaf(a.x, wv[0], s); s = fmaf(a.y, wv[1], s);
      s = fmaf(a.z, wv[2], s); s = fmaf(a.w, wv[3], s);
      s = fmaf(b.x, wv[4], s); s = fmaf(b.y, wv[5], s);
      s = fmaf(b.z, wv[6], s); s = fmaf(b.w, wv[7], s);
    }
    s = wave_sum(s);
    if (lane == 0) {
      if (bias) s += head_ld1(bias, k, bias_bf16);
      logits[n * K + k] = s;
    }
  }
}

// --------------------------------------------------------------------------
// backward, input gradient
// --------------------------------------------------------------------------
// grid N, block FT_BLOCK.  dx[n,hw,c] = (sum_k dl[n,k] w[k,c]) / HW.
template <typename TX, typename TW>
__global__ void __launch_bounds__(FT_BLOCK)
head_dx_k(const float* __restrict__ dl, const TW* __restrict__ w,
          TX* __restrict__ dx, int C, int HW, int K) {
  __shared__ float dls[HEAD_MAXK];
  __shared__ __attribute__((aligned(16))) float g[HEAD_MAXC];
  const int tid = threadIdx.x;
  const long n = blockIdx.x;
  for (int k = tid; k < K; k += FT_BLOCK) dls[k] = dl[n * K + k];
  __syncthreads();
  for (int c = tid; c < C; c += FT_BLOCK) {
    float s = 0.f;
    for (int k = 0; k < K; ++k)
      s = fmaf(dls[k], head_ld1(w, (long)k * C + c, sizeof(TW) == 2), s);
    g[c] = s / (float)HW;
  }
  __syncthreads();
  const int nchunk = C >> 3;
  const int total = HW * nchunk;
  TX* dp = dx + n * (long)HW * C;
  for (int i = tid; i < total; i += FT_BLOCK) {
    const int ch = i % nchunk;
    float v[8];
    const float4 a = reinterpret_cast<const float4*>(g + ch * 8)[0];
    const float4 b = reinterpret_cast<const float4*>(g + ch * 8)[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    head_st8(dp + (long)i * 8, v);
  }
}

// --------------------------------------------------------------------------
// backward, weight and bias gradients
// --------------------------------------------------------------------------
// grid (ceil(C/64), K), block FT_BLOCK.  Lane l owns channel c = 64*bx + l of
// class k; wave s sums the samples [s*Ns, (s+1)*Ns), Ns = ceil(N/4), in
// order; the 4 partials are added ((p0+p1)+p2)+p3.  dl[n,k] is a wave-uniform
// load.  The bx == 0 workgroups also produce db[k].
__global__ void __launch_bounds__(FT_BLOCK)
head_dwdb_k(const float* __restrict__ dl, const float* __restrict__ pooled,
            void* __restrict__ dw, int dw_bf16, void* __restrict__ db,
            int db_bf16, int N, int C, int K) {
  __shared__ float pw[FT_BLOCK / WAVE][WAVE];
  __shared__ float pb[FT_BLOCK / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  const int c = blockIdx.x * WAVE + lane;
  const int k = blockIdx.y;
  const int Ns = (N + FT_BLOCK / WAVE - 1) / (FT_BLOCK / WAVE);
  const int n0 = wid * Ns;
  const int n1 = (n0 + Ns) < N ? (n0 + Ns) : N;
  const bool live = c < C;
  float s = 0.f, sb = 0.f;
#pragma unroll 4
  for (int n = n0; n < n1; ++n) {
    const float d = dl[(long)n * K + k];
    const float p = live ? pooled[(long)n * C + c] : 0.f;
    s = fmaf(d, p, s);
    sb += d;
  }
  pw[wid][lane] = s;
  if (lane == 0) pb[wid] = sb;
  __syncthreads();
  if (wid == 0) {
    if (live)
      head_st1(dw, (long)k * C + c, dw_bf16,
               ((pw[0][lane] + pw[1][lane]) + pw[2][lane]) + pw[3][lane]);
    if (db && blockIdx.x == 0 && lane == 0)
      head_st1(db, k, db_bf16, ((pb[0] + pb[1]) + pb[2]) + pb[3]);
  }
}

// --------------------------------------------------------------------------
// cross-entropy + top-1 / top-5 accumulator
// --------------------------------------------------------------------------
// grid 1, block HEAD_CE_BLOCK (16 waves).  Wave s takes samples s, s+16, ...;
// per sample the lanes stride over the K logits twice (max; then sum of exp
// and the two rank counts), re-reading the <= 4 KB row from cache.
//   loss = log(sum_j exp(z_j - m)) - (z_t - m)
//   rank = #{j : z_j > z_t} + #{j < t : z_j == z_t};  top-k iff rank < k
// A target outside [0, K) (ignore_index included) skips the sample before
// anything is indexed with it.  Lane 0 of each wave keeps its samples' sums
// (loss in fp64), thread 0 adds the 16 wave sums in wave order into acc.
template <typename TL>
__global__ void __launch_bounds__(HEAD_CE_BLOCK)
ce_topk_k(const TL* __restrict__ z, const long* __restrict__ target,
          double* __restrict__ acc, int N, int K) {
  constexpr int NW = HEAD_CE_BLOCK / WAVE;
  __shared__ double s_loss[NW];
  __shared__ int s_cnt[NW][3];
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  double loss_sum = 0.0;
  int top1 = 0, top5 = 0, cnt = 0;
  for (int n = wid; n < N; n += NW) {
    const long t = target[n];
    if (t < 0 || t >= K) continue;       // wave-uniform
    const TL* zr = z + (long)n * K;
    float m = -INFINITY;
    for (int j = lane; j < K; j += WAVE)
      m = fmaxf(m, head_ld1(zr, j, sizeof(TL) == 2));
    m = wave_max(m);
    m = __shfl(m, 0, WAVE);
    const float zt = head_ld1(zr, t, sizeof(TL) == 2);
    float se = 0.f;
    int rank = 0;
    for (int j = lane; j < K; j += WAVE) {
      const float v = head_ld1(zr, j, sizeof(TL) == 2);
      se += expf(v - m);
      rank += (v > zt) || (v == zt && j < t);
    }
    se = wave_sum(se);
    rank = head_wave_sum_i(rank);
    if (lane == 0) {
      loss_sum += (double)(logf(se) - (zt - m));
      top1 += rank < 1;
      top5 += rank < 5;
      cnt += 1;
    }
  }
  if (lane == 0) {
    s_loss[wid] = loss_sum;
    s_cnt[wid][0] = top1; s_cnt[wid][1] = top5; s_cnt[wid][2] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double l = 0.0;
    int a = 0, b = 0, c = 0;
    for (int i = 0; i < NW; ++i) {
      l += s_loss[i];
      a += s_cnt[i][0]; b += s_cnt[i][1]; c += s_cnt[i][2];
    }
    acc[0] += l;
    acc[1] += (double)a;
    acc[2] += (double)b;
    acc[3] += (double)c;
  }
}
