// fedtorch_amd CDNA4 kernel pack (gfx950 / MI355X) — torch extension.
//
// Arena hot paths of the federated engine, each ONE kernel launch over the
// flat parameter arena (design rationale: SURVEY.md §2.3 — the reference
// fedtorch runs every one of these as P~65 per-parameter torch ops).
// Reference semantics cited per op in fedtorch_amd/ops/__init__.py.
//
// Build: hipcc --offload-arch=gfx950 via torch.utils.cpp_extension (see
// setup.py). No CUDA path, no hipify, no multi-backend dispatch.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include "common.h"
#include "batchnorm.h"
#include "stemconv.h"
#include "convwrw.h"
#include "convwrw2.h"
#include "convfwd.h"
#include "convs2bwd.h"
#include "head.h"
#include "gru.h"
#include "linearround.h"
#include "mlpround.h"
#include "cnnround.h"

#define CHK(x) TORCH_CHECK(x.is_cuda() && x.is_contiguous(), #x " must be contiguous on GPU")
#define STREAM at::hip::getCurrentHIPStream().stream()

// grid caps overridable via env for on-box tuning sweeps (read once)
static inline int ft_env_int(const char* k, int d) {
  const char* v = getenv(k);
  return v ? atoi(v) : d;
}


// ==========================================================================
// fused dual-mode SGD step (+ per-algorithm corrections)
// ==========================================================================
enum {
  F_DELTA = 1, F_CTRL = 2, F_PROX = 4, F_WD = 8,
  F_IN = 16, F_OUT = 32, F_NESTEROV = 64, F_FIRST_IN = 128,
  F_FIRST_OUT = 256, F_HALF = 512
};

__global__ void fused_sgd_kernel(
    float* __restrict__ p, const float* __restrict__ g,
    float* __restrict__ bin, float* __restrict__ bout,
    const float* __restrict__ delta, const float* __restrict__ cs,
    const float* __restrict__ cc, const float* __restrict__ server,
    __hip_bfloat16* __restrict__ half_p,
    long n4, long wd_n4, float wd, float m_in, float m_out,
    float omd_in, float omd_out, float step_scale, float prox_mu,
    int flags) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += stride) {
    float4 dv = reinterpret_cast<const float4*>(g)[i];
    float4 pv = reinterpret_cast<float4*>(p)[i];
    float* d = reinterpret_cast<float*>(&dv);
    float* pp = reinterpret_cast<float*>(&pv);
    if (flags & F_DELTA) {
      float4 t = reinterpret_cast<const float4*>(delta)[i];
      const float* tt = reinterpret_cast<const float*>(&t);
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] -= tt[j];
    }
    if (flags & F_CTRL) {
      float4 a = reinterpret_cast<const float4*>(cs)[i];
      float4 b = reinterpret_cast<const float4*>(cc)[i];
      const float* aa = reinterpret_cast<const float*>(&a);
      const float* bb = reinterpret_cast<const float*>(&b);
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] += aa[j] - bb[j];
    }
    if (flags & F_PROX) {
      float4 s = reinterpret_cast<const float4*>(server)[i];
      const float* ss = reinterpret_cast<const float*>(&s);
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] += prox_mu * (pp[j] - ss[j]);
    }
    if ((flags & F_WD) && i < wd_n4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] = fmaf(wd, pp[j], d[j]);
    }
    if (flags & F_IN) {
      float4 bv;
      if (flags & F_FIRST_IN) {
        bv = dv;
      } else {
        bv = reinterpret_cast<const float4*>(bin)[i];
        float* b = reinterpret_cast<float*>(&bv);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = fmaf(m_in, b[j], omd_in * d[j]);
      }
      reinterpret_cast<float4*>(bin)[i] = bv;
      const float* b = reinterpret_cast<const float*>(&bv);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        d[j] = (flags & F_NESTEROV) ? fmaf(m_in, b[j], d[j]) : b[j];
    }
    if (flags & F_OUT) {
      float4 bv;
      if (flags & F_FIRST_OUT) {
        bv = dv;
      } else {
        bv = reinterpret_cast<const float4*>(bout)[i];
        float* b = reinterpret_cast<float*>(&bv);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = fmaf(m_out, b[j], omd_out * d[j]);
      }
      reinterpret_cast<float4*>(bout)[i] = bv;
      const float* b = reinterpret_cast<const float*>(&bv);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        d[j] = (flags & F_NESTEROV) ? fmaf(m_out, b[j], d[j]) : b[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) pp[j] = fmaf(-step_scale, d[j], pp[j]);
    reinterpret_cast<float4*>(p)[i] = pv;
    if (flags & F_HALF) {  // refresh the bf16 compute copy in the same pass
      struct alignas(8) H4 { __hip_bfloat16 d[4]; };
      H4 hv;
#pragma unroll
      for (int j = 0; j < 4; ++j) hv.d[j] = __float2bfloat16(pp[j]);
      reinterpret_cast<H4*>(half_p)[i] = hv;
    }
  }
}

void fused_sgd_step(torch::Tensor p, torch::Tensor g, torch::Tensor in_buf,
                    torch::Tensor out_buf, torch::Tensor delta,
                    torch::Tensor ctrl_server, torch::Tensor ctrl_client,
                    torch::Tensor server, double lr, double scale, double wd,
                    double m_in, double m_out, double damp, bool nesterov,
                    bool apply_lr, bool apply_in, bool apply_out,
                    bool first_in, bool first_out, double prox_mu,
                    long wd_numel, torch::Tensor half_p) {
  CHK(p); CHK(g);
  TORCH_CHECK(p.numel() % 4 == 0, "arena numel must be float4-aligned");
  long n4 = p.numel() / 4;
  int flags = 0;
  if (delta.numel()) flags |= F_DELTA;
  if (ctrl_server.numel()) flags |= F_CTRL;
  if (prox_mu != 0.0 && server.numel()) flags |= F_PROX;
  if (wd != 0.0 && apply_lr) flags |= F_WD;
  if (apply_in && m_in != 0.0) flags |= F_IN;
  if (apply_out && m_out != 0.0) flags |= F_OUT;
  if (nesterov) flags |= F_NESTEROV;
  if (first_in) flags |= F_FIRST_IN;
  if (first_out) flags |= F_FIRST_OUT;
  if (half_p.numel()) flags |= F_HALF;
  hipLaunchKernelGGL(fused_sgd_kernel, dim3(ft_grid(n4)), dim3(FT_BLOCK), 0,
                     STREAM, p.data_ptr<float>(), g.data_ptr<float>(),
                     (flags & F_IN) ? in_buf.data_ptr<float>() : nullptr,
                     (flags & F_OUT) ? out_buf.data_ptr<float>() : nullptr,
                     (flags & F_DELTA) ? delta.data_ptr<float>() : nullptr,
                     (flags & F_CTRL) ? ctrl_server.data_ptr<float>() : nullptr,
                     (flags & F_CTRL) ? ctrl_client.data_ptr<float>() : nullptr,
                     (flags & F_PROX) ? server.data_ptr<float>() : nullptr,
                     (flags & F_HALF) ? reinterpret_cast<__hip_bfloat16*>(
                                            half_p.data_ptr())
                                      : nullptr,
                     n4, wd_numel / 4, (float)wd, (float)m_in, (float)m_out,
                     (float)(1.0 - damp), (float)(1.0 - damp),
                     (float)(apply_lr ? lr : scale), (float)prox_mu, flags);
}

// ==========================================================================
// elementwise arena ops
// ==========================================================================
__global__ void wdr_kernel(const float* __restrict__ s, float* __restrict__ c,
                           float* __restrict__ out, float w, long n4,
                           int restore) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += stride) {
    float4 sv = reinterpret_cast<const float4*>(s)[i];
    float4 cv = reinterpret_cast<float4*>(c)[i];
    float4 ov;
    float* o = reinterpret_cast<float*>(&ov);
    const float* ss = reinterpret_cast<const float*>(&sv);
    const float* ccp = reinterpret_cast<const float*>(&cv);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (ss[j] - ccp[j]) * w;
    reinterpret_cast<float4*>(out)[i] = ov;
    if (restore) reinterpret_cast<float4*>(c)[i] = sv;
  }
}

void weighted_diff_restore(torch::Tensor s, torch::Tensor c, torch::Tensor out,
                           double w) {
  CHK(s); CHK(c); CHK(out);
  long n4 = s.numel() / 4;
  hipLaunchKernelGGL(wdr_kernel, dim3(ft_grid(n4)), dim3(FT_BLOCK), 0, STREAM,
                     s.data_ptr<float>(), c.data_ptr<float>(),
                     out.data_ptr<float>(), (float)w, n4, 1);
}

void scaled_diff(torch::Tensor a, torch::Tensor b, torch::Tensor out,
                 double w) {
  CHK(a); CHK(b); CHK(out);
  long n4 = a.numel() / 4;
  hipLaunchKernelGGL(wdr_kernel, dim3(ft_grid(n4)), dim3(FT_BLOCK), 0, STREAM,
                     a.data_ptr<float>(), b.data_ptr<float>(),
                     out.data_ptr<float>(), (float)w, n4, 0);
}

// y = b*y + a*x ; ef: mem += g*invw - d ; delta += (s-agg-c)*coef ;
// ctrl_new = cc - cs + (s-c)*coef ; blend out = alpha*a+(1-alpha)*b —
// all are 2-4-operand streaming FMAs; one generic kernel each.
__global__ void axpby_kernel(float* __restrict__ y, const float* __restrict__ x,
                             float a, float b, long n4) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += stride) {
    float4 yv = reinterpret_cast<float4*>(y)[i];
    float4 xv = reinterpret_cast<const float4*>(x)[i];
    float* yy = reinterpret_cast<float*>(&yv);
    const float* xx = reinterpret_cast<const float*>(&xv);
#pragma unroll
    for (int j = 0; j < 4; ++j) yy[j] = fmaf(b, yy[j], a * xx[j]);
    reinterpret_cast<float4*>(y)[i] = yv;
  }
}

void axpby(torch::Tensor y, torch::Tensor x, double a, double b) {
  CHK(y); CHK(x);
  long n4 = y.numel() / 4;
  hipLaunchKernelGGL(axpby_kernel, dim3(ft_grid(n4)), dim3(FT_BLOCK), 0,
                     STREAM, y.data_ptr<float>(), x.data_ptr<float>(),
                     (float)a, (float)b, n4);
}

__global__ void ef_kernel(float* __restrict__ mem, const float* __restrict__ g,
                          const float* __restrict__ d, float invw, long n4) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += stride) {
    float4 mv = reinterpret_cast<float4*>(mem)[i];
    float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 dv = reinterpret_cast<const float4*>(d)[i];
    float* m = reinterpret_cast<float*>(&mv);
    const float* gg = reinterpret_cast<const float*>(&gv);
    const float* dd = reinterpret_cast<const float*>(&dv);
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = fmaf(invw, gg[j], m[j]) - dd[j];
    reinterpret_cast<float4*>(mem)[i] = mv;
  }
}

void error_feedback_update(torch::Tensor mem, torch::Tensor g, torch::Tensor d,
                           double invw) {
  CHK(mem); CHK(g); CHK(d);
  long n4 = mem.numel() / 4;
  hipLaunchKernelGGL(ef_kernel, dim3(ft_grid(n4)), dim3(FT_BLOCK), 0, STREAM,
                     mem.data_ptr<float>(), g.data_ptr<float>(),
                     d.data_ptr<float>(), (float)invw, n4);
}

__global__ void delta_kernel(float* __restrict__ delta,
                             const float* __restrict__ s,
                             const float* __restrict__ agg,
                             const float* __restrict__ c, float coef,
                             long n4) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += stride) {
    float4 dv = reinterpret_cast<float4*>(delta)[i];
    float4 sv = reinterpret_cast<const float4*>(s)[i];
    float4 av = reinterpret_cast<const float4*>(agg)[i];
    float4 cv = reinterpret_cast<const float4*>(c)[i];
    float* d = reinterpret_cast<float*>(&dv);
    const float* ss = reinterpret_cast<const float*>(&sv);
    const float* aa = reinterpret_cast<const float*>(&av);
    const float* cc2 = reinterpret_cast<const float*>(&cv);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      d[j] = fmaf(coef, ss[j] - aa[j] - cc2[j], d[j]);
    reinterpret_cast<float4*>(delta)[i] = dv;
  }
}

void delta_update(torch::Tensor delta, torch::Tensor s, torch::Tensor agg,
                  torch::Tensor c, double coef) {
  CHK(delta);
  long n4 = delta.numel() / 4;
  hipLaunchKernelGGL(delta_kernel, dim3(ft_grid(n4)), dim3(FT_BLOCK), 0,
                     STREAM, delta.data_ptr<float>(), s.data_ptr<float>(),
                     agg.data_ptr<float>(), c.data_ptr<float>(), (float)coef,
                     n4);
}

__global__ void ctrl_kernel(float* __restrict__ out,
                            const float* __restrict__ cc,
                            const float* __restrict__ cs,
                            const float* __restrict__ s,
                            const float* __restrict__ c, float coef, long n4) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += stride) {
    float4 a = reinterpret_cast<const float4*>(cc)[i];
    float4 b = reinterpret_cast<const float4*>(cs)[i];
    float4 sv = reinterpret_cast<const float4*>(s)[i];
    float4 cv = reinterpret_cast<const float4*>(c)[i];
    float4 ov;
    float* o = reinterpret_cast<float*>(&ov);
    const float* aa = reinterpret_cast<const float*>(&a);
    const float* bb = reinterpret_cast<const float*>(&b);
    const float* ss = reinterpret_cast<const float*>(&sv);
    const float* cc3 = reinterpret_cast<const float*>(&cv);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      o[j] = aa[j] - bb[j] + coef * (ss[j] - cc3[j]);
    reinterpret_cast<float4*>(out)[i] = ov;
  }
}

void scaffold_control_update(torch::Tensor out, torch::Tensor cc,
                             torch::Tensor cs, torch::Tensor s,
                             torch::Tensor c, double coef) {
  CHK(out);
  long n4 = out.numel() / 4;
  hipLaunchKernelGGL(ctrl_kernel, dim3(ft_grid(n4)), dim3(FT_BLOCK), 0,
                     STREAM, out.data_ptr<float>(), cc.data_ptr<float>(),
                     cs.data_ptr<float>(), s.data_ptr<float>(),
                     c.data_ptr<float>(), (float)coef, n4);
}

__global__ void blend_kernel(float* __restrict__ out,
                             const float* __restrict__ a,
                             const float* __restrict__ b, float alpha,
                             long n4) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += stride) {
    float4 av = reinterpret_cast<const float4*>(a)[i];
    float4 bv = reinterpret_cast<const float4*>(b)[i];
    float4 ov;
    float* o = reinterpret_cast<float*>(&ov);
    const float* aa = reinterpret_cast<const float*>(&av);
    const float* bb = reinterpret_cast<const float*>(&bv);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      o[j] = fmaf(alpha, aa[j] - bb[j], bb[j]);
    reinterpret_cast<float4*>(out)[i] = ov;
  }
}

void blend(torch::Tensor out, torch::Tensor a, torch::Tensor b, double alpha) {
  CHK(out);
  long n4 = out.numel() / 4;
  hipLaunchKernelGGL(blend_kernel, dim3(ft_grid(n4)), dim3(FT_BLOCK), 0,
                     STREAM, out.data_ptr<float>(), a.data_ptr<float>(),
                     b.data_ptr<float>(), (float)alpha, n4);
}

// APFL alpha gradient: dot(p_f - l_f, alpha*p_g + (1-alpha)*l_g) ----------
__global__ void alpha_grad_kernel(const float* __restrict__ lf,
                                  const float* __restrict__ pf,
                                  const float* __restrict__ lg,
                                  const float* __restrict__ pg, float alpha,
                                  long n, float* __restrict__ out) {
  const long stride = (long)gridDim.x * blockDim.x;
  float acc = 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += stride) {
    float dif = pf[i] - lf[i];
    float g = fmaf(alpha, pg[i] - lg[i], lg[i]);
    acc = fmaf(dif, g, acc);
  }
  acc = block_reduce<0>(acc);
  if (threadIdx.x == 0) atomicAdd(out, acc);
}

double alpha_grad(torch::Tensor lf, torch::Tensor pf, torch::Tensor lg,
                  torch::Tensor pg, double alpha) {
  CHK(lf);
  auto out = torch::zeros({1}, lf.options());
  long n = lf.numel();
  hipLaunchKernelGGL(alpha_grad_kernel, dim3(ft_grid(n)), dim3(FT_BLOCK), 0,
                     STREAM, lf.data_ptr<float>(), pf.data_ptr<float>(),
                     lg.data_ptr<float>(), pg.data_ptr<float>(), (float)alpha,
                     n, out.data_ptr<float>());
  return out.item<float>();
}

// ==========================================================================
// adaptive quantization (reference flow_utils.py:169-212 semantics)
// ==========================================================================
__global__ void minmaxsum_kernel(const float* __restrict__ x, long n,
                                 float* __restrict__ scratch) {
  // scratch layout: [gridDim] mins | [gridDim] maxs | [gridDim] sums
  const long stride = (long)gridDim.x * blockDim.x;
  float mn = 3.4e38f, mx = -3.4e38f, sm = 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += stride) {
    float v = x[i];
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
    sm += v;
  }
  float bmn = block_reduce<1>(mn);
  __syncthreads();
  float bmx = block_reduce<2>(mx);
  __syncthreads();
  float bsm = block_reduce<0>(sm);
  if (threadIdx.x == 0) {
    scratch[blockIdx.x] = bmn;
    scratch[gridDim.x + blockIdx.x] = bmx;
    scratch[2 * gridDim.x + blockIdx.x] = bsm;
  }
}

__global__ void quant_info_kernel(const float* __restrict__ scratch,
                                  int nblocks, long n, float qmin, float qmax,
                                  float* __restrict__ info) {
  // single block finalize: info = [scale, zero_point, mean]
  float mn = 3.4e38f, mx = -3.4e38f, sm = 0.f;
  for (int i = threadIdx.x; i < nblocks; i += blockDim.x) {
    mn = fminf(mn, scratch[i]);
    mx = fmaxf(mx, scratch[nblocks + i]);
    sm += scratch[2 * nblocks + i];
  }
  mn = block_reduce<1>(mn);
  __syncthreads();
  mx = block_reduce<2>(mx);
  __syncthreads();
  sm = block_reduce<0>(sm);
  if (threadIdx.x == 0) {
    float mean = sm / (float)n;
    float scale = (mx - mn) / (qmax - qmin);
    if (scale == 0.f) scale = 0.001f;
    float izp = qmin - (mn - mean) / scale;
    // reference: clamp then python int() = truncation toward zero
    float zp = izp < qmin ? qmin : (izp > qmax ? qmax : truncf(izp));
    info[0] = scale;
    info[1] = zp;
    info[2] = mean;
  }
}

template <typename QT>
__global__ void quant_encode_kernel(const float* __restrict__ x, long n,
                                    const float* __restrict__ info,
                                    float qmin, float qmax,
                                    QT* __restrict__ q) {
  const float scale = info[0], zp = info[1], mean = info[2];
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += stride) {
    float v = zp + (x[i] - mean) / scale;
    v = fminf(fmaxf(v, qmin), qmax);
    q[i] = (QT)rintf(v);  // round-half-even, matches torch round_()
  }
}

std::vector<torch::Tensor> quantize_adaptive(torch::Tensor x, long num_bits) {
  CHK(x);
  long n = x.numel();
  float qmin = -exp2f((float)(num_bits - 1));
  float qmax = exp2f((float)(num_bits - 1)) - 1.f;
  int blocks = ft_grid(n);
  auto scratch = torch::empty({3 * blocks}, x.options());
  auto info = torch::empty({3}, x.options());
  hipLaunchKernelGGL(minmaxsum_kernel, dim3(blocks), dim3(FT_BLOCK), 0,
                     STREAM, x.data_ptr<float>(), n,
                     scratch.data_ptr<float>());
  hipLaunchKernelGGL(quant_info_kernel, dim3(1), dim3(FT_BLOCK), 0, STREAM,
                     scratch.data_ptr<float>(), blocks, n, qmin, qmax,
                     info.data_ptr<float>());
  torch::Tensor q;
  if (num_bits == 8) {
    q = torch::empty({n}, x.options().dtype(torch::kChar));
    hipLaunchKernelGGL(quant_encode_kernel<int8_t>, dim3(ft_grid(n)),
                       dim3(FT_BLOCK), 0, STREAM, x.data_ptr<float>(), n,
                       info.data_ptr<float>(), qmin, qmax,
                       q.data_ptr<int8_t>());
  } else {
    q = torch::empty({n}, x.options().dtype(torch::kShort));
    hipLaunchKernelGGL(quant_encode_kernel<int16_t>, dim3(ft_grid(n)),
                       dim3(FT_BLOCK), 0, STREAM, x.data_ptr<float>(), n,
                       info.data_ptr<float>(), qmin, qmax,
                       q.data_ptr<int16_t>());
  }
  return {q, info};
}

template <typename QT>
__global__ void dequant_kernel(const QT* __restrict__ q, long n,
                               const float* __restrict__ info,
                               float* __restrict__ out) {
  const float scale = info[0], zp = info[1], mean = info[2];
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += stride)
    out[i] = fmaf(scale, (float)q[i] - zp, mean);
}

torch::Tensor dequantize(torch::Tensor q, torch::Tensor info) {
  CHK(q);
  long n = q.numel();
  auto out = torch::empty({n}, info.options());
  if (q.scalar_type() == torch::kChar)
    hipLaunchKernelGGL(dequant_kernel<int8_t>, dim3(ft_grid(n)),
                       dim3(FT_BLOCK), 0, STREAM, q.data_ptr<int8_t>(), n,
                       info.data_ptr<float>(), out.data_ptr<float>());
  else
    hipLaunchKernelGGL(dequant_kernel<int16_t>, dim3(ft_grid(n)),
                       dim3(FT_BLOCK), 0, STREAM, q.data_ptr<int16_t>(), n,
                       info.data_ptr<float>(), out.data_ptr<float>());
  return out;
}

template <typename QT>
__global__ void dequant_acc_kernel(const QT* __restrict__ qs, long k, long n,
                                   const float* __restrict__ infos,
                                   float* __restrict__ out) {
  // qs: [k, n]; infos: [k, 3]; out[i] = sum_j scale_j*(q_ji - zp_j) + mean_j
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += stride) {
    float acc = 0.f;
    for (long j = 0; j < k; ++j) {
      const float scale = infos[3 * j], zp = infos[3 * j + 1],
                  mean = infos[3 * j + 2];
      acc += fmaf(scale, (float)qs[j * n + i] - zp, mean);
    }
    out[i] = acc;
  }
}

void dequant_accumulate(torch::Tensor qs, torch::Tensor infos,
                        torch::Tensor out) {
  CHK(qs); CHK(out);
  long k = qs.size(0), n = qs.size(1);
  if (qs.scalar_type() == torch::kChar)
    hipLaunchKernelGGL(dequant_acc_kernel<int8_t>, dim3(ft_grid(n)),
                       dim3(FT_BLOCK), 0, STREAM, qs.data_ptr<int8_t>(), k, n,
                       infos.data_ptr<float>(), out.data_ptr<float>());
  else
    hipLaunchKernelGGL(dequant_acc_kernel<int16_t>, dim3(ft_grid(n)),
                       dim3(FT_BLOCK), 0, STREAM, qs.data_ptr<int16_t>(), k,
                       n, infos.data_ptr<float>(), out.data_ptr<float>());
}

// ==========================================================================
// top-k |x| selection: 4-pass device-side radix select + compaction
// (the reference's `x.abs().topk(k)` per tensor, `flow_utils.py:218-230`).
// ==========================================================================
__global__ void radix_hist_kernel(const float* __restrict__ x, long n,
                                  const unsigned int* __restrict__ state,
                                  int shift, unsigned int* __restrict__ hist) {
  // state = {prefix, k_remaining}; count keys matching prefix above `shift`
  __shared__ unsigned int lhist[256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) lhist[i] = 0;
  __syncthreads();
  const unsigned int prefix = state[0];
  const unsigned int pmask = (shift == 24) ? 0u
      : (0xFFFFFFFFu << (shift + 8));
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += stride) {
    unsigned int key = abs_key(x[i]);
    if ((key & pmask) == (prefix & pmask))
      atomicAdd(&lhist[(key >> shift) & 0xFF], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 256; i += blockDim.x)
    if (lhist[i]) atomicAdd(&hist[i], lhist[i]);
}

__global__ void radix_pick_kernel(unsigned int* __restrict__ hist, int shift,
                                  unsigned int* __restrict__ state) {
  // ONE thread walks the 256 buckets from the top: find the bucket where the
  // k-th largest key lands, fold it into the prefix, update k_remaining.
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  unsigned int k = state[1];
  unsigned int cum = 0;
  int b = 255;
  for (; b >= 0; --b) {
    unsigned int c = hist[b];
    if (cum + c >= k) break;
    cum += c;
  }
  if (b < 0) b = 0;
  state[0] |= ((unsigned int)b) << shift;
  state[1] = k - cum;
  for (int i = 0; i < 256; ++i) hist[i] = 0;  // reset for next pass
}

__global__ void topk_compact_kernel(const float* __restrict__ x, long n,
                                    const unsigned int* __restrict__ state,
                                    long k, float* __restrict__ v,
                                    int* __restrict__ idx,
                                    unsigned int* __restrict__ counters) {
  // counters[0]: slots for keys > threshold; counters[1]: ties (== thr).
  const unsigned int thr = state[0];
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += stride) {
    unsigned int key = abs_key(x[i]);
    if (key > thr) {
      unsigned int slot = atomicAdd(&counters[0], 1u);
      v[slot] = x[i];
      idx[slot] = (int)i;
    }
  }
}

__global__ void topk_ties_kernel(const float* __restrict__ x, long n,
                                 const unsigned int* __restrict__ state,
                                 long k, float* __restrict__ v,
                                 int* __restrict__ idx,
                                 unsigned int* __restrict__ counters) {
  const unsigned int thr = state[0];
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n;
       i += stride) {
    unsigned int key = abs_key(x[i]);
    if (key == thr) {
      unsigned int slot = atomicAdd(&counters[0], 1u);
      if (slot < (unsigned int)k) {
        v[slot] = x[i];
        idx[slot] = (int)i;
      }
    }
  }
}

std::vector<torch::Tensor> topk_compress(torch::Tensor x, long k) {
  CHK(x);
  long n = x.numel();
  TORCH_CHECK(k > 0 && k <= n, "invalid k");
  auto u32 = x.options().dtype(torch::kUInt32);
  auto state = torch::tensor({(int64_t)0, (int64_t)k},
                             torch::dtype(torch::kUInt32))
                   .to(x.device(), /*non_blocking=*/true);
  auto hist = torch::zeros({256}, u32);
  auto v = torch::empty({k}, x.options());
  auto idx = torch::empty({k}, x.options().dtype(torch::kInt32));
  auto counters = torch::zeros({2}, u32);
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(radix_hist_kernel, dim3(ft_grid(n)), dim3(FT_BLOCK), 0,
                       STREAM, x.data_ptr<float>(), n,
                       state.data_ptr<unsigned int>(), shift,
                       hist.data_ptr<unsigned int>());
    hipLaunchKernelGGL(radix_pick_kernel, dim3(1), dim3(1), 0, STREAM,
                       hist.data_ptr<unsigned int>(), shift,
                       state.data_ptr<unsigned int>());
  }
  hipLaunchKernelGGL(topk_compact_kernel, dim3(ft_grid(n)), dim3(FT_BLOCK), 0,
                     STREAM, x.data_ptr<float>(), n,
                     state.data_ptr<unsigned int>(), k, v.data_ptr<float>(),
                     idx.data_ptr<int>(), counters.data_ptr<unsigned int>());
  hipLaunchKernelGGL(topk_ties_kernel, dim3(ft_grid(n)), dim3(FT_BLOCK), 0,
                     STREAM, x.data_ptr<float>(), n,
                     state.data_ptr<unsigned int>(), k, v.data_ptr<float>(),
                     idx.data_ptr<int>(), counters.data_ptr<unsigned int>());
  return {v, idx};
}

// batched virtual-client aggregation: ONE pass over the [C, N] replica
// arena — out[i] = sum_c w[c] * (server[i] - replicas[c][i]).
// (packed mode, fedtorch_amd/parallel/multiclient.py; replaces C separate
// ==========================================================================
// FedAdam server normalizer (reference `federated/fedavg.py:81-85`, after
// arXiv:2003.00295): per-parameter-tensor v_p = beta*v_p + (1-beta)*||g_p||,
// g_p /= (sqrt(v_p)+tau).  ONE kernel, one workgroup per tensor segment,
// v resident on-device — the reference (and round-1 repo) ran a Python
// loop with a float(torch.norm(g)) host sync per tensor per sync round.
__global__ void fedadam_norm_kernel(float* __restrict__ g,
                                    const long* __restrict__ seg,
                                    float* __restrict__ v,
                                    float beta, float tau) {
  const int p = blockIdx.x;
  const long s = seg[2 * p], e = seg[2 * p + 1];
  __shared__ float red[FT_BLOCK / 64];
  __shared__ float inv_s;
  float acc = 0.f;
  for (long i = s + threadIdx.x; i < e; i += blockDim.x) {
    const float x = g[i];
    acc += x * x;
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < FT_BLOCK / 64; ++i) t += red[i];
    const float nv = beta * v[p] + (1.f - beta) * sqrtf(t);
    v[p] = nv;
    inv_s = 1.f / (sqrtf(nv) + tau);
  }
  __syncthreads();
  const float inv = inv_s;
  for (long i = s + threadIdx.x; i < e; i += blockDim.x) g[i] *= inv;
}

void fedadam_normalize(torch::Tensor g, torch::Tensor seg, torch::Tensor v,
                       double beta, double tau) {
  CHK(g); CHK(seg); CHK(v);
  TORCH_CHECK(seg.scalar_type() == torch::kLong && seg.numel() == 2 * v.numel(),
              "seg must be int64 [P,2]");
  hipLaunchKernelGGL(fedadam_norm_kernel, dim3((int)v.numel()),
                     dim3(FT_BLOCK), 0, STREAM, g.data_ptr<float>(),
                     seg.data_ptr<long>(), v.data_ptr<float>(),
                     (float)beta, (float)tau);
}

// diff+add launches.)
__global__ void multi_diff_acc_kernel(const float* __restrict__ server,
                                      const float* __restrict__ replicas,
                                      const float* __restrict__ w, long C,
                                      long n4, float wsum,
                                      float* __restrict__ out) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += stride) {
    float4 sv = reinterpret_cast<const float4*>(server)[i];
    const float* ss = reinterpret_cast<const float*>(&sv);
    float acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = wsum * ss[j];
    for (long c = 0; c < C; ++c) {
      float wc = w[c];
      if (wc == 0.f) continue;
      float4 rv = reinterpret_cast<const float4*>(replicas + c * n4 * 4)[i];
      const float* rr = reinterpret_cast<const float*>(&rv);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(-wc, rr[j], acc[j]);
    }
    float4 ov;
    float* oo = reinterpret_cast<float*>(&ov);
#pragma unroll
    for (int j = 0; j < 4; ++j) oo[j] = acc[j];
    reinterpret_cast<float4*>(out)[i] = ov;
  }
}

void multi_diff_accumulate(torch::Tensor server, torch::Tensor replicas,
                           torch::Tensor weights, torch::Tensor out,
                           double wsum) {
  CHK(server); CHK(replicas); CHK(out);
  long C = replicas.size(0);
  long n4 = server.numel() / 4;
  hipLaunchKernelGGL(multi_diff_acc_kernel, dim3(ft_grid(n4)),
                     dim3(FT_BLOCK), 0, STREAM, server.data_ptr<float>(),
                     replicas.data_ptr<float>(), weights.data_ptr<float>(),
                     C, n4, (float)wsum, out.data_ptr<float>());
}

// packed FedGATE / SCAFFOLD state rows, like multi_diff_acc_kernel: one thread
// per float4 of the arena, the loop over the clients inside the thread in
// client order (no atomics: bit-reproducible).  Rows with inv[c] == 0 are
// neither read nor written.  The per-row formulas are delta_kernel's and
// ctrl_kernel's + wdr_kernel's, expression for expression.
__global__ void multi_delta_kernel(float* __restrict__ delta,
                                   const float* __restrict__ server,
                                   const float* __restrict__ agg,
                                   const float* __restrict__ replicas,
                                   const float* __restrict__ inv, long C,
                                   long n4) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += stride) {
    float4 sv = reinterpret_cast<const float4*>(server)[i];
    float4 av = reinterpret_cast<const float4*>(agg)[i];
    const float* ss = reinterpret_cast<const float*>(&sv);
    const float* aa = reinterpret_cast<const float*>(&av);
    for (long c = 0; c < C; ++c) {
      const float coef = inv[c];
      if (coef == 0.f) continue;
      float4 dv = reinterpret_cast<float4*>(delta + c * n4 * 4)[i];
      float4 cv = reinterpret_cast<const float4*>(replicas + c * n4 * 4)[i];
      float* d = reinterpret_cast<float*>(&dv);
      const float* cc2 = reinterpret_cast<const float*>(&cv);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        d[j] = fmaf(coef, ss[j] - aa[j] - cc2[j], d[j]);
      reinterpret_cast<float4*>(delta + c * n4 * 4)[i] = dv;
    }
  }
}

static void multi_row_check(const char* who, const char* name,
                            const torch::Tensor& t, at::IntArrayRef shape,
                            const torch::Tensor& like) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() &&
                  t.scalar_type() == torch::kFloat && t.is_contiguous() &&
                  t.sizes() == shape,
              who, ": ", name, " must be contiguous fp32 ", shape,
              " on the GPU of the rows, got ", t.sizes());
}

void multi_delta_update(torch::Tensor delta, torch::Tensor server,
                        torch::Tensor agg, torch::Tensor replicas,
                        torch::Tensor inv) {
  const char* who = "multi_delta_update";
  TORCH_CHECK(delta.dim() == 2 && delta.is_cuda(), who,
              ": delta must be [C, N] on GPU");
  const long C = delta.size(0), N = delta.size(1);
  TORCH_CHECK(N % 4 == 0, who, ": arena numel must be float4-aligned");
  multi_row_check(who, "delta", delta, {C, N}, delta);
  multi_row_check(who, "server", server, {N}, delta);
  multi_row_check(who, "agg", agg, {N}, delta);
  multi_row_check(who, "replicas", replicas, {C, N}, delta);
  multi_row_check(who, "inv", inv, {C}, delta);
  if (C == 0 || N == 0) return;
  const long n4 = N / 4;
  hipLaunchKernelGGL(multi_delta_kernel, dim3(ft_grid(n4)), dim3(FT_BLOCK), 0,
                     STREAM, delta.data_ptr<float>(),
                     server.data_ptr<float>(), agg.data_ptr<float>(),
                     replicas.data_ptr<float>(), inv.data_ptr<float>(), C,
                     n4);
}

__global__ void multi_ctrl_kernel(float* __restrict__ ctrl,
                                  const float* __restrict__ ctrl_server,
                                  const float* __restrict__ server,
                                  const float* __restrict__ replicas,
                                  const float* __restrict__ inv,
                                  const float* __restrict__ w, long C,
                                  long n4, float* __restrict__ out) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += stride) {
    float4 b = reinterpret_cast<const float4*>(ctrl_server)[i];
    float4 sv = reinterpret_cast<const float4*>(server)[i];
    const float* bb = reinterpret_cast<const float*>(&b);
    const float* ss = reinterpret_cast<const float*>(&sv);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (long c = 0; c < C; ++c) {
      const float coef = inv[c];
      if (coef == 0.f) continue;
      const float wc = w[c];
      float4 a = reinterpret_cast<float4*>(ctrl + c * n4 * 4)[i];
      float4 cv = reinterpret_cast<const float4*>(replicas + c * n4 * 4)[i];
      float4 ov;
      float* o = reinterpret_cast<float*>(&ov);
      const float* aa = reinterpret_cast<const float*>(&a);
      const float* cc3 = reinterpret_cast<const float*>(&cv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = aa[j] - bb[j] + coef * (ss[j] - cc3[j]);
        acc[j] = fmaf(o[j] - aa[j], wc, acc[j]);
      }
      reinterpret_cast<float4*>(ctrl + c * n4 * 4)[i] = ov;
    }
    float4 rv;
    float* rr = reinterpret_cast<float*>(&rv);
#pragma unroll
    for (int j = 0; j < 4; ++j) rr[j] = acc[j];
    reinterpret_cast<float4*>(out)[i] = rv;
  }
}

void multi_scaffold_control_update(torch::Tensor ctrl,
                                   torch::Tensor ctrl_server,
                                   torch::Tensor server,
                                   torch::Tensor replicas, torch::Tensor inv,
                                   torch::Tensor weights, torch::Tensor out) {
  const char* who = "multi_scaffold_control_update";
  TORCH_CHECK(ctrl.dim() == 2 && ctrl.is_cuda(), who,
              ": ctrl must be [C, N] on GPU");
  const long C = ctrl.size(0), N = ctrl.size(1);
  TORCH_CHECK(N % 4 == 0, who, ": arena numel must be float4-aligned");
  multi_row_check(who, "ctrl", ctrl, {C, N}, ctrl);
  multi_row_check(who, "ctrl_server", ctrl_server, {N}, ctrl);
  multi_row_check(who, "server", server, {N}, ctrl);
  multi_row_check(who, "replicas", replicas, {C, N}, ctrl);
  multi_row_check(who, "inv", inv, {C}, ctrl);
  multi_row_check(who, "weights", weights, {C}, ctrl);
  multi_row_check(who, "out", out, {N}, ctrl);
  if (N == 0) return;
  const long n4 = N / 4;
  hipLaunchKernelGGL(multi_ctrl_kernel, dim3(ft_grid(n4)), dim3(FT_BLOCK), 0,
                     STREAM, ctrl.data_ptr<float>(),
                     ctrl_server.data_ptr<float>(), server.data_ptr<float>(),
                     replicas.data_ptr<float>(), inv.data_ptr<float>(),
                     weights.data_ptr<float>(), C, n4, out.data_ptr<float>());
}

// fused decompress + K-way sum: out = sum_k scatter(vs[k] @ idxs[k]) -------
__global__ void scatter_acc_kernel(const float* __restrict__ vs,
                                   const int* __restrict__ idxs, long total,
                                   float* __restrict__ out) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += stride)
    atomicAdd(&out[idxs[i]], vs[i]);
}

void scatter_accumulate(torch::Tensor out, torch::Tensor vs,
                        torch::Tensor idxs) {
  CHK(out); CHK(vs); CHK(idxs);
  out.zero_();
  long total = vs.numel();
  hipLaunchKernelGGL(scatter_acc_kernel, dim3(ft_grid(total)), dim3(FT_BLOCK),
                     0, STREAM, vs.data_ptr<float>(), idxs.data_ptr<int>(),
                     total, out.data_ptr<float>());
}

// ==========================================================================
// grad gather: scattered autograd-owned grad buffers -> flat grad arena.
//
// With p.grad = None at hipGraph-capture time, AccumulateGrad STEALS the
// produced tensor instead of launching one fp32 add per parameter per step
// (~65 CUDAFunctor_add kernels/step on ResNet-20, ~300 us at b256 —
// profiles/r01_bench_notes.md).  This single kernel then copies every
// stolen buffer into the contiguous grad arena that the fused SGD step and
// the grad-norm trackers read.  Chunk table is built once per capture on
// the host (shapes are static).
// ==========================================================================
// table row: (src_idx, src_off, dst_off, n, is_bf16).  bf16 sources (grads
// of bf16-compute params) are cast to fp32 during the copy — no separate
// cast kernel.
__global__ void gather_chunks_kernel(const unsigned long long* __restrict__
                                         srcs,
                                     const int* __restrict__ table /*[B,5]*/,
                                     float* __restrict__ dst) {
  const int* e = table + 5 * blockIdx.x;
  float* out = dst + e[2];
  const int n = e[3];
  if (e[4]) {  // bf16 source
    const __hip_bfloat16* src =
        reinterpret_cast<const __hip_bfloat16*>(srcs[e[0]]) + e[1];
    const int n8 = n >> 3;
    for (int i = threadIdx.x; i < n8; i += blockDim.x) {
      struct alignas(16) V8 { __hip_bfloat16 d[8]; };
      V8 v = reinterpret_cast<const V8*>(src)[i];
      float4 lo, hi;
      float* l = reinterpret_cast<float*>(&lo);
      float* h = reinterpret_cast<float*>(&hi);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        l[j] = __bfloat162float(v.d[j]);
        h[j] = __bfloat162float(v.d[4 + j]);
      }
      reinterpret_cast<float4*>(out)[2 * i] = lo;
      reinterpret_cast<float4*>(out)[2 * i + 1] = hi;
    }
    for (int i = (n8 << 3) + threadIdx.x; i < n; i += blockDim.x)
      out[i] = __bfloat162float(src[i]);
    return;
  }
  const float* src = reinterpret_cast<const float*>(srcs[e[0]]) + e[1];
  const int n4 = n >> 2;
  for (int i = threadIdx.x; i < n4; i += blockDim.x)
    reinterpret_cast<float4*>(out)[i] =
        reinterpret_cast<const float4*>(src)[i];
  for (int i = (n4 << 2) + threadIdx.x; i < n; i += blockDim.x)
    out[i] = src[i];
}

void gather_grads(torch::Tensor srcs, torch::Tensor table,
                  torch::Tensor dst) {
  CHK(dst); CHK(srcs); CHK(table);
  TORCH_CHECK(table.dim() == 2 && table.size(1) == 5, "table must be [B,5]");
  TORCH_CHECK(srcs.scalar_type() == torch::kLong, "srcs must be int64 ptrs");
  TORCH_CHECK(table.scalar_type() == torch::kInt, "table must be int32");
  const int B = (int)table.size(0);
  hipLaunchKernelGGL(gather_chunks_kernel, dim3(B), dim3(FT_BLOCK), 0,
                     STREAM,
                     reinterpret_cast<const unsigned long long*>(
                         srcs.data_ptr<long>()),
                     table.data_ptr<int>(), dst.data_ptr<float>());
}

// fp32 master arena -> bf16 compute arena (one pass; used after any direct
// mutation of the master outside the fused SGD kernel, e.g. aggregation)
__global__ void cast_half_kernel(const float* __restrict__ src,
                                 __hip_bfloat16* __restrict__ dst, long n8) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n8;
       i += stride) {
    float4 lo = reinterpret_cast<const float4*>(src)[2 * i];
    float4 hi = reinterpret_cast<const float4*>(src)[2 * i + 1];
    struct alignas(16) V8 { __hip_bfloat16 d[8]; };
    V8 v;
    const float* l = reinterpret_cast<const float*>(&lo);
    const float* h = reinterpret_cast<const float*>(&hi);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v.d[j] = __float2bfloat16(l[j]);
      v.d[4 + j] = __float2bfloat16(h[j]);
    }
    reinterpret_cast<V8*>(dst)[i] = v;
  }
}

void cast_to_half(torch::Tensor src, torch::Tensor dst) {
  CHK(src); CHK(dst);
  TORCH_CHECK(src.numel() == dst.numel() && src.numel() % 8 == 0,
              "cast_to_half: numel mismatch / not 8-aligned");
  long n8 = src.numel() / 8;
  hipLaunchKernelGGL(cast_half_kernel, dim3(ft_grid(n8)), dim3(FT_BLOCK), 0,
                     STREAM, src.data_ptr<float>(),
                     reinterpret_cast<__hip_bfloat16*>(dst.data_ptr()), n8);
}

// ==========================================================================
// What the 3x3 conv launchers share: the instance table, the dispatch over
// it, the argument checks and the pointer casts
// ==========================================================================
// One (channels, width, stride) instance the conv kernels are built for.
// W is the OUTPUT width, as the kernels expect; a launcher sees W_IN.
template <int CI_, int CO_, int CO_TILE_, int W_, int S_>
struct ConvInst {
  static constexpr int CI = CI_, CO = CO_, CO_TILE = CO_TILE_, W = W_, S = S_;
  static constexpr int W_IN = W * S;
  static constexpr int SPLIT = CO / CO_TILE;  // workgroups per 8-row tile
};

template <class... I>
struct ConvInstList {};

// the ResNet body convs (Co == Ci, stride 1) and the two transitions
// (Co == 2 Ci, stride 2): THE shape table of every launcher below
using ConvInsts = ConvInstList<
    ConvInst<16, 16, 16, 32, 1>, ConvInst<32, 32, 32, 16, 1>,
    ConvInst<64, 64, 32, 8, 1>, ConvInst<16, 32, 32, 16, 2>,
    ConvInst<32, 64, 32, 8, 2>>;

template <int S, class F, class... I>
static inline bool conv_match(ConvInstList<I...>, int Ci, int Co, int W_in,
                              F& f) {
  auto one = [&](auto inst) {
    using T = decltype(inst);
    if constexpr (T::S == S) {
      if (Ci == T::CI && Co == T::CO && W_in == T::W_IN) {
        f(inst);
        return true;
      }
    }
    return false;
  };
  return (one(I{}) || ...);
}

// f(ConvInst<...>{}) for the stride-S instance that matches, else the
// "unsupported" error.  S is a template argument so that a launcher
// instantiates its kernels for the instances of its own stride only.
template <int S, class F>
static inline void conv_dispatch(const char* who, int Ci, int Co, int W_in,
                                 F&& f) {
  TORCH_CHECK(conv_match<S>(ConvInsts{}, Ci, Co, W_in, f), who,
              ": unsupported (Ci,Co,W)=", Ci, ",", Co, ",", W_in,
              " at stride ", S);
}

// a runtime flag as the std::bool_constant a kernel's template flag takes
template <class F>
static inline void bool_dispatch(bool b, F&& f) {
  if (b) f(std::true_type{}); else f(std::false_type{});
}

static inline const __hip_bfloat16* bf16_ptr(const torch::Tensor& t) {
  return reinterpret_cast<const __hip_bfloat16*>(t.data_ptr());
}

static inline __hip_bfloat16* bf16_out(const torch::Tensor& t) {
  return reinterpret_cast<__hip_bfloat16*>(t.data_ptr());
}

// argument checks: the kernels index every pointer from the activation's
// sizes alone, so each tensor handed to them is validated here.  Optional
// arguments are absent when empty.
static inline bool conv_present(const torch::Tensor& t) {
  return t.defined() && t.numel() > 0;
}

// t: 4D bf16 channels_last on the GPU (activations, gradients, weights)
static inline void conv_check_act(const char* who, const char* name,
                                  const torch::Tensor& t) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 4, who, ": ", name,
              " must be 4D on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, who, ": ", name,
              " must be bf16");
  TORCH_CHECK(t.is_contiguous(at::MemoryFormat::ChannelsLast), who, ": ",
              name, " must be channels_last");
}

// t: conv_check_act with exactly these sizes
static inline void conv_check_like(const char* who, const char* name,
                                   const torch::Tensor& t,
                                   at::IntArrayRef sizes) {
  conv_check_act(who, name, t);
  TORCH_CHECK(t.sizes() == sizes, who, ": ", name, " must be ", sizes);
}

// dy of a weight-gradient launcher: the gradient of an [N, Co, H, W] output
static inline void conv_check_dy(const char* who, const torch::Tensor& dy,
                                 int N, int H, int W) {
  conv_check_act(who, "dy", dy);
  TORCH_CHECK(dy.size(0) == N && dy.size(2) == H && dy.size(3) == W, who,
              ": dy must be [N, Co, H, W] = [", N, ", Co, ", H, ", ", W, "]");
}

// w, after conv_check_act: [Co, Ci, 3, 3] (memory [Co][3][3][Ci])
static inline void conv_check_w(const char* who, const torch::Tensor& w,
                                int Co, int Ci) {
  TORCH_CHECK(w.size(0) == Co && w.size(1) == Ci && w.size(2) == 3 &&
                  w.size(3) == 3,
              who, ": w must be [Co, Ci, 3, 3] = [", Co, ", ", Ci,
              ", 3, 3]");
}

// a new channels_last tensor of t's dtype and device
static inline torch::Tensor conv_empty(const torch::Tensor& t,
                                       at::IntArrayRef sizes) {
  return torch::empty(
      sizes, t.options().memory_format(at::MemoryFormat::ChannelsLast));
}

// ==========================================================================
// MFMA wrw v2 (convwrw2.h): transposed LDS staging, alignbit tap shifts
// ==========================================================================
// supertile streams launched at most (a stream = the G workgroups that share
// one grid-stride walk over the supertiles).  Every stream emits one fp32
// copy of dw as partials (9 / 36 / 144 KB for C16 / C32 / C64), so the cap
// trades partial traffic against busy CUs; defaults from the N=256 sweep in
// profiles/wrw2_notes.md.  FT_WRW2_NBLK overrides (read per call, so one
// process can sweep it).  Exposed so the grid-stride remainder test can size
// its batch past it.
int conv3x3_wrw2_grid_cap(int C) {
  const int cap = ft_env_int("FT_WRW2_NBLK", 0);
  return cap > 0 ? cap : (C == 16 ? 256 : C == 32 ? 128 : 64);
}

// work split <COW, CIWV, NB> and final-kernel width CW of one instance
template <class I, int COW, int CIWV, int NB, int CW>
static torch::Tensor conv3x3_wrw2_launch(const torch::Tensor& dy,
                                         const torch::Tensor& x, int N,
                                         int H) {
  using C = Wrw2Cfg<I::CO, I::CI, I::W, COW, CIWV, NB>;
  // a supertile is 128 positions (64 at W=8) of whole rows of ONE image
  TORCH_CHECK(N > 0 && H > 0 && H % C::SR == 0,
              "conv3x3_wrw2: unsupported (N,H)=", N, ",", H);
  auto dw = conv_empty(x, {I::CO, I::CI, 3, 3});
  const long tiles = (long)N * (H / C::SR);
  const int cap = conv3x3_wrw2_grid_cap(I::CO);
  const int RQ = (int)(tiles < cap ? tiles : cap);   // streams = rows/quadrant
  auto part = torch::empty({(long)C::Q * RQ, 9L * 256},
                           x.options().dtype(torch::kFloat));
  hipLaunchKernelGGL((conv3x3_wrw2_k<I::CO, I::CI, I::W, COW, CIWV, NB>),
                     dim3(RQ * C::G), dim3(FT_BLOCK), 0, STREAM, bf16_ptr(dy),
                     bf16_ptr(x), part.data_ptr<float>(), N, H, RQ);
  hipLaunchKernelGGL(conv3x3_wrw2_final_k<CW>, dim3(C::Q * (9 * 256 / CW)),
                     dim3(FT_BLOCK), 0, STREAM, part.data_ptr<float>(), RQ,
                     bf16_out(dw), I::CO);
  return dw;
}

torch::Tensor conv3x3_wrw2(torch::Tensor dy, torch::Tensor x) {
  const char* who = "conv3x3_wrw2";
  conv_check_act(who, "x", x);
  const int N = x.size(0), Ci = x.size(1), H = x.size(2), W = x.size(3);
  conv_check_dy(who, dy, N, H, W);
  const int Co = dy.size(1);
  torch::Tensor dw;
  // the splits: header of convwrw2.h and the sweep in profiles/wrw2_notes.md
  conv_dispatch<1>(who, Ci, Co, W, [&](auto inst) {
    using I = decltype(inst);
    if constexpr (I::CO == 16)
      dw = conv3x3_wrw2_launch<I, 1, 1, 1, 16>(dy, x, N, H);
    else if constexpr (I::CO == 32)
      dw = conv3x3_wrw2_launch<I, 2, 1, 1, 32>(dy, x, N, H);
    else
      dw = conv3x3_wrw2_launch<I, 2, 2, 1, 32>(dy, x, N, H);
  });
  return dw;
}

// ==========================================================================
// MFMA direct NHWC 3x3/s1/p1 conv FORWARD with fused BN prologue/epilogue
// (convfwd.h)
// ==========================================================================

// ysum: [grid, Co, 2] fp32 stats partials, or empty
static inline float* conv_check_ysum(const char* who,
                                     const torch::Tensor& ysum, long grid,
                                     int Co) {
  if (!conv_present(ysum)) return nullptr;
  TORCH_CHECK(ysum.is_cuda() && ysum.scalar_type() == torch::kFloat &&
                  ysum.is_contiguous(),
              who, ": ysum must be contiguous fp32 on GPU");
  TORCH_CHECK(ysum.numel() == grid * Co * 2, who,
              ": ysum must be [grid, Co, 2] fp32, grid=", grid);
  return ysum.data_ptr<float>();
}

torch::Tensor conv3x3_bn_fwd(torch::Tensor x, torch::Tensor w,
                             torch::Tensor ysum, torch::Tensor in_a,
                             torch::Tensor in_b, torch::Tensor res,
                             bool relu_in) {
  const char* who = "conv3x3_bn_fwd";
  conv_check_act(who, "x", x);
  conv_check_act(who, "w", w);
  const int N = x.size(0), Ci = x.size(1), H = x.size(2), W = x.size(3);
  const int Co = w.size(0);
  TORCH_CHECK(N > 0 && H > 0 && H % 8 == 0, who, ": unsupported (N,H)=", N,
              ",", H);
  conv_check_w(who, w, Co, Ci);
  TORCH_CHECK(conv_present(in_a) == conv_present(in_b), who,
              ": in_a and in_b go together");
  const float* ap = nullptr;
  const float* bp = nullptr;
  if (conv_present(in_a)) {
    TORCH_CHECK(in_a.is_cuda() && in_b.is_cuda() &&
                    in_a.scalar_type() == torch::kFloat &&
                    in_b.scalar_type() == torch::kFloat &&
                    in_a.is_contiguous() && in_b.is_contiguous() &&
                    in_a.numel() == Ci && in_b.numel() == Ci,
                who, ": in_a/in_b must be fp32 [Ci] on GPU, Ci=", Ci);
    ap = in_a.data_ptr<float>();
    bp = in_b.data_ptr<float>();
  }
  const __hip_bfloat16* rp = nullptr;
  if (conv_present(res)) {
    conv_check_like(who, "res", res, x.sizes());
    rp = bf16_ptr(res);
  }
  TORCH_CHECK(!rp || ap, who, ": residual needs in_a/in_b");
  torch::Tensor y;
  conv_dispatch<1>(who, Ci, Co, W, [&](auto inst) {
    using I = decltype(inst);
    const int grid = N * (H / 8) * I::SPLIT;
    float* ysp = conv_check_ysum(who, ysum, grid, Co);
    y = conv_empty(x, {N, Co, H, W});
    auto launch = [&](auto fuse_in, auto has_res) {
      hipLaunchKernelGGL(
          (conv3x3_bn_fwd_k<I::CI, I::CO, I::CO_TILE, I::W,
                            decltype(fuse_in)::value,
                            decltype(has_res)::value>),
          dim3(grid), dim3(FT_BLOCK), 0, STREAM, bf16_ptr(x), bf16_ptr(w),
          bf16_out(y), ysp, ap, bp, rp, N, H, relu_in ? 1 : 0);
    };
    // the three flag pairs the kernel is built for
    if (rp) launch(std::true_type{}, std::true_type{});
    else if (ap) launch(std::true_type{}, std::false_type{});
    else launch(std::false_type{}, std::false_type{});
  });
  return y;
}

// ==========================================================================
// MFMA fused conv fwd, STRIDE 2 (the ResNet transition convs)
// ==========================================================================
torch::Tensor conv3x3s2_bn_fwd(torch::Tensor x, torch::Tensor w,
                               torch::Tensor ysum) {
  const char* who = "conv3x3s2_bn_fwd";
  conv_check_act(who, "x", x);
  conv_check_act(who, "w", w);
  const int N = x.size(0), Ci = x.size(1), HI = x.size(2), WI = x.size(3);
  const int Co = w.size(0);
  const int H = HI / 2;
  TORCH_CHECK(N > 0 && HI > 0 && HI % 16 == 0, who,
              ": unsupported (N,H_in)=", N, ",", HI);
  conv_check_w(who, w, Co, Ci);
  torch::Tensor y;
  conv_dispatch<2>(who, Ci, Co, WI, [&](auto inst) {
    using I = decltype(inst);
    const int grid = N * (H / 8) * I::SPLIT;
    float* ysp = conv_check_ysum(who, ysum, grid, Co);
    y = conv_empty(x, {N, Co, H, I::W});
    hipLaunchKernelGGL(
        (conv3x3_bn_fwd_k<I::CI, I::CO, I::CO_TILE, I::W, false, false, 2>),
        dim3(grid), dim3(FT_BLOCK), 0, STREAM, bf16_ptr(x), bf16_ptr(w),
        bf16_out(y), ysp, nullptr, nullptr, nullptr, N, H, 0);
  });
  return y;
}

// ==========================================================================
// MFMA conv fwd with the INFERENCE epilogue (convfwd.h
// conv3x3_bn_act_fwd_k): y = [relu](bn_running(conv3x3(x, w)) [+ res]),
// stride 1 (body shapes) or 2 (transitions), one launch
// ==========================================================================
// t: contiguous fp32 [n] on the GPU
static inline const float* conv_check_vec(const char* who, const char* name,
                                          const torch::Tensor& t, int n) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat, who, ": ",
              name, " must be fp32 on GPU");
  TORCH_CHECK(t.dim() == 1 && t.size(0) == n && t.is_contiguous(), who, ": ",
              name, " must be contiguous [Co] = [", n, "]");
  return t.data_ptr<float>();
}

torch::Tensor conv3x3_bn_act_fwd(torch::Tensor x, torch::Tensor w,
                                 torch::Tensor gamma, torch::Tensor beta,
                                 torch::Tensor running_mean,
                                 torch::Tensor running_var, double eps,
                                 bool relu, torch::Tensor res, long stride) {
  const char* who = "conv3x3_bn_act_fwd";
  TORCH_CHECK(stride == 1 || stride == 2, who, ": stride must be 1 or 2, got ",
              stride);
  conv_check_act(who, "x", x);
  conv_check_act(who, "w", w);
  const int N = x.size(0), Ci = x.size(1), HI = x.size(2), WI = x.size(3);
  const int Co = w.size(0);
  const int S = (int)stride;
  TORCH_CHECK(N > 0 && HI > 0 && HI % (8 * S) == 0, who,
              ": unsupported (N,H)=", N, ",", HI, " at stride ", S);
  conv_check_w(who, w, Co, Ci);
  const float* gp = conv_check_vec(who, "gamma", gamma, Co);
  const float* bp = conv_check_vec(who, "beta", beta, Co);
  const float* mp = conv_check_vec(who, "running_mean", running_mean, Co);
  const float* vp = conv_check_vec(who, "running_var", running_var, Co);
  const int H = HI / S, W = WI / S;
  const __hip_bfloat16* rp = nullptr;
  if (conv_present(res)) {
    conv_check_like(who, "res", res, {N, Co, H, W});   // the OUTPUT shape
    rp = bf16_ptr(res);
  }
  TORCH_CHECK((long)N * (H / 8) * 2 < (1L << 31), who, ": N too large");
  torch::Tensor y;
  auto run = [&](auto inst) {
    using I = decltype(inst);
    const int grid = N * (H / 8) * I::SPLIT;
    y = conv_empty(x, {N, Co, H, W});
    bool_dispatch(rp != nullptr, [&](auto has_res) {
      hipLaunchKernelGGL(
          (conv3x3_bn_act_fwd_k<I::CI, I::CO, I::CO_TILE, I::W,
                                decltype(has_res)::value, I::S>),
          dim3(grid), dim3(FT_BLOCK), 0, STREAM, bf16_ptr(x), bf16_ptr(w),
          bf16_out(y), gp, bp, mp, vp, rp, (float)eps, N, H, relu ? 1 : 0);
    });
  };
  if (S == 1) conv_dispatch<1>(who, Ci, Co, WI, run);
  else conv_dispatch<2>(who, Ci, Co, WI, run);
  return y;
}

// ==========================================================================
// MFMA direct conv backward-data (convfwd.h conv3x3_dgrad_k)
// ==========================================================================
torch::Tensor conv3x3_dgrad(torch::Tensor dy, torch::Tensor w) {
  const char* who = "conv3x3_dgrad";
  conv_check_act(who, "dy", dy);
  conv_check_act(who, "w", w);
  const int N = dy.size(0), Co = dy.size(1), H = dy.size(2),
            W = dy.size(3);
  const int Ci = w.size(1);
  TORCH_CHECK(N > 0 && H > 0 && H % 8 == 0, who, ": unsupported (N,H)=", N,
              ",", H);
  conv_check_w(who, w, Co, Ci);
  torch::Tensor dx;
  // the output tile of the mirror kernel is a CI tile; Ci == Co here
  conv_dispatch<1>(who, Ci, Co, W, [&](auto inst) {
    using I = decltype(inst);
    dx = conv_empty(dy, {N, Ci, H, W});
    hipLaunchKernelGGL(
        (conv3x3_dgrad_k<I::CI, I::CO, I::CO_TILE, I::W, false>),
        dim3(N * (H / 8) * I::SPLIT), dim3(FT_BLOCK), 0, STREAM,
        bf16_ptr(dy), bf16_ptr(w), bf16_out(dx), nullptr, nullptr, nullptr,
        nullptr, nullptr, N, H, 0);
  });
  return dx;
}

// deferred-BN-backward dgrad: dy here is dz (the BN output gradient);
// the kernel applies dy_conv = A*mask(dz) + B + D*x_bn while staging and
// ALSO writes dy_conv out (the wrw consumer reads it) — the separate
// bnh_bwd_dx pass disappears.
std::vector<torch::Tensor> conv3x3_dgrad_bn(
    torch::Tensor dz, torch::Tensor w, torch::Tensor xbn, torch::Tensor z,
    torch::Tensor coefs, bool relu, torch::Tensor dres) {
  const char* who = "conv3x3_dgrad_bn";
  conv_check_act(who, "dz", dz);
  conv_check_act(who, "w", w);
  const int N = dz.size(0), Co = dz.size(1), H = dz.size(2),
            W = dz.size(3);
  const int Ci = w.size(1);
  TORCH_CHECK(N > 0 && H > 0 && H % 8 == 0, who, ": unsupported (N,H)=", N,
              ",", H);
  conv_check_w(who, w, Co, Ci);
  conv_check_like(who, "xbn", xbn, dz.sizes());
  conv_check_like(who, "z", z, dz.sizes());
  TORCH_CHECK(coefs.numel() == 3 * Co && coefs.is_cuda() &&
                  coefs.scalar_type() == torch::kFloat &&
                  coefs.is_contiguous(),
              who, ": coefs must be fp32 [3, Co]");
  const bool want_dres = conv_present(dres);
  if (want_dres) conv_check_like(who, "dres", dres, dz.sizes());
  torch::Tensor dx, dyc;
  conv_dispatch<1>(who, Ci, Co, W, [&](auto inst) {
    using I = decltype(inst);
    dx = conv_empty(dz, {N, Ci, H, W});
    dyc = torch::empty_like(dz);
    bool_dispatch(want_dres, [&](auto has_dres) {
      hipLaunchKernelGGL(
          (conv3x3_dgrad_k<I::CI, I::CO, I::CO_TILE, I::W, true,
                           decltype(has_dres)::value>),
          dim3(N * (H / 8) * I::SPLIT), dim3(FT_BLOCK), 0, STREAM,
          bf16_ptr(dz), bf16_ptr(w), bf16_out(dx), bf16_ptr(xbn), bf16_ptr(z),
          coefs.data_ptr<float>(), bf16_out(dyc),
          want_dres ? bf16_out(dres) : nullptr, N, H, relu ? 1 : 0);
    });
  });
  return {dx, dyc};
}

// ==========================================================================
// MFMA backward of the 3x3/s2 transition convs (convs2bwd.h)
// ==========================================================================
torch::Tensor conv3x3s2_dgrad(torch::Tensor dy, torch::Tensor w) {
  const char* who = "conv3x3s2_dgrad";
  conv_check_act(who, "dy", dy);
  conv_check_act(who, "w", w);
  const int N = dy.size(0), Co = dy.size(1);
  const int HI = dy.size(2) * 2, WI = dy.size(3) * 2;
  const int Ci = w.size(1);
  TORCH_CHECK(HI > 0 && HI % 16 == 0, who, ": H_in % 16 != 0");
  conv_check_w(who, w, Co, Ci);
  torch::Tensor dx;
  conv_dispatch<2>(who, Ci, Co, WI, [&](auto inst) {
    using I = decltype(inst);
    // a workgroup: 256 input pixels (whole rows) x 16 input channels
    constexpr int CI_TILE = 16, R = 256 / I::W_IN;
    dx = conv_empty(dy, {N, Ci, HI, WI});
    if (N == 0) return;
    hipLaunchKernelGGL((conv3x3s2_dgrad_k<I::CI, I::CO, CI_TILE, I::W_IN>),
                       dim3(N * (HI / R) * (I::CI / CI_TILE)),
                       dim3(FT_BLOCK), 0, STREAM, bf16_ptr(dy), bf16_ptr(w),
                       bf16_out(dx), N, HI);
  });
  return dx;
}

// supertile streams launched at most.  Every stream emits one fp32 copy of
// dw as partials (18 KB for 16->32, 72 KB for 32->64), so the cap trades
// partial traffic against busy CUs; measured best at N=256: 256 / 128
// (profiles/s2bwd_notes.md).  Exposed so the grid-stride remainder test
// can size its batch past it.
int conv3x3s2_wrw_grid_cap(int Ci) {
  static const int cap = ft_env_int("FT_S2WRW_NBLK", 0);
  return cap > 0 ? cap : (Ci == 16 ? 256 : 128);
}

torch::Tensor conv3x3s2_wrw(torch::Tensor dy, torch::Tensor x) {
  const char* who = "conv3x3s2_wrw";
  conv_check_act(who, "x", x);
  const int N = x.size(0), Ci = x.size(1), HI = x.size(2), WI = x.size(3);
  TORCH_CHECK(N > 0 && HI > 0 && HI % 16 == 0, who,
              ": unsupported (N,H_in)=", N, ",", HI);
  conv_check_dy(who, dy, N, HI / 2, WI / 2);
  const int Co = dy.size(1);
  torch::Tensor dw;
  conv_dispatch<2>(who, Ci, Co, WI, [&](auto inst) {
    using I = decltype(inst);
    constexpr int Q = (I::CO / 16) * (I::CI / 16);
    dw = conv_empty(x, {Co, Ci, 3, 3});
    const long tiles = (long)N * (HI / 16);        // 8 output rows each
    const int cap = conv3x3s2_wrw_grid_cap(Ci);
    const int RQ = (int)(tiles < cap ? tiles : cap);   // rows per quadrant
    auto part = torch::empty({(long)Q * RQ, 9L * 256},
                             x.options().dtype(torch::kFloat));
    hipLaunchKernelGGL((conv3x3s2_wrw_k<I::CO, I::CI, I::W_IN>), dim3(RQ),
                       dim3(FT_BLOCK), 0, STREAM, bf16_ptr(dy), bf16_ptr(x),
                       part.data_ptr<float>(), N, HI, RQ);
    hipLaunchKernelGGL(conv3x3_wrw2_final_k<32>, dim3(Q * 72),
                       dim3(FT_BLOCK), 0, STREAM, part.data_ptr<float>(), RQ,
                       bf16_out(dw), Ci);
  });
  return dw;
}

// ==========================================================================
// MFMA 3x3/s1/p1 NHWC bf16 conv weight gradient (convwrw.h)
// ==========================================================================
torch::Tensor conv3x3_wrw(torch::Tensor dy, torch::Tensor x) {
  const char* who = "conv3x3_wrw";
  conv_check_act(who, "x", x);
  const int N = x.size(0), Ci = x.size(1), H = x.size(2), W = x.size(3);
  conv_check_dy(who, dy, N, H, W);
  const int Co = dy.size(1);
  static const int cap1 = ft_env_int("FT_WRW_NBLK1", 256);
  static const int capq = ft_env_int("FT_WRW_NBLKQ", 128);
  torch::Tensor dw;
  conv_dispatch<1>(who, Ci, Co, W, [&](auto inst) {
    using I = decltype(inst);
    constexpr int R = 32 / I::W;   // image rows per 32-position K-tile
    TORCH_CHECK(H % R == 0, who, ": H % (32/W) != 0");
    const long tiles = (long)N * (H / R);
    int nblk, groups;
    if (I::CO == 16) {  // Q==1: 4 independent tile streams per block
      groups = 4;
      long b = (tiles + 4 * 4 - 1) / (4 * 4);  // >=4 tiles per stream
      nblk = (int)(b < 1 ? 1 : (b > cap1 ? cap1 : b));
    } else {
      groups = 1;
      long b = tiles > capq ? capq : tiles;
      nblk = (int)(b < 1 ? 1 : b);
    }
    const long rows = (long)nblk * groups;
    auto part = torch::empty({rows, (long)9 * Co * Ci},
                             x.options().dtype(torch::kFloat));
    dw = conv_empty(x, {Co, Ci, 3, 3});
    hipLaunchKernelGGL((conv3x3_wrw_k<I::CO, I::CI, I::W>), dim3(nblk),
                       dim3(FT_BLOCK), 0, STREAM, bf16_ptr(dy), bf16_ptr(x),
                       part.data_ptr<float>(), N, H);
    const int wn = Co * 9 * Ci;
    hipLaunchKernelGGL(conv3x3_wrw_final_k, dim3((wn + 63) / 64),
                       dim3(FT_BLOCK), 0, STREAM, part.data_ptr<float>(),
                       rows, wn, bf16_out(dw), Co, Ci);
  });
  return dw;
}

// ==========================================================================
// MFMA layout probe (convwrw.h) — used by the GPU layout test
// ==========================================================================
torch::Tensor mfma_probe(torch::Tensor A, torch::Tensor B) {
  CHK(A); CHK(B);
  TORCH_CHECK(A.scalar_type() == torch::kBFloat16 && A.numel() == 16 * 32
                  && B.numel() == 32 * 16, "probe expects A[16,32] B[32,16] bf16");
  auto D = torch::empty({16, 16}, A.options().dtype(torch::kFloat));
  hipLaunchKernelGGL(mfma_probe_gemm, dim3(1), dim3(64), 0, STREAM,
                     bf16_ptr(A), bf16_ptr(B), D.data_ptr<float>());
  return D;
}

// ==========================================================================
// NHWC stem convolution (kernels in stemconv.h)
// ==========================================================================
static inline bool stem_cl(const torch::Tensor& t) {
  return t.is_contiguous(at::MemoryFormat::ChannelsLast);
}

torch::Tensor stem_conv_fwd(torch::Tensor x, torch::Tensor w, bool out_bf16) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && stem_cl(x),
              "stem_conv_fwd: x must be 4D channels_last on GPU");
  TORCH_CHECK(w.is_cuda() && w.dim() == 4 && stem_cl(w)
                  && w.scalar_type() == torch::kFloat,
              "stem_conv_fwd: w must be fp32 channels_last");
  const int N = x.size(0), Ci = x.size(1), H = x.size(2), W = x.size(3);
  const int Co = w.size(0);
  TORCH_CHECK(w.size(1) == Ci && w.size(2) == 3 && w.size(3) == 3
                  && Ci == 3 && (Co == 16 || Co == 32),
              "stem_conv_fwd: supported shapes are Ci=3, Co in {16,32}");
  auto y = torch::empty({N, Co, H, W},
                        x.options()
                            .dtype(out_bf16 ? torch::kBFloat16
                                            : torch::kFloat)
                            .memory_format(at::MemoryFormat::ChannelsLast));
  const long total = (long)N * H * W;
  const int grid = ft_grid(total);
  AT_DISPATCH_FLOATING_TYPES_AND(at::ScalarType::BFloat16, x.scalar_type(),
                                 "stem_fwd", [&] {
    using TX = std::conditional_t<std::is_same_v<scalar_t, at::BFloat16>,
                                  __hip_bfloat16, scalar_t>;
    if (out_bf16) {
      auto* yp = reinterpret_cast<__hip_bfloat16*>(y.data_ptr());
      if (Co == 16)
        hipLaunchKernelGGL((stem_fwd_k<TX, __hip_bfloat16, 3, 16>),
                           dim3(grid), dim3(FT_BLOCK), 0, STREAM,
                           reinterpret_cast<const TX*>(x.data_ptr()),
                           w.data_ptr<float>(), yp, N, H, W);
      else
        hipLaunchKernelGGL((stem_fwd_k<TX, __hip_bfloat16, 3, 32>),
                           dim3(grid), dim3(FT_BLOCK), 0, STREAM,
                           reinterpret_cast<const TX*>(x.data_ptr()),
                           w.data_ptr<float>(), yp, N, H, W);
    } else {
      auto* yp = reinterpret_cast<float*>(y.data_ptr());
      if (Co == 16)
        hipLaunchKernelGGL((stem_fwd_k<TX, float, 3, 16>), dim3(grid),
                           dim3(FT_BLOCK), 0, STREAM,
                           reinterpret_cast<const TX*>(x.data_ptr()),
                           w.data_ptr<float>(), yp, N, H, W);
      else
        hipLaunchKernelGGL((stem_fwd_k<TX, float, 3, 32>), dim3(grid),
                           dim3(FT_BLOCK), 0, STREAM,
                           reinterpret_cast<const TX*>(x.data_ptr()),
                           w.data_ptr<float>(), yp, N, H, W);
    }
  });
  return y;
}

torch::Tensor stem_conv_wrw(torch::Tensor dy, torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && stem_cl(x), "stem_wrw: x");
  TORCH_CHECK(dy.is_cuda() && dy.dim() == 4 && stem_cl(dy), "stem_wrw: dy");
  const int N = x.size(0), Ci = x.size(1), H = x.size(2), W = x.size(3);
  const int Co = dy.size(1);
  TORCH_CHECK(Ci == 3 && (Co == 16 || Co == 32),
              "stem_wrw: supported shapes are Ci=3, Co in {16,32}");
  TORCH_CHECK(dy.size(0) == N && dy.size(2) == H && dy.size(3) == W,
              "stem_wrw: dy must be [N, Co, H, W] of x");
  TORCH_CHECK(at::isFloatingType(x.scalar_type()) &&
                  at::isFloatingType(dy.scalar_type()),
              "stem_wrw: floating-point x and dy only");
  const int wn = Co * 9 * Ci;
  const int B = 1024;
  auto f32 = x.options().dtype(torch::kFloat);
  auto part = torch::empty({B, wn}, f32);
  auto dw = torch::empty(
      {Co, Ci, 3, 3}, f32.memory_format(at::MemoryFormat::ChannelsLast));
  AT_DISPATCH_FLOATING_TYPES_AND(at::ScalarType::BFloat16, x.scalar_type(),
                                 "stem_wrw_x", [&] {
    using TX = std::conditional_t<std::is_same_v<scalar_t, at::BFloat16>,
                                  __hip_bfloat16, scalar_t>;
    AT_DISPATCH_FLOATING_TYPES_AND(at::ScalarType::BFloat16,
                                   dy.scalar_type(), "stem_wrw_dy", [&] {
      using TY = std::conditional_t<std::is_same_v<scalar_t, at::BFloat16>,
                                    __hip_bfloat16, scalar_t>;
      if (Co == 16)
        hipLaunchKernelGGL((stem_wrw_k<TY, TX, 3, 16>), dim3(B),
                           dim3(FT_BLOCK), 0, STREAM,
                           reinterpret_cast<const TY*>(dy.data_ptr()),
                           reinterpret_cast<const TX*>(x.data_ptr()),
                           part.data_ptr<float>(), N, H, W);
      else
        hipLaunchKernelGGL((stem_wrw_k<TY, TX, 3, 32>), dim3(B),
                           dim3(FT_BLOCK), 0, STREAM,
                           reinterpret_cast<const TY*>(dy.data_ptr()),
                           reinterpret_cast<const TX*>(x.data_ptr()),
                           part.data_ptr<float>(), N, H, W);
    });
  });
  hipLaunchKernelGGL(stem_wrw_final_k,
                     dim3((wn + FT_BLOCK / WAVE - 1) / (FT_BLOCK / WAVE)),
                     dim3(FT_BLOCK), 0, STREAM, part.data_ptr<float>(), B,
                     wn, dw.data_ptr<float>());
  return dw;
}

// ==========================================================================
// fused spatial BatchNorm (training fwd/bwd) — kernels in batchnorm.h
// ==========================================================================
// number of per-channel partial blocks for the reduction kernels: target
// ~512 blocks total (2/CU for a ~2-5 us kernel), ≤64 partials per channel
// so the consumer's finalize loop stays trivial.
static inline int bn_nparts(long per_v, long C) {
  long target = 512 / (C > 0 ? C : 1);
  long by_work = (per_v + FT_BLOCK - 1) / FT_BLOCK;
  long B = target < by_work ? target : by_work;
  if (B > 64) B = 64;
  if (B < 1) B = 1;
  return (int)B;
}

// grid.x for the elementwise kernels (pure streaming, no partial buffer):
// ~1024 blocks total, 2+ vector-iterations per thread.
static inline int bn_ew_chunks(long per_v, long C) {
  long cap = 1024 / (C > 0 ? C : 1);
  long by_work = (per_v + FT_BLOCK - 1) / FT_BLOCK;
  long c = cap < by_work ? cap : by_work;
  return (int)(c < 1 ? 1 : c);
}

// NHWC eligibility: C a multiple of the 16 B vector width with a
// power-of-two group count ≤ 64 lanes and ≤ 256 (blockDim) channels.
static inline bool bnh_ok(long C, int VN) {
  if (C <= 0 || C > 256 || C % VN) return false;
  long cgc = C / VN;
  return cgc <= 64 && (cgc & (cgc - 1)) == 0;
}
static inline int bnh_lgc(long C, int VN) {
  int l = 0;
  for (long c = C / VN; c > 1; c >>= 1) ++l;
  return l;
}
static inline int bnh_red_grid(long tasks) {
  static const int cap = ft_env_int("FT_BNH_RED_CAP", 256);
  static const int iters = ft_env_int("FT_BNH_RED_ITERS", 8);
  long b = (tasks + FT_BLOCK * iters - 1) / (FT_BLOCK * iters);
  if (b > cap) b = cap;
  return (int)(b < 1 ? 1 : b);
}
static inline int bnh_ew_grid(long tasks) {
  static const int cap = ft_env_int("FT_BNH_EW_CAP", 1024);
  static const int iters = ft_env_int("FT_BNH_EW_ITERS", 2);
  long b = (tasks + FT_BLOCK * iters - 1) / (FT_BLOCK * iters);
  if (b > cap) b = cap;
  return (int)(b < 1 ? 1 : b);
}

// ---- launcher argument checks (all run before any allocation/launch) ----
// 16 B vector width of the NHWC kernels for x's dtype; 0 = unsupported
static inline int bn_vn(const torch::Tensor& x) {
  switch (x.scalar_type()) {
    case torch::kBFloat16: return 8;
    case torch::kFloat: return 4;
    case torch::kDouble: return 2;
    default: return 0;
  }
}

// x: 4D on the GPU, bf16/fp32/fp64, N*HW < 2^31 (u32 row/element indices)
static inline void bn_check_x(const char* who, const torch::Tensor& x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, who, ": x must be 4D on GPU");
  TORCH_CHECK(bn_vn(x) != 0, who, ": x must be bf16, fp32 or fp64");
  TORCH_CHECK(x.size(0) * x.size(2) * x.size(3) < (1L << 31), who,
              ": N*HW must fit in int32");
}

// activation-shaped operand: same dtype, sizes and memory layout as x
static inline void bn_check_like(const char* who, const char* name,
                                 const torch::Tensor& t,
                                 const torch::Tensor& x, bool nhwc) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == x.scalar_type(), who, ": ",
              name, " must match x (same dtype, on GPU)");
  TORCH_CHECK(t.dim() == 4 && t.sizes() == x.sizes() &&
                  (nhwc ? t.is_contiguous(at::MemoryFormat::ChannelsLast)
                        : t.is_contiguous()),
              who, ": ", name, " must match x (", x.sizes(), ", ",
              nhwc ? "channels_last" : "contiguous", ")");
}

// per-channel fp32 vector of length C; an empty tensor means "absent"
static inline const float* bn_check_vec(const char* who, const char* name,
                                        const torch::Tensor& t, long C,
                                        bool optional) {
  if (!conv_present(t)) {
    TORCH_CHECK(optional, who, ": ", name, " must be fp32 [C] = [", C, "]");
    return nullptr;
  }
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat, who, ": ",
              name, " must be fp32 on GPU");
  TORCH_CHECK(t.numel() == C && t.is_contiguous(), who, ": ", name,
              " must be contiguous [C] = [", C, "]");
  return t.data_ptr<float>();
}

// running_mean / running_var go together
static inline void bn_check_running(const char* who,
                                    const torch::Tensor& running_mean,
                                    const torch::Tensor& running_var,
                                    long C) {
  TORCH_CHECK(conv_present(running_mean) == conv_present(running_var), who,
              ": running_mean and running_var go together");
  bn_check_vec(who, "running_mean", running_mean, C, true);
  bn_check_vec(who, "running_var", running_var, C, true);
}

// collapse [G, C, 2] stats partials to [B2, C, 2]: bnh_norm_k's
// per-block finalize re-reads ALL partial rows in EVERY normalize block
// (B=1024 conv-epilogue rows measured 21 us/norm vs 7.9 at B~64).
__global__ void __launch_bounds__(FT_BLOCK) part_reduce_k(
    const float* __restrict__ part, long G, int cols /* C*2 */,
    float* __restrict__ out, int B2) {
  // block b: rows [b*G/B2, (b+1)*G/B2), 2D thread split (row-parallel x
  // col) + LDS tree — the first serial-per-column version measured
  // 7.9 us/call (105 us/step over 19 layers)
  __shared__ float lds[FT_BLOCK];
  const long r0 = (long)blockIdx.x * G / B2;
  const long r1 = (long)(blockIdx.x + 1) * G / B2;
  if (cols > FT_BLOCK) {
    // more columns than threads (C > 128): no row-parallel split, each
    // thread walks columns c, c + FT_BLOCK, ... serially over the rows
    for (int cc = threadIdx.x; cc < cols; cc += FT_BLOCK) {
      float a = 0.f;
      for (long r = r0; r < r1; ++r) a += part[r * cols + cc];
      out[(long)blockIdx.x * cols + cc] = a;
    }
    return;
  }
  const int rp = FT_BLOCK / cols;            // row-parallel factor
  const int c = threadIdx.x % cols, p = threadIdx.x / cols;
  float s = 0.f;
  if (p < rp)
    for (long r = r0 + p; r < r1; r += rp) s += part[r * cols + c];
  lds[threadIdx.x] = s;
  __syncthreads();
  if (p == 0) {
    for (int i = 1; i < rp; ++i) s += lds[i * cols + c];
    out[(long)blockIdx.x * cols + c] = s;
  }
}

// bn_fwd_train with PRECOMPUTED stats partials (conv3x3_bn_fwd epilogue
// rows, [B, C, 2] fp32): the bnh_stats pass is skipped entirely — one
// bnh_norm_k launch finalizes the partials and normalizes.
std::vector<torch::Tensor> bn_fwd_train_part(
    torch::Tensor x, torch::Tensor part, torch::Tensor weight,
    torch::Tensor bias, torch::Tensor running_mean, torch::Tensor running_var,
    double eps, double momentum, bool relu, torch::Tensor res) {
  const char* who = "bn_fwd_train_part";
  bn_check_x(who, x);
  const bool nhwc =
      x.is_contiguous(at::MemoryFormat::ChannelsLast) && !x.is_contiguous();
  TORCH_CHECK(nhwc, "bn_fwd_train_part: channels_last only");
  long N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  TORCH_CHECK(bnh_ok(C, bn_vn(x)), "bn_fwd_train_part: unsupported C=", C);
  TORCH_CHECK(part.is_cuda() && part.dim() == 3 && part.size(1) == C &&
                  part.size(2) == 2 &&
                  part.scalar_type() == torch::kFloat,
              "bn_fwd_train_part: part must be [B, C, 2] fp32");
  TORCH_CHECK(part.size(0) >= 1 && part.is_contiguous(),
              "bn_fwd_train_part: part must be contiguous with B >= 1 rows");
  bn_check_vec(who, "weight", weight, C, true);
  bn_check_vec(who, "bias", bias, C, true);
  bn_check_running(who, running_mean, running_var, C);
  if (conv_present(res)) bn_check_like(who, "res", res, x, true);
  auto f32 = x.options().dtype(torch::kFloat);
  auto save_mean = torch::empty({C}, f32);
  auto save_ivar = torch::empty({C}, f32);
  auto y = torch::empty_like(x);
  auto mask = torch::empty({0}, x.options().dtype(torch::kByte));
  bool track = running_mean.numel() > 0;
  if (part.size(0) > 64) {
    const int B2 = 32;
    auto small = torch::empty({B2, C, 2}, f32);
    hipLaunchKernelGGL(part_reduce_k, dim3(B2), dim3(FT_BLOCK), 0, STREAM,
                       part.data_ptr<float>(), part.size(0), (int)(C * 2),
                       small.data_ptr<float>(), B2);
    part = small;
  }
  const int B = (int)part.size(0);
  AT_DISPATCH_FLOATING_TYPES_AND(at::ScalarType::BFloat16, x.scalar_type(),
                                 "bnh_fwd_part", [&] {
    using T = std::conditional_t<std::is_same_v<scalar_t, at::BFloat16>,
                                 __hip_bfloat16, scalar_t>;
    constexpr int VN = BnVec<T>::N;
    TORCH_CHECK(bnh_ok(C, VN), "bn_fwd_train_part: unsupported C=", C);
    const int lgc = bnh_lgc(C, VN);
    const long NI = N * HW, tasks = NI << lgc;
    hipLaunchKernelGGL((bnh_norm_k<T, typename BnVec<T>::V, VN>),
                       dim3(bnh_ew_grid(tasks)), dim3(FT_BLOCK), 0, STREAM,
                       reinterpret_cast<const T*>(x.data_ptr()),
                       reinterpret_cast<T*>(y.data_ptr()),
                       part.data_ptr<float>(), B,
                       weight.numel() ? weight.data_ptr<float>() : nullptr,
                       bias.numel() ? bias.data_ptr<float>() : nullptr,
                       save_mean.data_ptr<float>(),
                       save_ivar.data_ptr<float>(),
                       track ? running_mean.data_ptr<float>() : nullptr,
                       track ? running_var.data_ptr<float>() : nullptr,
                       res.numel()
                           ? reinterpret_cast<const T*>(res.data_ptr())
                           : nullptr,
                       nullptr, NI, C, lgc, (float)eps, (float)momentum,
                       relu ? 1 : 0);
  });
  return {y, save_mean, save_ivar, mask};
}

std::vector<torch::Tensor> bn_fwd_train(torch::Tensor x, torch::Tensor weight,
                                        torch::Tensor bias,
                                        torch::Tensor running_mean,
                                        torch::Tensor running_var,
                                        double eps, double momentum,
                                        bool relu, torch::Tensor res) {
  const char* who = "bn_fwd_train";
  bn_check_x(who, x);
  const bool nhwc =
      x.is_contiguous(at::MemoryFormat::ChannelsLast) && !x.is_contiguous();
  TORCH_CHECK(nhwc || x.is_contiguous(), "bn_fwd_train: x not contiguous");
  long N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  TORCH_CHECK(!nhwc || bnh_ok(C, bn_vn(x)),
              "bn_fwd_train NHWC: unsupported C=", C);
  bn_check_vec(who, "weight", weight, C, true);
  bn_check_vec(who, "bias", bias, C, true);
  bn_check_running(who, running_mean, running_var, C);
  if (conv_present(res)) bn_check_like(who, "res", res, x, nhwc);
  auto f32 = x.options().dtype(torch::kFloat);
  auto save_mean = torch::empty({C}, f32);
  auto save_ivar = torch::empty({C}, f32);
  auto y = torch::empty_like(x);
  auto mask = torch::empty({0}, x.options().dtype(torch::kByte));
  bool track = running_mean.numel() > 0;
  if (nhwc) {
    AT_DISPATCH_FLOATING_TYPES_AND(at::ScalarType::BFloat16, x.scalar_type(),
                                   "bnh_fwd", [&] {
      using T = std::conditional_t<std::is_same_v<scalar_t, at::BFloat16>,
                                   __hip_bfloat16, scalar_t>;
      constexpr int VN = BnVec<T>::N;
      TORCH_CHECK(bnh_ok(C, VN), "bn_fwd_train NHWC: unsupported C=", C);
      const int lgc = bnh_lgc(C, VN);
      const long NI = N * HW, tasks = NI << lgc;
      const int B = bnh_red_grid(tasks);
      auto part = torch::empty({B, C, 2}, f32);
      // measured ~1-2% SLOWER at ResNet-20/b256 (y re-reads are
      // LLC-hot; byte traffic adds overhead) — default off, kept for
      // larger feature maps (profiles/r01_bench_notes.md)
      static const bool use_mask = ft_env_int("FT_BNH_MASK", 0) != 0;
      if (relu && VN == 8 && use_mask)  // bwd reads 1 bit/elem instead of y
        mask = torch::empty({(NI * C) >> 3},
                            x.options().dtype(torch::kByte));
      hipLaunchKernelGGL((bnh_stats_k<T, typename BnVec<T>::V, VN>),
                         dim3(B), dim3(FT_BLOCK), 0, STREAM,
                         reinterpret_cast<const T*>(x.data_ptr()), NI, C,
                         lgc, part.data_ptr<float>());
      hipLaunchKernelGGL((bnh_norm_k<T, typename BnVec<T>::V, VN>),
                         dim3(bnh_ew_grid(tasks)), dim3(FT_BLOCK), 0, STREAM,
                         reinterpret_cast<const T*>(x.data_ptr()),
                         reinterpret_cast<T*>(y.data_ptr()),
                         part.data_ptr<float>(), B,
                         weight.numel() ? weight.data_ptr<float>() : nullptr,
                         bias.numel() ? bias.data_ptr<float>() : nullptr,
                         save_mean.data_ptr<float>(),
                         save_ivar.data_ptr<float>(),
                         track ? running_mean.data_ptr<float>() : nullptr,
                         track ? running_var.data_ptr<float>() : nullptr,
                         res.numel()
                             ? reinterpret_cast<const T*>(res.data_ptr())
                             : nullptr,
                         mask.numel() ? mask.data_ptr<unsigned char>()
                                      : nullptr,
                         NI, C, lgc, (float)eps, (float)momentum,
                         relu ? 1 : 0);
    });
    return {y, save_mean, save_ivar, mask};
  }
  AT_DISPATCH_FLOATING_TYPES_AND(at::ScalarType::BFloat16, x.scalar_type(),
                                 "bn_fwd", [&] {
    using T = std::conditional_t<std::is_same_v<scalar_t, at::BFloat16>,
                                 __hip_bfloat16, scalar_t>;
    const bool vec = (HW % BnVec<T>::N) == 0;
    const int VN = vec ? BnVec<T>::N : 1;
    const long per_v = (N * HW) / VN;
    const int B = bn_nparts(per_v, C);
    auto part = torch::empty({C, B, 2}, f32);
    dim3 rgrid(B, C), egrid(bn_ew_chunks(per_v, C), C);
    auto stats_fn = vec ? bn_stats_k<T, typename BnVec<T>::V, BnVec<T>::N>
                        : bn_stats_k<T, typename Bn1<T>::V, 1>;
    auto norm_fn = vec ? bn_norm_k<T, typename BnVec<T>::V, BnVec<T>::N>
                       : bn_norm_k<T, typename Bn1<T>::V, 1>;
    hipLaunchKernelGGL(stats_fn, rgrid, dim3(FT_BLOCK), 0, STREAM,
                       reinterpret_cast<const T*>(x.data_ptr()), N, C, HW,
                       part.data_ptr<float>());
    hipLaunchKernelGGL(norm_fn, egrid, dim3(FT_BLOCK), 0, STREAM,
                       reinterpret_cast<const T*>(x.data_ptr()),
                       reinterpret_cast<T*>(y.data_ptr()),
                       part.data_ptr<float>(), B,
                       weight.numel() ? weight.data_ptr<float>() : nullptr,
                       bias.numel() ? bias.data_ptr<float>() : nullptr,
                       save_mean.data_ptr<float>(),
                       save_ivar.data_ptr<float>(),
                       track ? running_mean.data_ptr<float>() : nullptr,
                       track ? running_var.data_ptr<float>() : nullptr,
                       res.numel() ? reinterpret_cast<const T*>(res.data_ptr())
                                   : nullptr,
                       N, C, HW, (float)eps, (float)momentum, relu ? 1 : 0);
  });
  return {y, save_mean, save_ivar, mask};
}

// NHWC inference BatchNorm: y = [relu](bn_running(x) [+ res]), one streaming
// launch (batchnorm.h bnh_eval_k); bf16 or fp32, channels_last only.
template <typename T>
static void bn_fwd_eval_launch(const torch::Tensor& x, torch::Tensor& y,
                               const float* gp, const float* bp,
                               const float* mp, const float* vp,
                               const torch::Tensor& res, long NI, long C,
                               float eps, bool relu) {
  constexpr int VN = BnVec<T>::N;
  using V = typename BnVec<T>::V;
  TORCH_CHECK(bnh_ok(C, VN), "bn_fwd_eval: unsupported C=", C);
  const int lgc = bnh_lgc(C, VN);
  const long tasks = NI << lgc;
  const T* xp = reinterpret_cast<const T*>(x.data_ptr());
  T* yp = reinterpret_cast<T*>(y.data_ptr());
  if (res.numel())
    hipLaunchKernelGGL((bnh_eval_k<T, V, VN, true>), dim3(bnh_ew_grid(tasks)),
                       dim3(FT_BLOCK), 0, STREAM, xp, yp, gp, bp, mp, vp,
                       reinterpret_cast<const T*>(res.data_ptr()), NI, C,
                       lgc, eps, relu ? 1 : 0);
  else
    hipLaunchKernelGGL((bnh_eval_k<T, V, VN, false>),
                       dim3(bnh_ew_grid(tasks)), dim3(FT_BLOCK), 0, STREAM,
                       xp, yp, gp, bp, mp, vp, (const T*)nullptr, NI, C, lgc,
                       eps, relu ? 1 : 0);
}

torch::Tensor bn_fwd_eval(torch::Tensor x, torch::Tensor gamma,
                          torch::Tensor beta, torch::Tensor running_mean,
                          torch::Tensor running_var, double eps, bool relu,
                          torch::Tensor res) {
  const char* who = "bn_fwd_eval";
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, who, ": x must be 4D on GPU");
  // (a 1x1 map is channels_last AND plainly contiguous: same memory)
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast), who,
              ": channels_last only");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16 ||
                  x.scalar_type() == torch::kFloat,
              who, ": bf16 or fp32 only");
  const long N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  TORCH_CHECK(N * HW > 0, who, ": empty input");
  const float* gp = conv_check_vec(who, "gamma", gamma, (int)C);
  const float* bp = conv_check_vec(who, "beta", beta, (int)C);
  const float* mp = conv_check_vec(who, "running_mean", running_mean, (int)C);
  const float* vp = conv_check_vec(who, "running_var", running_var, (int)C);
  if (conv_present(res)) {
    TORCH_CHECK(res.is_cuda() && res.scalar_type() == x.scalar_type() &&
                    res.sizes() == x.sizes() &&
                    res.is_contiguous(at::MemoryFormat::ChannelsLast),
                who, ": res must match x (", x.sizes(),
                ", same dtype, channels_last)");
  }
  auto y = torch::empty(
      x.sizes(), x.options().memory_format(at::MemoryFormat::ChannelsLast));
  if (x.scalar_type() == torch::kBFloat16)
    bn_fwd_eval_launch<__hip_bfloat16>(x, y, gp, bp, mp, vp, res, N * HW, C,
                                       (float)eps, relu);
  else
    bn_fwd_eval_launch<float>(x, y, gp, bp, mp, vp, res, N * HW, C,
                              (float)eps, relu);
  return y;
}

std::vector<torch::Tensor> bn_bwd(torch::Tensor dy, torch::Tensor x,
                                  torch::Tensor y, torch::Tensor mask,
                                  torch::Tensor save_mean,
                                  torch::Tensor save_ivar,
                                  torch::Tensor weight, bool relu,
                                  bool has_res) {
  const char* who = "bn_bwd";
  bn_check_x(who, x);
  const bool nhwc =
      x.is_contiguous(at::MemoryFormat::ChannelsLast) && !x.is_contiguous();
  TORCH_CHECK(nhwc || x.is_contiguous(), "bn_bwd: x/dy must be contiguous");
  long N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  TORCH_CHECK(!nhwc || bnh_ok(C, bn_vn(x)), "bn_bwd NHWC: unsupported C=",
              C);
  bn_check_like(who, "dy", dy, x, nhwc);
  bn_check_vec(who, "save_mean", save_mean, C, false);
  bn_check_vec(who, "save_ivar", save_ivar, C, false);
  bn_check_vec(who, "weight", weight, C, true);
  if (conv_present(mask)) {
    // one bit per element over the flat NHWC index, 8 channels per byte:
    // only the bf16 (VN = 8) channels_last kernels index it that way
    TORCH_CHECK(nhwc && x.scalar_type() == torch::kBFloat16,
                "bn_bwd: mask needs channels_last bf16 x");
    TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == torch::kByte &&
                    mask.is_contiguous() && mask.numel() == (N * HW * C) >> 3,
                "bn_bwd: mask must be contiguous uint8 [N*HW*C/8] = [",
                (N * HW * C) >> 3, "] on GPU");
  }
  TORCH_CHECK(!relu || conv_present(mask) || conv_present(y),
              "bn_bwd: relu needs y/mask");
  if (relu && conv_present(y)) bn_check_like(who, "y", y, x, nhwc);
  auto f32 = x.options().dtype(torch::kFloat);
  auto dx = torch::empty_like(x);
  auto dres = has_res ? torch::empty_like(x)
                      : torch::empty({0}, x.options());
  auto dweight = torch::empty({C}, f32);
  auto dbias = torch::empty({C}, f32);
  if (nhwc) {
    TORCH_CHECK(dy.is_contiguous(at::MemoryFormat::ChannelsLast),
                "bn_bwd NHWC: dy must be channels_last");
    AT_DISPATCH_FLOATING_TYPES_AND(at::ScalarType::BFloat16, x.scalar_type(),
                                   "bnh_bwd", [&] {
      using T = std::conditional_t<std::is_same_v<scalar_t, at::BFloat16>,
                                   __hip_bfloat16, scalar_t>;
      constexpr int VN = BnVec<T>::N;
      TORCH_CHECK(bnh_ok(C, VN), "bn_bwd NHWC: unsupported C=", C);
      const int lgc = bnh_lgc(C, VN);
      const long NI = N * HW, tasks = NI << lgc;
      const int B = bnh_red_grid(tasks);
      auto part = torch::empty({B, C, 2}, f32);
      const unsigned char* mp =
          mask.numel() ? mask.data_ptr<unsigned char>() : nullptr;
      const T* yp = (relu && !mp)
                        ? reinterpret_cast<const T*>(y.data_ptr())
                        : nullptr;
      TORCH_CHECK(!relu || mp || y.numel(), "bn_bwd NHWC: relu needs y/mask");
      hipLaunchKernelGGL((bnh_bwd_stats_k<T, typename BnVec<T>::V, VN>),
                         dim3(B), dim3(FT_BLOCK), 0, STREAM,
                         reinterpret_cast<const T*>(dy.data_ptr()),
                         reinterpret_cast<const T*>(x.data_ptr()), yp, mp,
                         save_mean.data_ptr<float>(),
                         save_ivar.data_ptr<float>(), NI, C, lgc,
                         part.data_ptr<float>(), relu ? 1 : 0);
      hipLaunchKernelGGL((bnh_bwd_dx_k<T, typename BnVec<T>::V, VN>),
                         dim3(bnh_ew_grid(tasks)), dim3(FT_BLOCK), 0, STREAM,
                         reinterpret_cast<const T*>(dy.data_ptr()),
                         reinterpret_cast<const T*>(x.data_ptr()), yp, mp,
                         part.data_ptr<float>(), B,
                         save_mean.data_ptr<float>(),
                         save_ivar.data_ptr<float>(),
                         weight.numel() ? weight.data_ptr<float>() : nullptr,
                         reinterpret_cast<T*>(dx.data_ptr()),
                         has_res ? reinterpret_cast<T*>(dres.data_ptr())
                                 : nullptr,
                         dweight.data_ptr<float>(), dbias.data_ptr<float>(),
                         NI, C, lgc, relu ? 1 : 0);
    });
    return {dx, dweight, dbias, dres};
  }
  TORCH_CHECK(x.is_contiguous() && dy.is_contiguous(),
              "bn_bwd: x/dy must be contiguous");
  AT_DISPATCH_FLOATING_TYPES_AND(at::ScalarType::BFloat16, x.scalar_type(),
                                 "bn_bwd", [&] {
    using T = std::conditional_t<std::is_same_v<scalar_t, at::BFloat16>,
                                 __hip_bfloat16, scalar_t>;
    const T* yp = relu ? reinterpret_cast<const T*>(y.data_ptr()) : nullptr;
    const bool vec = (HW % BnVec<T>::N) == 0;
    const int VN = vec ? BnVec<T>::N : 1;
    const long per_v = (N * HW) / VN;
    const int B = bn_nparts(per_v, C);
    auto part = torch::empty({C, B, 2}, f32);
    dim3 rgrid(B, C), egrid(bn_ew_chunks(per_v, C), C);
    auto stats_fn = vec ? bn_bwd_stats_k<T, typename BnVec<T>::V, BnVec<T>::N>
                        : bn_bwd_stats_k<T, typename Bn1<T>::V, 1>;
    auto dx_fn = vec ? bn_bwd_dx_k<T, typename BnVec<T>::V, BnVec<T>::N>
                     : bn_bwd_dx_k<T, typename Bn1<T>::V, 1>;
    hipLaunchKernelGGL(stats_fn, rgrid, dim3(FT_BLOCK), 0,
                       STREAM, reinterpret_cast<const T*>(dy.data_ptr()),
                       reinterpret_cast<const T*>(x.data_ptr()), yp,
                       save_mean.data_ptr<float>(),
                       save_ivar.data_ptr<float>(), N, C, HW,
                       part.data_ptr<float>(), relu ? 1 : 0);
    hipLaunchKernelGGL(dx_fn, egrid, dim3(FT_BLOCK), 0, STREAM,
                       reinterpret_cast<const T*>(dy.data_ptr()),
                       reinterpret_cast<const T*>(x.data_ptr()), yp,
                       part.data_ptr<float>(), B, save_mean.data_ptr<float>(),
                       save_ivar.data_ptr<float>(),
                       weight.numel() ? weight.data_ptr<float>() : nullptr,
                       reinterpret_cast<T*>(dx.data_ptr()),
                       has_res ? reinterpret_cast<T*>(dres.data_ptr())
                               : nullptr,
                       dweight.data_ptr<float>(), dbias.data_ptr<float>(),
                       N, C, HW, relu ? 1 : 0);
  });
  return {dx, dweight, dbias, dres};
}

// deferred BN backward: stats + per-channel affine coefs (+ optional
// dres); the elementwise dx pass moves into the consuming conv's staging
std::vector<torch::Tensor> bn_bwd_defer(
    torch::Tensor dz, torch::Tensor x, torch::Tensor z,
    torch::Tensor save_mean, torch::Tensor save_ivar, torch::Tensor weight,
    bool relu, bool has_res) {
  const char* who = "bn_bwd_defer";
  bn_check_x(who, x);
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "bn_bwd_defer: channels_last GPU");
  long N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  TORCH_CHECK(bnh_ok(C, bn_vn(x)), "bn_bwd_defer: unsupported C=", C);
  bn_check_like(who, "dz", dz, x, true);
  // the dres kernel masks by z unconditionally
  TORCH_CHECK(relu || !has_res, "bn_bwd_defer: has_res needs relu");
  if (relu) bn_check_like(who, "z", z, x, true);
  bn_check_vec(who, "save_mean", save_mean, C, false);
  bn_check_vec(who, "save_ivar", save_ivar, C, false);
  bn_check_vec(who, "weight", weight, C, true);
  TORCH_CHECK(!has_res || N * HW * C / bn_vn(x) < (1L << 31),
              "bn_bwd_defer: N*HW*C too large for the dres pass");
  auto f32 = x.options().dtype(torch::kFloat);
  auto coefs = torch::empty({3, C}, f32);
  auto dweight = torch::empty({C}, f32);
  auto dbias = torch::empty({C}, f32);
  auto dres = has_res ? torch::empty_like(x)
                      : torch::empty({0}, x.options());
  AT_DISPATCH_FLOATING_TYPES_AND(at::ScalarType::BFloat16, x.scalar_type(),
                                 "bnh_bwd_defer", [&] {
    using T = std::conditional_t<std::is_same_v<scalar_t, at::BFloat16>,
                                 __hip_bfloat16, scalar_t>;
    constexpr int VN = BnVec<T>::N;
    TORCH_CHECK(bnh_ok(C, VN), "bn_bwd_defer: unsupported C=", C);
    const int lgc = bnh_lgc(C, VN);
    const long NI = N * HW, tasks = NI << lgc;
    const int B = bnh_red_grid(tasks);
    auto part = torch::empty({B, C, 2}, f32);
    const T* yp = relu ? reinterpret_cast<const T*>(z.data_ptr()) : nullptr;
    hipLaunchKernelGGL((bnh_bwd_stats_k<T, typename BnVec<T>::V, VN>),
                       dim3(B), dim3(FT_BLOCK), 0, STREAM,
                       reinterpret_cast<const T*>(dz.data_ptr()),
                       reinterpret_cast<const T*>(x.data_ptr()), yp,
                       nullptr, save_mean.data_ptr<float>(),
                       save_ivar.data_ptr<float>(), NI, C, lgc,
                       part.data_ptr<float>(), relu ? 1 : 0);
    torch::Tensor red = part;
    int Bred = B;
    if (B > 64) {
      // collapse partials first: the 1-block coef kernel over ~1000 rows
      // is a serial latency chain (measured 5.9 us/call, ~98 us/step)
      const int B2 = 32;
      red = torch::empty({B2, C, 2}, f32);
      hipLaunchKernelGGL(part_reduce_k, dim3(B2), dim3(FT_BLOCK), 0,
                         STREAM, part.data_ptr<float>(), B, (int)(C * 2),
                         red.data_ptr<float>(), B2);
      Bred = B2;
    }
    hipLaunchKernelGGL(bnh_bwd_coef_k, dim3(1), dim3(FT_BLOCK), 0, STREAM,
                       red.data_ptr<float>(), Bred, NI,
                       save_mean.data_ptr<float>(),
                       save_ivar.data_ptr<float>(),
                       weight.numel() ? weight.data_ptr<float>() : nullptr,
                       C, coefs.data_ptr<float>(),
                       dweight.data_ptr<float>(), dbias.data_ptr<float>());
    if (has_res) {
      const long total_v = NI * C / VN;
      hipLaunchKernelGGL((bnh_mask_dres_k<T, typename BnVec<T>::V, VN>),
                         dim3(ft_grid(total_v)), dim3(FT_BLOCK), 0, STREAM,
                         reinterpret_cast<const T*>(dz.data_ptr()),
                         reinterpret_cast<const T*>(z.data_ptr()),
                         reinterpret_cast<T*>(dres.data_ptr()), total_v);
    }
  });
  return {coefs, dweight, dbias, dres};
}

// ==========================================================================
// classifier tail (head.h): pool + FC head fwd/bwd, loss / top-k accumulator
// ==========================================================================
static inline bool head_is_float(const torch::Tensor& t) {
  return t.scalar_type() == torch::kBFloat16 ||
         t.scalar_type() == torch::kFloat;
}
static inline bool head_aligned16(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// weight [K, C] and bias [K] / empty of the FC layer, any bf16/fp32 mix
static void head_check_fc(const char* who, const torch::Tensor& weight,
                          const torch::Tensor& bias, long C,
                          const torch::Device& dev) {
  TORCH_CHECK(weight.is_cuda() && weight.device() == dev, who,
              ": weight must be on x's GPU");
  TORCH_CHECK(weight.dim() == 2 && weight.is_contiguous(), who,
              ": weight must be contiguous [K, C]");
  TORCH_CHECK(head_is_float(weight), who, ": weight must be bf16 or fp32");
  TORCH_CHECK(weight.size(1) == C, who, ": weight is ", weight.sizes(),
              ", expected [K, ", C, "]");
  const long K = weight.size(0);
  TORCH_CHECK(C % 8 == 0 && C >= 8 && C <= HEAD_MAXC, who,
              ": unsupported C=", C, " (C % 8 == 0, 8 <= C <= 1024)");
  TORCH_CHECK(K >= 1 && K <= HEAD_MAXK, who, ": unsupported K=", K,
              " (1 <= K <= 1024)");
  TORCH_CHECK(head_aligned16(weight), who, ": weight must be 16-byte aligned");
  if (bias.numel()) {
    TORCH_CHECK(bias.is_cuda() && bias.device() == dev, who,
                ": bias must be on x's GPU");
    TORCH_CHECK(head_is_float(bias), who, ": bias must be bf16 or fp32");
    TORCH_CHECK(bias.dim() == 1 && bias.numel() == K && bias.is_contiguous(),
                who, ": bias must be contiguous [K] = [", K, "] or empty");
  }
}

std::vector<torch::Tensor> head_fwd(torch::Tensor x, torch::Tensor weight,
                                    torch::Tensor bias) {
  const char* who = "head_fwd";
  TORCH_CHECK(x.is_cuda() && x.dim() == 4, who, ": x must be 4D on GPU");
  TORCH_CHECK(x.is_contiguous(at::MemoryFormat::ChannelsLast), who,
              ": channels_last only");
  TORCH_CHECK(head_is_float(x), who, ": x must be bf16 or fp32");
  const long N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  TORCH_CHECK(N >= 1 && HW >= 1, who, ": empty input");
  TORCH_CHECK(N < (1L << 31) && HW * C < (1L << 31), who,
              ": input too large");
  head_check_fc(who, weight, bias, C, x.device());
  TORCH_CHECK(head_aligned16(x), who, ": x must be 16-byte aligned");
  const long K = weight.size(0);
  auto fopt = x.options().dtype(torch::kFloat).memory_format(
      at::MemoryFormat::Contiguous);
  auto logits = torch::empty({N, K}, fopt);
  auto pooled = torch::empty({N, C}, fopt);
  const void* bp = bias.numel() ? bias.data_ptr() : nullptr;
  const int bbf = bias.numel() && bias.scalar_type() == torch::kBFloat16;
  const bool xb = x.scalar_type() == torch::kBFloat16;
  const bool wb = weight.scalar_type() == torch::kBFloat16;
#define HEAD_FWD_LAUNCH(TX, TW)                                              \
  hipLaunchKernelGGL((head_fwd_k<TX, TW>), dim3((unsigned)N),                \
                     dim3(FT_BLOCK), 0, STREAM,                              \
                     reinterpret_cast<const TX*>(x.data_ptr()),              \
                     reinterpret_cast<const TW*>(weight.data_ptr()), bp,     \
                     bbf, logits.data_ptr<float>(),                          \
                     pooled.data_ptr<float>(), (int)C, (int)HW, (int)K)
  if (xb && wb) HEAD_FWD_LAUNCH(__hip_bfloat16, __hip_bfloat16);
  else if (xb) HEAD_FWD_LAUNCH(__hip_bfloat16, float);
  else if (wb) HEAD_FWD_LAUNCH(float, __hip_bfloat16);
  else HEAD_FWD_LAUNCH(float, float);
#undef HEAD_FWD_LAUNCH
  return {logits, pooled};
}

// returns {dx, dw, db}; dx is undefined (None) without need_dx, db without
// a bias.  dw / db are fresh contiguous tensors in the parameters' dtypes.
std::vector<torch::Tensor> head_bwd(torch::Tensor dlogits,
                                    torch::Tensor pooled,
                                    torch::Tensor weight, torch::Tensor bias,
                                    long H, long W, bool x_is_bf16,
                                    bool need_dx) {
  const char* who = "head_bwd";
  TORCH_CHECK(pooled.is_cuda() && pooled.dim() == 2 &&
                  pooled.scalar_type() == torch::kFloat &&
                  pooled.is_contiguous(),
              who, ": pooled must be contiguous fp32 [N, C] on GPU");
  const long N = pooled.size(0), C = pooled.size(1), HW = H * W;
  TORCH_CHECK(N >= 1 && H >= 1 && W >= 1, who, ": empty input");
  TORCH_CHECK(N < (1L << 31) && HW * C < (1L << 31), who,
              ": input too large");
  head_check_fc(who, weight, bias, C, pooled.device());
  const long K = weight.size(0);
  TORCH_CHECK(dlogits.is_cuda() && dlogits.device() == pooled.device() &&
                  dlogits.scalar_type() == torch::kFloat &&
                  dlogits.dim() == 2 && dlogits.size(0) == N &&
                  dlogits.size(1) == K && dlogits.is_contiguous(),
              who, ": dlogits must be contiguous fp32 [N, K] = [", N, ", ", K,
              "] on pooled's GPU");
  const bool wb = weight.scalar_type() == torch::kBFloat16;
  torch::Tensor dx, db;
  auto dw = torch::empty({K, C}, weight.options().memory_format(
                                     at::MemoryFormat::Contiguous));
  if (bias.numel())
    db = torch::empty({K}, bias.options().memory_format(
                               at::MemoryFormat::Contiguous));
  if (need_dx) {
    dx = torch::empty(
        {N, C, H, W},
        pooled.options()
            .dtype(x_is_bf16 ? torch::kBFloat16 : torch::kFloat)
            .memory_format(at::MemoryFormat::ChannelsLast));
#define HEAD_DX_LAUNCH(TX, TW)                                               \
  hipLaunchKernelGGL((head_dx_k<TX, TW>), dim3((unsigned)N), dim3(FT_BLOCK), \
                     0, STREAM, dlogits.data_ptr<float>(),                   \
                     reinterpret_cast<const TW*>(weight.data_ptr()),         \
                     reinterpret_cast<TX*>(dx.data_ptr()), (int)C, (int)HW,  \
                     (int)K)
    if (x_is_bf16 && wb) HEAD_DX_LAUNCH(__hip_bfloat16, __hip_bfloat16);
    else if (x_is_bf16) HEAD_DX_LAUNCH(__hip_bfloat16, float);
    else if (wb) HEAD_DX_LAUNCH(float, __hip_bfloat16);
    else HEAD_DX_LAUNCH(float, float);
#undef HEAD_DX_LAUNCH
  }
  hipLaunchKernelGGL(head_dwdb_k, dim3((unsigned)((C + WAVE - 1) / WAVE),
                                       (unsigned)K),
                     dim3(FT_BLOCK), 0, STREAM, dlogits.data_ptr<float>(),
                     pooled.data_ptr<float>(), dw.data_ptr(), wb ? 1 : 0,
                     db.defined() ? db.data_ptr() : nullptr,
                     db.defined() && db.scalar_type() == torch::kBFloat16,
                     (int)N, (int)C, (int)K);
  return {dx, dw, db};
}

// acc (fp64 [4] on the GPU) += (loss_sum, top1_count, top5_count, n) of the
// batch; one launch, one workgroup, no host synchronisation.
void ce_topk_accum(torch::Tensor logits, torch::Tensor target,
                   torch::Tensor acc) {
  const char* who = "ce_topk_accum";
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.is_contiguous(),
              who, ": logits must be contiguous [N, K] on GPU");
  TORCH_CHECK(head_is_float(logits), who, ": logits must be bf16 or fp32");
  const long N = logits.size(0), K = logits.size(1);
  TORCH_CHECK(K >= 1 && K <= HEAD_MAXK, who, ": unsupported K=", K,
              " (1 <= K <= 1024)");
  TORCH_CHECK(N < (1L << 31), who, ": batch too large");
  TORCH_CHECK(target.is_cuda() && target.device() == logits.device() &&
                  target.scalar_type() == torch::kLong &&
                  target.dim() == 1 && target.size(0) == N &&
                  target.is_contiguous(),
              who, ": target must be contiguous int64 [N] = [", N,
              "] on logits' GPU");
  TORCH_CHECK(acc.is_cuda() && acc.device() == logits.device() &&
                  acc.scalar_type() == torch::kDouble && acc.dim() == 1 &&
                  acc.numel() == 4 && acc.is_contiguous(),
              who, ": acc must be contiguous float64 [4] on logits' GPU");
  if (N == 0) return;
  if (logits.scalar_type() == torch::kBFloat16)
    hipLaunchKernelGGL(ce_topk_k<__hip_bfloat16>, dim3(1),
                       dim3(HEAD_CE_BLOCK), 0, STREAM,
                       reinterpret_cast<const __hip_bfloat16*>(
                           logits.data_ptr()),
                       target.data_ptr<long>(), acc.data_ptr<double>(),
                       (int)N, (int)K);
  else
    hipLaunchKernelGGL(ce_topk_k<float>, dim3(1), dim3(HEAD_CE_BLOCK), 0,
                       STREAM, logits.data_ptr<float>(),
                       target.data_ptr<long>(), acc.data_ptr<double>(),
                       (int)N, (int)K);
}

// ==========================================================================
// persistent GRU sequence kernels (gru.h)
// ==========================================================================
// fp32 contiguous tensor of the given shape on `dev`
static void gru_check_f32(const char* who, const char* name,
                          const torch::Tensor& t, at::IntArrayRef shape,
                          const torch::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev, who, ": ", name,
              " must be on gx's GPU");
  TORCH_CHECK(t.scalar_type() == torch::kFloat, who, ": ", name,
              " must be fp32");
  TORCH_CHECK(t.sizes() == shape && t.is_contiguous(), who, ": ", name,
              " must be contiguous ", shape, ", got ", t.sizes());
}
// bf16 / fp32 contiguous parameter of the given shape on `dev`
static void gru_check_param(const char* who, const char* name,
                            const torch::Tensor& t, at::IntArrayRef shape,
                            const torch::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev, who, ": ", name,
              " must be on gx's GPU");
  TORCH_CHECK(head_is_float(t), who, ": ", name, " must be bf16 or fp32");
  TORCH_CHECK(t.sizes() == shape && t.is_contiguous(), who, ": ", name,
              " must be contiguous ", shape, ", got ", t.sizes());
}
static void gru_check_dims(const char* who, long B, long T, long H) {
  TORCH_CHECK(H >= 1 && H <= GRU_MAXH, who, ": unsupported H=", H,
              " (1 <= H <= 64)");
  TORCH_CHECK(B >= 1 && T >= 1, who, ": empty input");
  TORCH_CHECK(B < (1L << 31) && T < (1L << 31) &&
                  B * T < (1L << 40), who, ": input too large");
}

// returns {out [B,T,H], gates [B,T,4,H] = (r,z,n,q)}; gates is an empty
// tensor without save_gates
std::vector<torch::Tensor> gru_fwd(torch::Tensor gx, torch::Tensor w_hh,
                                   torch::Tensor b_hh, torch::Tensor h0,
                                   bool save_gates) {
  const char* who = "gru_fwd";
  TORCH_CHECK(gx.is_cuda() && gx.dim() == 3 && gx.is_contiguous(), who,
              ": gx must be contiguous [B, T, 3H] on GPU");
  TORCH_CHECK(gx.scalar_type() == torch::kFloat, who, ": gx must be fp32");
  TORCH_CHECK(gx.size(2) % 3 == 0, who, ": gx is ", gx.sizes(),
              ", expected [B, T, 3H]");
  const long B = gx.size(0), T = gx.size(1), H = gx.size(2) / 3;
  gru_check_dims(who, B, T, H);
  const auto dev = gx.device();
  gru_check_param(who, "w_hh", w_hh, {3 * H, H}, dev);
  gru_check_param(who, "b_hh", b_hh, {3 * H}, dev);
  gru_check_f32(who, "h0", h0, {B, H}, dev);
  auto out = torch::empty({B, T, H}, gx.options());
  auto gates = save_gates ? torch::empty({B, T, 4, H}, gx.options())
                          : torch::empty({0}, gx.options());
  const int wbf = w_hh.scalar_type() == torch::kBFloat16;
  const int bbf = b_hh.scalar_type() == torch::kBFloat16;
  const unsigned grid = (unsigned)((B + GRU_ROWS - 1) / GRU_ROWS);
#define GRU_FWD_LAUNCH(NT)                                                   \
  hipLaunchKernelGGL(gru_fwd_k<NT>, dim3(grid), dim3(NT * WAVE), 0, STREAM,  \
                     gx.data_ptr<float>(), w_hh.data_ptr(), wbf,             \
                     b_hh.data_ptr(), bbf, h0.data_ptr<float>(),             \
                     out.data_ptr<float>(),                                  \
                     save_gates ? gates.data_ptr<float>() : nullptr, (int)B, \
                     (int)T, (int)H)
  switch ((H + 15) / 16) {
    case 1: GRU_FWD_LAUNCH(1); break;
    case 2: GRU_FWD_LAUNCH(2); break;
    case 3: GRU_FWD_LAUNCH(3); break;
    default: GRU_FWD_LAUNCH(4); break;
  }
#undef GRU_FWD_LAUNCH
  return {out, gates};
}

// returns {dgx [B,T,3H], dgh [B,T,3H], dh0 [B,H]}
std::vector<torch::Tensor> gru_bwd(torch::Tensor dout, torch::Tensor out,
                                   torch::Tensor gates, torch::Tensor w_hh,
                                   torch::Tensor h0) {
  const char* who = "gru_bwd";
  TORCH_CHECK(out.is_cuda() && out.dim() == 3 && out.is_contiguous(), who,
              ": out must be contiguous [B, T, H] on GPU");
  TORCH_CHECK(out.scalar_type() == torch::kFloat, who, ": out must be fp32");
  const long B = out.size(0), T = out.size(1), H = out.size(2);
  gru_check_dims(who, B, T, H);
  const auto dev = out.device();
  gru_check_f32(who, "dout", dout, {B, T, H}, dev);
  gru_check_f32(who, "gates", gates, {B, T, 4, H}, dev);
  gru_check_param(who, "w_hh", w_hh, {3 * H, H}, dev);
  gru_check_f32(who, "h0", h0, {B, H}, dev);
  auto dgx = torch::empty({B, T, 3 * H}, out.options());
  auto dgh = torch::empty({B, T, 3 * H}, out.options());
  auto dh0 = torch::empty({B, H}, out.options());
  const int wbf = w_hh.scalar_type() == torch::kBFloat16;
  const unsigned grid = (unsigned)((B + GRU_ROWS - 1) / GRU_ROWS);
#define GRU_BWD_LAUNCH(NT)                                                   \
  hipLaunchKernelGGL(gru_bwd_k<NT>, dim3(grid), dim3(NT * WAVE), 0, STREAM,  \
                     dout.data_ptr<float>(), out.data_ptr<float>(),          \
                     gates.data_ptr<float>(), w_hh.data_ptr(), wbf,          \
                     h0.data_ptr<float>(), dgx.data_ptr<float>(),            \
                     dgh.data_ptr<float>(), dh0.data_ptr<float>(), (int)B,   \
                     (int)T, (int)H)
  switch ((H + 15) / 16) {
    case 1: GRU_BWD_LAUNCH(1); break;
    case 2: GRU_BWD_LAUNCH(2); break;
    case 3: GRU_BWD_LAUNCH(3); break;
    default: GRU_BWD_LAUNCH(4); break;
  }
#undef GRU_BWD_LAUNCH
  return {dgx, dgh, dh0};
}

// ==========================================================================
// packed linear models: all clients' local steps in one launch
// (linearround.h)
// ==========================================================================
// LDS floats one client needs: resident state plus the per-step scratch
static long linround_lds_need(long F, long K, long B, bool uses_momentum) {
  return (uses_momentum ? 2 : 1) * (F + 1) * (K | 1) + B * (K + 2);
}
// the LDS floats left for one client's resident image, (F + 1) * (K | 1);
// the B * (K + 2) floats of step scratch come off the same budget
long linear_round_max_floats(bool uses_momentum) {
  return LINROUND_LDS_FLOATS / (uses_momentum ? 2 : 1);
}
long linear_round_lds_floats(long F, long K, long B, bool uses_momentum) {
  return linround_lds_need(F, K, B, uses_momentum);
}

static void linround_check(const char* who, const char* name,
                           const torch::Tensor& t, at::ScalarType st,
                           at::IntArrayRef shape, const torch::Device& dev) {
  TORCH_CHECK(t.is_cuda() && t.device() == dev, who, ": ", name,
              " must be on X's GPU");
  TORCH_CHECK(t.scalar_type() == st, who, ": ", name, " must be ", st,
              ", got ", t.scalar_type());
  TORCH_CHECK(t.sizes() == shape && t.is_contiguous(), who, ": ", name,
              " must be contiguous ", shape, ", got ", t.sizes());
}

// returns loss [C, T]; writes replicas / in_mom / mom_init / snap rows of the
// clients with steps > 0.  idx is range-checked on the host unless the
// stream is capturing (the kernel itself never reads X outside [0, M)).
torch::Tensor linear_local_rounds(
    torch::Tensor X, torch::Tensor Y, torch::Tensor idx, torch::Tensor steps,
    torch::Tensor lr, torch::Tensor server, torch::Tensor replicas,
    torch::Tensor in_mom, torch::Tensor mom_init, torch::Tensor snap,
    long k_cut, long w_off, long b_off, long K, long loss_kind,
    double weight_decay, double momentum, double dampening, bool nesterov,
    torch::Tensor delta, torch::Tensor ctrl_server, torch::Tensor ctrl_client,
    double prox_mu) {
  const char* who = "linear_local_rounds";
  TORCH_CHECK(X.is_cuda() && X.dim() == 2 && X.is_contiguous(), who,
              ": X must be contiguous [M, F] on GPU");
  TORCH_CHECK(X.scalar_type() == torch::kFloat, who, ": X must be fp32");
  const long M = X.size(0), F = X.size(1);
  const auto dev = X.device();
  TORCH_CHECK(M >= 1 && F >= 1, who, ": empty X");
  TORCH_CHECK(M < (1L << 31) && F < (1L << 31), who, ": X too large");
  TORCH_CHECK(server.dim() == 1 && server.size(0) < (1L << 30), who,
              ": server must be [N], N < 2^30");
  TORCH_CHECK(K >= 1 && K <= LINROUND_MAXK, who, ": unsupported K=", K,
              " (1 <= K <= 16)");
  TORCH_CHECK(loss_kind == 0 || loss_kind == 1, who, ": loss_kind is ",
              loss_kind, ", expected 0 (softmax-CE) or 1 (MSE)");
  TORCH_CHECK(loss_kind == 0 || K == 1, who, ": MSE needs K == 1, got ", K);
  linround_check(who, "Y", Y, loss_kind == 0 ? torch::kInt : torch::kFloat,
                 {M}, dev);
  TORCH_CHECK(idx.dim() == 3, who, ": idx must be [C, T, B], got ",
              idx.sizes());
  const long C = idx.size(0), T = idx.size(1), B = idx.size(2);
  TORCH_CHECK(C >= 1 && T >= 1 && B >= 1, who, ": empty idx");
  TORCH_CHECK(C < (1L << 31) && T < (1L << 31) && B < (1L << 31), who,
              ": idx too large");
  linround_check(who, "idx", idx, torch::kInt, {C, T, B}, dev);
  linround_check(who, "steps", steps, torch::kInt, {C}, dev);
  linround_check(who, "lr", lr, torch::kFloat, {C, T}, dev);
  const long N = server.size(0);
  linround_check(who, "server", server, torch::kFloat, {N}, dev);
  linround_check(who, "replicas", replicas, torch::kFloat, {C, N}, dev);
  linround_check(who, "mom_init", mom_init, torch::kInt, {C}, dev);
  const bool use_mom = momentum != 0.0;
  if (use_mom)
    linround_check(who, "in_mom", in_mom, torch::kFloat, {C, N}, dev);
  const bool has_snap = snap.numel() != 0;
  if (has_snap) linround_check(who, "snap", snap, torch::kFloat, {C, N}, dev);
  // the gradient correction of the round (an empty tensor: none)
  const bool has_delta = delta.numel() != 0;
  const bool has_cs = ctrl_server.numel() != 0;
  const bool has_cc = ctrl_client.numel() != 0;
  TORCH_CHECK(has_cs == has_cc, who, ": ctrl_server and ctrl_client come as "
              "a pair, got only ", has_cs ? "ctrl_server" : "ctrl_client");
  TORCH_CHECK(!(has_delta && has_cs), who, ": delta and a control pair "
              "together are not supported (one correction vector per "
              "client)");
  if (has_delta)
    linround_check(who, "delta", delta, torch::kFloat, {C, N}, dev);
  if (has_cs) {
    linround_check(who, "ctrl_server", ctrl_server, torch::kFloat, {N}, dev);
    linround_check(who, "ctrl_client", ctrl_client, torch::kFloat, {C, N},
                   dev);
  }
  TORCH_CHECK(std::isfinite(prox_mu), who, ": prox_mu is not finite");
  TORCH_CHECK(w_off >= 0 && b_off >= 0 && w_off + K * F <= N &&
                  b_off + K <= N &&
                  (w_off + K * F <= b_off || b_off + K <= w_off),
              who, ": weight [", w_off, ", +", K * F, ") / bias [", b_off,
              ", +", K, ") do not fit the arena of ", N);
  TORCH_CHECK(!nesterov || (use_mom && dampening == 0.0), who,
              ": nesterov needs a momentum and zero dampening");
  const long need = linround_lds_need(F, K, B, use_mom);
  TORCH_CHECK(need <= LINROUND_LDS_FLOATS, who, ": F=", F, " K=", K, " B=", B,
              use_mom ? " with" : " without", " momentum needs ", need,
              " floats of LDS, the limit is ", (long)LINROUND_LDS_FLOATS);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  TORCH_CHECK(hipStreamIsCapturing(STREAM, &cap) == hipSuccess, who,
              ": hipStreamIsCapturing failed");
  if (cap == hipStreamCaptureStatusNone) {
    const long top = idx.max().item<int>();
    TORCH_CHECK(top < M, who, ": idx holds row ", top, " but X has ", M,
                " rows");
    const long most = steps.max().item<int>();
    TORCH_CHECK(most <= T, who, ": steps holds ", most, " but idx has T=", T);
  }

  auto loss = torch::zeros({C, T}, X.options());
  LinRoundArgs a;
  a.X = X.data_ptr<float>();
  a.Y = Y.data_ptr();
  a.idx = idx.data_ptr<int>();
  a.steps = steps.data_ptr<int>();
  a.lr = lr.data_ptr<float>();
  a.server = server.data_ptr<float>();
  a.replicas = replicas.data_ptr<float>();
  a.in_mom = use_mom ? in_mom.data_ptr<float>() : nullptr;
  a.mom_init = mom_init.data_ptr<int>();
  a.snap = has_snap ? snap.data_ptr<float>() : nullptr;
  a.loss = loss.data_ptr<float>();
  a.M = (int)M; a.F = (int)F; a.B = (int)B; a.T = (int)T;
  a.N = (int)N; a.w_off = (int)w_off; a.b_off = (int)b_off;
  a.k_cut = (int)std::min<long>(std::max<long>(k_cut, 0), 1L << 30);
  a.use_mom = use_mom; a.nesterov = nesterov;
  a.wd = (float)weight_decay; a.mom = (float)momentum;
  a.omd = (float)(1.0 - dampening);
  a.corr_rows = has_delta ? delta.data_ptr<float>()
                : has_cs  ? ctrl_client.data_ptr<float>()
                          : nullptr;
  a.ctrl_s = has_cs ? ctrl_server.data_ptr<float>() : nullptr;
  a.prox_mu = (float)prox_mu;
  a.corr = (has_delta ? LINROUND_DELTA : 0) | (has_cs ? LINROUND_CTRL : 0) |
           (prox_mu != 0.0 ? LINROUND_PROX : 0);
#define LINROUND_LAUNCH(KK, LOSS)                                            \
  hipLaunchKernelGGL((linear_round_k<KK, LOSS>), dim3((unsigned)C),          \
                     dim3(LINROUND_THREADS), 0, STREAM, a)
#define LINROUND_CASE(KK) case KK: LINROUND_LAUNCH(KK, 0); break
  if (loss_kind == 1) {
    LINROUND_LAUNCH(1, 1);
  } else {
    switch (K) {
      LINROUND_CASE(1); LINROUND_CASE(2); LINROUND_CASE(3); LINROUND_CASE(4);
      LINROUND_CASE(5); LINROUND_CASE(6); LINROUND_CASE(7); LINROUND_CASE(8);
      LINROUND_CASE(9); LINROUND_CASE(10); LINROUND_CASE(11);
      LINROUND_CASE(12); LINROUND_CASE(13); LINROUND_CASE(14);
      LINROUND_CASE(15); LINROUND_CASE(16);
    }
  }
#undef LINROUND_CASE
#undef LINROUND_LAUNCH
  return loss;
}

// ==========================================================================
// packed MLP: all clients' local steps batched per layer (mlpround.h)
// ==========================================================================
long mlp_round_max_batch() { return MLPROUND_MAXB; }
long mlp_round_max_classes() { return MLPROUND_MAXK; }
long mlp_round_max_layers() { return MLPROUND_MAXL; }

// layout: [L, (w, b, gamma, beta, in, out) x L, fc, H, K] -- arena offsets
// and shapes of the blocks and of the head.  Returns loss [C, T]; writes
// replicas / in_mom / mom_init / snap rows of the clients with steps > 0.
// idx and steps are range-checked on the host unless the stream is
// capturing (the kernels never read X outside [0, M)).
torch::Tensor mlp_local_rounds(
    torch::Tensor X, torch::Tensor Y, torch::Tensor idx, torch::Tensor steps,
    torch::Tensor lr, torch::Tensor server, torch::Tensor replicas,
    torch::Tensor in_mom, torch::Tensor mom_init, torch::Tensor snap,
    long k_cut, std::vector<int64_t> layout, double eps, long wd_numel,
    double weight_decay, double momentum, double dampening, bool nesterov,
    torch::Tensor delta, torch::Tensor ctrl_server, torch::Tensor ctrl_client,
    double prox_mu) {
  const char* who = "mlp_local_rounds";
  TORCH_CHECK(X.is_cuda() && X.dim() == 2 && X.is_contiguous(), who,
              ": X must be contiguous [M, F] on GPU");
  TORCH_CHECK(X.scalar_type() == torch::kFloat, who, ": X must be fp32");
  const long M = X.size(0), F = X.size(1);
  const auto dev = X.device();
  TORCH_CHECK(M >= 1 && F >= 1, who, ": empty X");
  TORCH_CHECK(M < (1L << 31) && F < (1L << 21), who, ": X too large");
  TORCH_CHECK(server.dim() == 1 && server.size(0) < (1L << 30), who,
              ": server must be [N], N < 2^30");
  const long N = server.size(0);
  linround_check(who, "Y", Y, torch::kInt, {M}, dev);
  TORCH_CHECK(idx.dim() == 3, who, ": idx must be [C, T, B], got ",
              idx.sizes());
  const long C = idx.size(0), T = idx.size(1), B = idx.size(2);
  TORCH_CHECK(C >= 1 && T >= 1, who, ": empty idx");
  TORCH_CHECK(C < 65536 && T < (1L << 31), who, ": idx too large");
  TORCH_CHECK(B >= 2 && B <= MLPROUND_MAXB, who, ": unsupported B=", B,
              " (2 <= B <= ", MLPROUND_MAXB, ")");
  linround_check(who, "idx", idx, torch::kInt, {C, T, B}, dev);
  linround_check(who, "steps", steps, torch::kInt, {C}, dev);
  linround_check(who, "lr", lr, torch::kFloat, {C, T}, dev);
  linround_check(who, "server", server, torch::kFloat, {N}, dev);
  linround_check(who, "replicas", replicas, torch::kFloat, {C, N}, dev);
  linround_check(who, "mom_init", mom_init, torch::kInt, {C}, dev);
  const bool use_mom = momentum != 0.0;
  if (use_mom)
    linround_check(who, "in_mom", in_mom, torch::kFloat, {C, N}, dev);
  const bool has_snap = snap.numel() != 0;
  if (has_snap) linround_check(who, "snap", snap, torch::kFloat, {C, N}, dev);
  // the gradient correction of the round (an empty tensor: none)
  const bool has_delta = delta.numel() != 0;
  const bool has_cs = ctrl_server.numel() != 0;
  const bool has_cc = ctrl_client.numel() != 0;
  TORCH_CHECK(has_cs == has_cc, who, ": ctrl_server and ctrl_client come as "
              "a pair, got only ", has_cs ? "ctrl_server" : "ctrl_client");
  TORCH_CHECK(!(has_delta && has_cs), who, ": delta and a control pair "
              "together are not supported (one correction vector per "
              "client)");
  if (has_delta)
    linround_check(who, "delta", delta, torch::kFloat, {C, N}, dev);
  if (has_cs) {
    linround_check(who, "ctrl_server", ctrl_server, torch::kFloat, {N}, dev);
    linround_check(who, "ctrl_client", ctrl_client, torch::kFloat, {C, N},
                   dev);
  }
  TORCH_CHECK(std::isfinite(prox_mu) && prox_mu >= 0.0, who,
              ": prox_mu must be finite and >= 0, got ", prox_mu);
  TORCH_CHECK(k_cut >= 0, who, ": k_cut is ", k_cut, ", expected >= 0");
  TORCH_CHECK(!nesterov || (use_mom && dampening == 0.0), who,
              ": nesterov needs a momentum and zero dampening");
  TORCH_CHECK(std::isfinite(eps) && eps > 0.0, who, ": eps must be > 0");
  TORCH_CHECK(wd_numel >= 0 && wd_numel <= N, who, ": wd_numel is ", wd_numel,
              ", the arena has ", N);

  // the layout
  TORCH_CHECK(!layout.empty(), who, ": empty layout");
  const long L = layout[0];
  TORCH_CHECK(L >= 1 && L <= MLPROUND_MAXL, who, ": layout has ", L,
              " blocks (1 <= L <= ", MLPROUND_MAXL, ")");
  TORCH_CHECK((long)layout.size() == 1 + 6 * L + 3, who, ": layout of ", L,
              " blocks must hold ", 1 + 6 * L + 3, " numbers, got ",
              layout.size());
  MlpLayout lay;
  lay.L = (int)L;
  std::vector<std::pair<long, long>> spans;      // [start, end) in the arena
  auto span = [&](long off, long len, const char* what, long i) {
    TORCH_CHECK(off >= 0 && len >= 1 && off + len <= N, who, ": layout ",
                what, " of block ", i, " [", off, ", +", len,
                ") does not fit the arena of ", N);
    spans.emplace_back(off, off + len);
  };
  long prev = F;
  for (long i = 0; i < L; ++i) {
    const int64_t* e = layout.data() + 1 + 6 * i;
    const long in = e[4], out = e[5];
    // column tiles are the grid's y dimension (<= 65535 blocks of 32)
    TORCH_CHECK(in == prev && out >= 1 && out < (1L << 21), who,
                ": layout block ", i, " is [", out, ", ", in,
                "] but its input has ", prev, " features");
    span(e[0], in * out, "weight", i);
    span(e[1], out, "bias", i);
    span(e[2], out, "gamma", i);
    span(e[3], out, "beta", i);
    lay.w[i] = (int)e[0]; lay.b[i] = (int)e[1]; lay.g[i] = (int)e[2];
    lay.be[i] = (int)e[3]; lay.in[i] = (int)in; lay.out[i] = (int)out;
    prev = out;
  }
  const int64_t* h = layout.data() + 1 + 6 * L;
  const long H = h[1], K = h[2];
  TORCH_CHECK(H == prev, who, ": layout head reads ", H,
              " features but the last block has ", prev);
  TORCH_CHECK(K >= 1 && K <= MLPROUND_MAXK, who, ": unsupported K=", K,
              " (1 <= K <= ", MLPROUND_MAXK, ")");
  span(h[0], H * K, "head weight", L);
  lay.fc = (int)h[0]; lay.H = (int)H; lay.K = (int)K;
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i)
    TORCH_CHECK(spans[i - 1].second <= spans[i].first, who,
                ": layout tensors overlap at arena element ", spans[i].first);

  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  TORCH_CHECK(hipStreamIsCapturing(STREAM, &cap) == hipSuccess, who,
              ": hipStreamIsCapturing failed");
  if (cap == hipStreamCaptureStatusNone) {
    const long top = idx.max().item<int>();
    TORCH_CHECK(top < M, who, ": idx holds row ", top, " but X has ", M,
                " rows");
    const long most = steps.max().item<int>();
    TORCH_CHECK(most <= T, who, ": steps holds ", most, " but idx has T=", T);
  }

  // workspace per client: xh, a, rstd per block; dz per block; dlogits
  long off = 0;
  for (long i = 0; i < L; ++i) {
    lay.xh[i] = (int)off;   off += B * lay.out[i];
    lay.act[i] = (int)off;  off += B * lay.out[i];
    lay.rstd[i] = (int)off; off += lay.out[i];
    lay.dz[i] = (int)off;   off += B * lay.out[i];
  }
  lay.dz[L] = (int)off; off += B * K;
  TORCH_CHECK(off < (1L << 31), who, ": workspace too large");
  lay.ws_stride = off;
  auto ws = torch::empty({C, off}, X.options());
  auto loss = torch::zeros({C, T}, X.options());

  MlpRoundArgs a;
  a.X = X.data_ptr<float>();
  a.Y = Y.data_ptr<int>();
  a.idx = idx.data_ptr<int>();
  a.steps = steps.data_ptr<int>();
  a.lr = lr.data_ptr<float>();
  a.server = server.data_ptr<float>();
  a.replicas = replicas.data_ptr<float>();
  a.in_mom = use_mom ? in_mom.data_ptr<float>() : nullptr;
  a.mom_init = mom_init.data_ptr<int>();
  a.snap = has_snap ? snap.data_ptr<float>() : nullptr;
  a.loss = loss.data_ptr<float>();
  a.ws = ws.data_ptr<float>();
  a.M = (int)M; a.B = (int)B; a.T = (int)T; a.N = (int)N;
  a.k_cut = (int)std::min<long>(k_cut, 1L << 30);
  a.use_mom = use_mom; a.nesterov = nesterov; a.wd_numel = (int)wd_numel;
  a.wd = (float)weight_decay; a.mom = (float)momentum;
  a.omd = (float)(1.0 - dampening); a.eps = (float)eps;
  a.corr_rows = has_delta ? delta.data_ptr<float>()
                : has_cs  ? ctrl_client.data_ptr<float>()
                          : nullptr;
  a.ctrl_s = has_cs ? ctrl_server.data_ptr<float>() : nullptr;
  a.prox_mu = (float)prox_mu;
  a.corr = (has_delta ? MLPROUND_DELTA : 0) | (has_cs ? MLPROUND_CTRL : 0) |
           (prox_mu != 0.0 ? MLPROUND_PROX : 0);
  a.lay = lay;

  const dim3 blk(MLPROUND_THREADS);
  auto tiles = [](long n) { return (unsigned)((n + MLP_TN - 1) / MLP_TN); };
  const unsigned rowb =
      (unsigned)std::min<long>((N + 4 * MLPROUND_THREADS - 1) /
                                   (4 * MLPROUND_THREADS), 64);
  const unsigned Cu = (unsigned)C;
  hipLaunchKernelGGL(mlp_rows_k, dim3(Cu, rowb), blk, 0, STREAM, a, 0);
  for (int s = 0; s < (int)T; ++s) {
    if (has_snap && s + 1 == k_cut)
      hipLaunchKernelGGL(mlp_rows_k, dim3(Cu, rowb), blk, 0, STREAM, a, 1);
    hipLaunchKernelGGL(mlp_fwd_layer_k<true>, dim3(Cu, tiles(lay.out[0])),
                       blk, 0, STREAM, a, s, 0);
    for (int i = 1; i < (int)L; ++i)
      hipLaunchKernelGGL(mlp_fwd_layer_k<false>, dim3(Cu, tiles(lay.out[i])),
                         blk, 0, STREAM, a, s, i);
    hipLaunchKernelGGL(mlp_head_k<false>, dim3(Cu), blk, 0, STREAM, a, s,
                       0);
    // without a correction: the kernels that know none
    for (int i = (int)L - 1; i >= 0; --i) {
      if (a.corr)
        hipLaunchKernelGGL((mlp_bwd_k<false, true>),
                           dim3(Cu, tiles(lay.out[i])), blk, 0, STREAM, a, s,
                           i);
      else
        hipLaunchKernelGGL((mlp_bwd_k<false, false>),
                           dim3(Cu, tiles(lay.out[i])), blk, 0, STREAM, a, s,
                           i);
    }
    if (a.corr)
      hipLaunchKernelGGL((mlp_bwd_k<true, true>), dim3(Cu, tiles(lay.in[0])),
                         blk, 0, STREAM, a, s, 0);
    else
      hipLaunchKernelGGL((mlp_bwd_k<true, false>), dim3(Cu, tiles(lay.in[0])),
                         blk, 0, STREAM, a, s, 0);
  }
  if (use_mom)
    hipLaunchKernelGGL(mlp_rows_k, dim3(Cu, 1), blk, 0, STREAM, a, 2);
  return loss;
}

// ==========================================================================
// packed CNN: all clients' local steps batched per layer (cnnround.h)
// ==========================================================================
// [max B, max K, max Cin, max S, max C1, max C2, max H]
std::vector<int64_t> cnn_round_limits() {
  return {CNNROUND_MAXB, CNNROUND_MAXK, CNNROUND_MAXCIN, CNNROUND_MAXS,
          CNNROUND_MAXC1, CNNROUND_MAXC2, CNNROUND_MAXH};
}

// layout: [Cin, S, w1, b1, C1, nhwc1, w2, b2, C2, nhwc2, fw1, fb1, H, fw2,
// fb2, K] -- the image, and arena offsets and shapes of conv1, conv2, fc1,
// fc2.  Returns loss [C, T]; writes replicas / in_mom / mom_init / snap rows
// of the clients with steps > 0.  idx and steps are range-checked on the host
// unless the stream is capturing (the kernels never read X outside [0, M)).
torch::Tensor cnn_local_rounds(
    torch::Tensor X, torch::Tensor Y, torch::Tensor idx, torch::Tensor steps,
    torch::Tensor lr, torch::Tensor server, torch::Tensor replicas,
    torch::Tensor in_mom, torch::Tensor mom_init, torch::Tensor snap,
    long k_cut, std::vector<int64_t> layout, long wd_numel,
    double weight_decay, double momentum, double dampening, bool nesterov) {
  const char* who = "cnn_local_rounds";
  TORCH_CHECK(X.is_cuda() && X.dim() == 2 && X.is_contiguous(), who,
              ": X must be contiguous [M, Cin*S*S] on GPU");
  TORCH_CHECK(X.scalar_type() == torch::kFloat, who, ": X must be fp32");
  const long M = X.size(0), F = X.size(1);
  const auto dev = X.device();
  TORCH_CHECK(M >= 1 && F >= 1, who, ": empty X");
  TORCH_CHECK(M < (1L << 31), who, ": X too large");
  TORCH_CHECK(server.dim() == 1 && server.size(0) < (1L << 30), who,
              ": server must be [N], N < 2^30");
  const long N = server.size(0);
  linround_check(who, "Y", Y, torch::kInt, {M}, dev);
  TORCH_CHECK(idx.dim() == 3, who, ": idx must be [C, T, B], got ",
              idx.sizes());
  const long C = idx.size(0), T = idx.size(1), B = idx.size(2);
  TORCH_CHECK(C >= 1 && T >= 1, who, ": empty idx");
  TORCH_CHECK(C < 65536 && T < (1L << 31), who, ": idx too large");
  TORCH_CHECK(B >= 1 && B <= CNNROUND_MAXB, who, ": unsupported B=", B,
              " (1 <= B <= ", CNNROUND_MAXB, ")");
  linround_check(who, "idx", idx, torch::kInt, {C, T, B}, dev);
  linround_check(who, "steps", steps, torch::kInt, {C}, dev);
  linround_check(who, "lr", lr, torch::kFloat, {C, T}, dev);
  linround_check(who, "server", server, torch::kFloat, {N}, dev);
  linround_check(who, "replicas", replicas, torch::kFloat, {C, N}, dev);
  linround_check(who, "mom_init", mom_init, torch::kInt, {C}, dev);
  const bool use_mom = momentum != 0.0;
  if (use_mom)
    linround_check(who, "in_mom", in_mom, torch::kFloat, {C, N}, dev);
  const bool has_snap = snap.numel() != 0;
  if (has_snap) linround_check(who, "snap", snap, torch::kFloat, {C, N}, dev);
  TORCH_CHECK(k_cut >= 0, who, ": k_cut is ", k_cut, ", expected >= 0");
  TORCH_CHECK(!nesterov || (use_mom && dampening == 0.0), who,
              ": nesterov needs a momentum and zero dampening");
  TORCH_CHECK(wd_numel >= 0 && wd_numel <= N, who, ": wd_numel is ", wd_numel,
              ", the arena has ", N);

  // the layout
  TORCH_CHECK(layout.size() == 16, who, ": layout must hold 16 numbers "
              "(image, conv1, conv2, fc1, fc2), got ", layout.size());
  const long Cin = layout[0], S = layout[1], C1 = layout[4], C2 = layout[8],
             H = layout[12], K = layout[15];
  TORCH_CHECK(Cin >= 1 && Cin <= CNNROUND_MAXCIN && S >= 1 &&
                  S <= CNNROUND_MAXS,
              who, ": unsupported image (Cin=", Cin, ", S=", S,
              "), 1 <= Cin <= ", CNNROUND_MAXCIN, ", S <= ", CNNROUND_MAXS);
  TORCH_CHECK(S >= 6 && (S - 4) % 2 == 0 && (S - 4) / 2 >= 6 &&
                  ((S - 4) / 2 - 4) % 2 == 0,
              who, ": S=", S, " does not pool evenly twice (S - 4 and "
              "(S - 4) / 2 - 4 even, the last map at least 1x1)");
  const long S1 = (S - 4) / 2, O2 = S1 - 4, S2 = O2 / 2, F2 = C2 * S2 * S2;
  TORCH_CHECK(F == Cin * S * S, who, ": X has ", F, " features, the image (",
              Cin, ", ", S, ", ", S, ") has ", Cin * S * S);
  TORCH_CHECK(C1 >= 1 && C1 <= CNNROUND_MAXC1 && C2 >= 1 &&
                  C2 <= CNNROUND_MAXC2 && H >= 1 && H <= CNNROUND_MAXH,
              who, ": unsupported C1=", C1, " C2=", C2, " H=", H,
              " (C1 <= ", CNNROUND_MAXC1, ", C2 <= ", CNNROUND_MAXC2,
              ", H <= ", CNNROUND_MAXH, ")");
  TORCH_CHECK(K >= 1 && K <= CNNROUND_MAXK, who, ": unsupported K=", K,
              " (1 <= K <= ", CNNROUND_MAXK, ")");
  for (int i : {5, 9})
    TORCH_CHECK(layout[i] == 0 || layout[i] == 1, who,
                ": the nhwc flag of a conv must be 0 or 1, got ", layout[i]);
  std::vector<std::pair<long, long>> spans;      // [start, end) in the arena
  auto span = [&](long off, long len, const char* what) {
    TORCH_CHECK(off >= 0 && off + len <= N, who, ": layout ", what, " [", off,
                ", +", len, ") does not fit the arena of ", N);
    spans.emplace_back(off, off + len);
  };
  span(layout[2], C1 * Cin * 25, "conv1 weight");
  span(layout[3], C1, "conv1 bias");
  span(layout[6], C2 * C1 * 25, "conv2 weight");
  span(layout[7], C2, "conv2 bias");
  span(layout[10], H * F2, "fc1 weight");
  span(layout[11], H, "fc1 bias");
  span(layout[13], K * H, "fc2 weight");
  span(layout[14], K, "fc2 bias");
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i)
    TORCH_CHECK(spans[i - 1].second <= spans[i].first, who,
                ": layout tensors overlap at arena element ", spans[i].first);

  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  TORCH_CHECK(hipStreamIsCapturing(STREAM, &cap) == hipSuccess, who,
              ": hipStreamIsCapturing failed");
  if (cap == hipStreamCaptureStatusNone) {
    const long top = idx.max().item<int>();
    TORCH_CHECK(top < M, who, ": idx holds row ", top, " but X has ", M,
                " rows");
    const long most = steps.max().item<int>();
    TORCH_CHECK(most <= T, who, ": steps holds ", most, " but idx has T=", T);
  }

  CnnLayout lay;
  lay.Cin = (int)Cin; lay.S = (int)S; lay.C1 = (int)C1; lay.C2 = (int)C2;
  lay.H = (int)H; lay.K = (int)K;
  lay.S1 = (int)S1; lay.S2 = (int)S2; lay.O2 = (int)O2; lay.F2 = (int)F2;
  lay.w1 = (int)layout[2]; lay.b1 = (int)layout[3];
  lay.nhwc1 = (int)layout[5];
  lay.w2 = (int)layout[6]; lay.b2 = (int)layout[7];
  lay.nhwc2 = (int)layout[9];
  lay.fw1 = (int)layout[10]; lay.fb1 = (int)layout[11];
  lay.fw2 = (int)layout[13]; lay.fb2 = (int)layout[14];
  // workspace per client: p1, p2, a, dlogits, dz1, dp2, dp1; argmax bytes
  const long np1 = C1 * S1 * S1;
  long off = 0;
  lay.p1 = (int)off;  off += B * np1;
  lay.p2 = (int)off;  off += B * F2;
  lay.act = (int)off; off += B * H;
  lay.dl = (int)off;  off += B * K;
  lay.dz1 = (int)off; off += B * H;
  lay.dp2 = (int)off; off += B * F2;
  lay.dp1 = (int)off; off += B * np1;
  lay.am1 = 0;
  lay.am2 = (int)(B * np1);
  lay.wsb_stride = B * np1 + B * F2;
  auto ws = torch::empty({C, off}, X.options());
  auto wsb = torch::empty({C, lay.wsb_stride},
                          X.options().dtype(torch::kUInt8));
  auto loss = torch::zeros({C, T}, X.options());

  CnnRoundArgs a;
  MlpRoundArgs& m = a.m;
  m.X = X.data_ptr<float>();
  m.Y = Y.data_ptr<int>();
  m.idx = idx.data_ptr<int>();
  m.steps = steps.data_ptr<int>();
  m.lr = lr.data_ptr<float>();
  m.server = server.data_ptr<float>();
  m.replicas = replicas.data_ptr<float>();
  m.in_mom = use_mom ? in_mom.data_ptr<float>() : nullptr;
  m.mom_init = mom_init.data_ptr<int>();
  m.snap = has_snap ? snap.data_ptr<float>() : nullptr;
  m.loss = loss.data_ptr<float>();
  m.ws = ws.data_ptr<float>();
  m.corr_rows = nullptr; m.ctrl_s = nullptr;
  m.M = (int)M; m.B = (int)B; m.T = (int)T; m.N = (int)N;
  m.k_cut = (int)std::min<long>(k_cut, 1L << 30);
  m.use_mom = use_mom; m.nesterov = nesterov; m.wd_numel = (int)wd_numel;
  m.wd = (float)weight_decay; m.mom = (float)momentum;
  m.omd = (float)(1.0 - dampening); m.eps = 0.f;
  m.prox_mu = 0.f; m.corr = 0;
  // what mlp_head_k reads: one block whose activation is fc1's
  m.lay = MlpLayout{};
  m.lay.L = 1;
  m.lay.act[0] = lay.act; m.lay.dz[1] = lay.dl;
  m.lay.fc = lay.fw2; m.lay.H = lay.H; m.lay.K = lay.K;
  m.lay.ws_stride = off;
  a.lay = lay;
  a.wsb = wsb.data_ptr<uint8_t>();

  const dim3 blk(CNNROUND_THREADS);
  auto tiles = [](long n) { return (unsigned)((n + MLP_TN - 1) / MLP_TN); };
  const unsigned rowb =
      (unsigned)std::min<long>((N + 4 * MLPROUND_THREADS - 1) /
                                   (4 * MLPROUND_THREADS), 64);
  const unsigned Cu = (unsigned)C, Bu = (unsigned)B;
  const long K2 = 25 * C1, Kp = (K2 + 3) / 4 * 4, npx = O2 * O2;
  const size_t lds_fwd = sizeof(float) * (Kp * 16 + np1 + Kp);
  const size_t lds_dg = sizeof(float) *
      (CNN_DG_CO * (S1 + 4) * (S1 + 4) + 25 * CNN_DG_CO * 17);
  const size_t lds_wrw = sizeof(float) *
      (CNNROUND_MAXC2 * (npx | 1) + np1 + 16 * CNN_WRW_NT + npx +
       CNNROUND_THREADS);
  const unsigned t16c2 = (unsigned)((C2 + 15) / 16);
  const unsigned t16c1 = (unsigned)((C1 + 15) / 16);
  const unsigned nwrw =
      (unsigned)((K2 + 16 * CNN_WRW_NT - 1) / (16 * CNN_WRW_NT));
  hipLaunchKernelGGL(mlp_rows_k, dim3(Cu, rowb), blk, 0, STREAM, m, 0);
  for (int s = 0; s < (int)T; ++s) {
    if (has_snap && s + 1 == k_cut)
      hipLaunchKernelGGL(mlp_rows_k, dim3(Cu, rowb), blk, 0, STREAM, m, 1);
    hipLaunchKernelGGL(cnn_conv1_fwd_k, dim3(Cu, Bu), blk, 0, STREAM, a, s);
    hipLaunchKernelGGL(cnn_conv2_fwd_k,
                       dim3(Cu, t16c2, std::min(Bu, 8u)), blk, lds_fwd,
                       STREAM, a, s);
    hipLaunchKernelGGL(cnn_fc1_fwd_k, dim3(Cu, tiles(H)), blk, 0, STREAM, a,
                       s);
    hipLaunchKernelGGL(mlp_head_k<true>, dim3(Cu), blk, 0, STREAM, m, s,
                       lay.fb2);
    hipLaunchKernelGGL(cnn_fc_bwd_k<true>, dim3(Cu, tiles(H)), blk, 0, STREAM,
                       a, s);
    hipLaunchKernelGGL(cnn_fc_bwd_k<false>, dim3(Cu, tiles(F2)), blk, 0,
                       STREAM, a, s);
    hipLaunchKernelGGL(cnn_conv2_dgrad_k, dim3(Cu, t16c1, Bu), blk, lds_dg,
                       STREAM, a, s);
    hipLaunchKernelGGL(cnn_conv2_wrw_k, dim3(Cu, nwrw), blk, lds_wrw, STREAM,
                       a, s);
    hipLaunchKernelGGL(cnn_conv1_wrw_k, dim3(Cu, (unsigned)C1), blk, 0,
                       STREAM, a, s);
  }
  if (use_mom)
    hipLaunchKernelGGL(mlp_rows_k, dim3(Cu, 1), blk, 0, STREAM, m, 2);
  return loss;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("cnn_local_rounds", &cnn_local_rounds);
  m.def("cnn_round_limits", &cnn_round_limits);
  m.def("mlp_local_rounds", &mlp_local_rounds);
  m.def("mlp_round_max_batch", &mlp_round_max_batch);
  m.def("mlp_round_max_classes", &mlp_round_max_classes);
  m.def("mlp_round_max_layers", &mlp_round_max_layers);
  m.def("linear_local_rounds", &linear_local_rounds);
  m.def("linear_round_max_floats", &linear_round_max_floats);
  m.def("linear_round_lds_floats", &linear_round_lds_floats);
  m.def("gru_fwd", &gru_fwd);
  m.def("gru_bwd", &gru_bwd);
  m.def("head_fwd", &head_fwd);
  m.def("head_bwd", &head_bwd);
  m.def("ce_topk_accum", &ce_topk_accum);
  m.def("bn_fwd_train", &bn_fwd_train);
  m.def("bn_fwd_train_part", &bn_fwd_train_part);
  m.def("bn_bwd", &bn_bwd);
  m.def("fused_sgd_step", &fused_sgd_step, "fused dual-mode SGD step");
  m.def("weighted_diff_restore", &weighted_diff_restore);
  m.def("scaled_diff", &scaled_diff);
  m.def("axpby", &axpby);
  m.def("error_feedback_update", &error_feedback_update);
  m.def("delta_update", &delta_update);
  m.def("scaffold_control_update", &scaffold_control_update);
  m.def("blend", &blend);
  m.def("alpha_grad", &alpha_grad);
  m.def("quantize_adaptive", &quantize_adaptive);
  m.def("dequantize", &dequantize);
  m.def("dequant_accumulate", &dequant_accumulate);
  m.def("topk_compress", &topk_compress);
  m.def("scatter_accumulate", &scatter_accumulate);
  m.def("multi_diff_accumulate", &multi_diff_accumulate);
  m.def("multi_delta_update", &multi_delta_update);
  m.def("multi_scaffold_control_update", &multi_scaffold_control_update);
  m.def("fedadam_normalize", &fedadam_normalize);
  m.def("gather_grads", &gather_grads);
  m.def("stem_conv_fwd", &stem_conv_fwd);
  m.def("stem_conv_wrw", &stem_conv_wrw);
  m.def("cast_to_half", &cast_to_half);
  m.def("mfma_probe", &mfma_probe);
  m.def("conv3x3_wrw", &conv3x3_wrw);
  m.def("conv3x3_wrw2", &conv3x3_wrw2);
  m.def("conv3x3_wrw2_grid_cap", &conv3x3_wrw2_grid_cap);
  m.def("conv3x3_dgrad", &conv3x3_dgrad);
  m.def("conv3x3_dgrad_bn", &conv3x3_dgrad_bn);
  m.def("bn_bwd_defer", &bn_bwd_defer);
  m.def("conv3x3_bn_fwd", &conv3x3_bn_fwd);
  m.def("conv3x3s2_bn_fwd", &conv3x3s2_bn_fwd);
  m.def("conv3x3_bn_act_fwd", &conv3x3_bn_act_fwd);
  m.def("bn_fwd_eval", &bn_fwd_eval);
  m.def("conv3x3s2_dgrad", &conv3x3s2_dgrad);
  m.def("conv3x3s2_wrw", &conv3x3s2_wrw);
  m.def("conv3x3s2_wrw_grid_cap", &conv3x3s2_wrw_grid_cap);
}
