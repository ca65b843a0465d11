// The forward sequence kernel of gru.h, included twice:
//   GRU_FWD_TOK 0  gru_fwd_k<NT>      gx [B, T, 3H]
//   GRU_FWD_TOK 1  gru_tok_fwd_k<NT>  P [V, 3H] and tok [B, T] in place of gx,
//                                     scalar fp32 code only (GRU_SCALAR_F32)
// A function's target attribute cannot depend on a template parameter, and a
// shared __device__ body inlined into two kernels changes the register
// allocation of gru_fwd_k, so the text is shared instead: gru_fwd_k is the
// code it was before the token variant existed.
// grid ceil(B/16), block 64*NT.  gates [B, T, 4, H] = (r, z, n, q) or null.
template <int NT>
#if GRU_FWD_TOK
__global__ void __launch_bounds__(NT * WAVE) GRU_SCALAR_F32
gru_tok_fwd_k(const float* __restrict__ gx, const long* __restrict__ tok,
              int V, const void* __restrict__ w,
#else
__global__ void __launch_bounds__(NT * WAVE)
gru_fwd_k(const float* __restrict__ gx, const void* __restrict__ w,
#endif
          int w_bf16, const void* __restrict__ bias, int b_bf16,
          const float* __restrict__ h0, float* __restrict__ out,
          float* __restrict__ gates, int B, int T, int H) {
  constexpr bool TOK = GRU_FWD_TOK;
#if !GRU_FWD_TOK
  constexpr const long* tok = nullptr;  // unused
  constexpr int V = 0;
#endif
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
  int tk[4];                            // TOK: P offset of step t + 1, or -1
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (TOK) {
      const long ti = (b0 + 4 * lk + i) * T;
      const int o = gru_tok_off(tok, ti, live[i], V, 3 * H);
      tk[i] = gru_tok_off(tok, ti + 1, live[i] && 1 < T, V, 3 * H);
      const float* p = gx + o + col;
      xr[i] = o >= 0 ? p[0] : 0.f;
      xz[i] = o >= 0 ? p[H] : 0.f;
      xn[i] = o >= 0 ? p[2 * H] : 0.f;
    } else {
      const float* p = gx + ob[i] * 3 - 2 * col;   // (b*T + 0)*3H + col
      xr[i] = live[i] ? p[0] : 0.f;
      xz[i] = live[i] ? p[H] : 0.f;
      xn[i] = live[i] ? p[2 * H] : 0.f;
    }
  }
  __syncthreads();

  const float* wr = Ws + (0 * HP + col) * S + lk;
  const float* wz = Ws + (1 * HP + col) * S + lk;
  const float* wn = Ws + (2 * HP + col) * S + lk;
  for (int t = 0; t < T; ++t) {
    const int cur = t & 1;
    // next step's input projection, in flight during the MFMAs
    float yr[4], yz[4], yn[4];
    int tn[4];                          // TOK: P offset of step t + 2, or -1
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (TOK) {
        // tk is -1 beyond the last step and on dead rows
        const float* p = gx + tk[i] + col;
        yr[i] = tk[i] >= 0 ? p[0] : 0.f;
        yz[i] = tk[i] >= 0 ? p[H] : 0.f;
        yn[i] = tk[i] >= 0 ? p[2 * H] : 0.f;
        tn[i] = gru_tok_off(tok, (b0 + 4 * lk + i) * T + t + 2,
                            live[i] && t + 2 < T, V, 3 * H);
      } else {
        const bool ld = live[i] && t + 1 < T;
        const float* p = gx + (ob[i] + (long)(t + 1) * H) * 3 - 2 * col;
        yr[i] = ld ? p[0] : 0.f;
        yz[i] = ld ? p[H] : 0.f;
        yn[i] = ld ? p[2 * H] : 0.f;
      }
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
      float h;
      if constexpr (TOK) {
        // gru_fwd_k adds two ROUNDED products here (its compiler pairs them
        // into packed multiplies); the scalar-only kernel spells that out, so
        // that both give the same bits for the same gx
#pragma clang fp contract(off)
        const float p0 = (1.f - z) * n, p1 = z * hprev[i];
        h = p0 + p1;
      } else {
        h = (1.f - z) * n + z * hprev[i];
      }
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
      if constexpr (TOK) tk[i] = tn[i];
    }
    __syncthreads();
  }
}
