// K6, row-wise kernels of the sentence encoder: one wave per token (or per weight row), fp32 math, nothing on MFMA.
//   enc_embed_ln_kernel   gather word + position + type rows, LayerNorm, one wave per token
//   enc_ln_kernel         LayerNorm, scalar form (the residual add is in the GEMM epilogue)
//   enc_ln_vec_kernel     LayerNorm when H % 8 == 0 and H <= 2048: the row read once as 16-byte chunks, kept in registers
//   enc_ln_stats_kernel   fused-LayerNorm flow: (mu, rstd) per token from the partial sums a GEMM epilogue left
//   enc_fold_ln_kernel    fused-LayerNorm flow: gamma folded into the weights of the Linear that consumes a LayerNorm
//   enc_add_vec_kernel    fused-LayerNorm flow: bias + beta
//   enc_pool_kernel       masked mean or CLS, optional L2 normalisation, fp32 out
#include "enc_kernels.h"

namespace mrag {

// ------------------------------------------------------------------ embeddings + LayerNorm
template <typename E>
__global__ __launch_bounds__(256) void enc_embed_ln_kernel(const int32_t* __restrict__ ids, int64_t n_tok, int S, int H, int vocab,
                                                           const float* __restrict__ word, const float* __restrict__ pos,
                                                           const float* __restrict__ type0, const float* __restrict__ g,
                                                           const float* __restrict__ b, float eps, E* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t tok = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= n_tok) return;
  int id = ids[tok];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const int s = (int)(tok % S);
  const float* w = word + (size_t)id * H;
  const float* p = pos + (size_t)s * H;
  float sum = 0.f, sq = 0.f;
  for (int i = lane; i < H; i += 64) {
    const float x = w[i] + p[i] + type0[i];
    sum += x;
  }
  sum = wave_sum(sum);
  const float mean = sum / H;
  for (int i = lane; i < H; i += 64) {
    const float x = w[i] + p[i] + type0[i] - mean;
    sq += x * x;
  }
  sq = wave_sum(sq);
  const float rstd = 1.0f / sqrtf(sq / H + eps);
  for (int i = lane; i < H; i += 64) {
    const float x = w[i] + p[i] + type0[i];
    out[(size_t)tok * H + i] = (E)((x - mean) * rstd * g[i] + b[i]);
  }
}

template <typename E>
__global__ __launch_bounds__(256) void enc_ln_kernel(const E* __restrict__ x, int64_t n_tok, int H, const float* __restrict__ g,
                                                     const float* __restrict__ b, float eps, E* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t tok = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= n_tok) return;
  const E* r = x + (size_t)tok * H;
  float sum = 0.f, sq = 0.f;
  for (int i = lane; i < H; i += 64) sum += (float)r[i];
  sum = wave_sum(sum);
  const float mean = sum / H;
  for (int i = lane; i < H; i += 64) {
    const float d = (float)r[i] - mean;
    sq += d * d;
  }
  sq = wave_sum(sq);
  const float rstd = 1.0f / sqrtf(sq / H + eps);
  for (int i = lane; i < H; i += 64) out[(size_t)tok * H + i] = (E)(((float)r[i] - mean) * rstd * g[i] + b[i]);
}

// Vector form used when H % 8 == 0 and H <= 2048: one wave per token, the row is read ONCE as 16-byte
// chunks (chunk c of lane l: c = l, l + 64, ...) and kept in registers for the mean, the variance
// (two passes over registers, same arithmetic as above) and the normalised 16-byte stores.  HBM-bound:
// 2 x H x 2 bytes per token.  (The scalar kernel above moved 128 B per wave instruction and re-read the
// row twice: 1.6 TB/s measured at H = 768.)
template <typename E>
__global__ __launch_bounds__(256) void enc_ln_vec_kernel(const E* __restrict__ x, int64_t n_tok, int H, const float* __restrict__ g,
                                                         const float* __restrict__ b, float eps, E* __restrict__ out) {
  typedef E e8 __attribute__((ext_vector_type(8)));
  constexpr int MAXC = 4;
  const int lane = threadIdx.x & 63;
  const int64_t tok = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tok >= n_tok) return;
  const int nch = H >> 3;
  const e8* r = (const e8*)(x + (size_t)tok * H);
  float v[MAXC][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
      const e8 t = r[c];
#pragma unroll
      for (int j = 0; j < 8; ++j) { v[i][j] = (float)t[j]; sum += v[i][j]; }
    }
  }
  sum = wave_sum(sum);
  const float mean = sum / H;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float d = v[i][j] - mean; sq += d * d; }
    }
  }
  sq = wave_sum(sq);
  const float rstd = 1.0f / sqrtf(sq / H + eps);
  e8* o = (e8*)(out + (size_t)tok * H);
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nch) {
      const float4 g0 = ((const float4*)g)[2 * c], g1 = ((const float4*)g)[2 * c + 1];
      const float4 b0 = ((const float4*)b)[2 * c], b1 = ((const float4*)b)[2 * c + 1];
      const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
      const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
      e8 t;
#pragma unroll
      for (int j = 0; j < 8; ++j) t[j] = (E)((v[i][j] - mean) * rstd * gg[j] + bb[j]);
      o[c] = t;
    }
  }
}

// (mu, rstd) per token from the partial sums of the producing GEMM (fixed slot order: deterministic)
__global__ void enc_ln_stats_kernel(const float2* __restrict__ partials, int np, int64_t n_tok, int H, float eps, float2* __restrict__ stats) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tok) return;
  float s1 = 0.f, s2 = 0.f;
  for (int i = 0; i < np; ++i) { const float2 p = partials[t * np + i]; s1 += p.x; s2 += p.y; }
  const float mean = s1 / H;
  const float var = fmaxf(s2 / H - mean * mean, 0.f);
  stats[t] = make_float2(mean, 1.0f / sqrtf(var + eps));
}

// LayerNorm folded into the Linear that consumes it: Wf = round(gamma o W), s_n = sum_k Wf[n][k], c_n = b_n + sum_k beta_k W[n][k].
// One wave per output row.
template <typename E>
__global__ __launch_bounds__(256) void enc_fold_ln_kernel(const E* __restrict__ W, const float* __restrict__ b, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, int N, int K, E* __restrict__ Wf,
                                                          float* __restrict__ c, float* __restrict__ svec) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  float s = 0.f, cb = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float w = (float)W[(size_t)n * K + k];
    const E wf = (E)(gamma[k] * w);
    Wf[(size_t)n * K + k] = wf;
    s += (float)wf;
    cb += beta[k] * w;
  }
  s = wave_sum(s); cb = wave_sum(cb);
  if (lane == 0) { svec[n] = s; c[n] = b[n] + cb; }
}

__global__ void enc_add_vec_kernel(const float* __restrict__ a, const float* __restrict__ b, int n, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] + b[i];
}

// ------------------------------------------------------------------ pooling + L2 norm
template <typename E>
__global__ __launch_bounds__(256) void enc_pool_kernel(const E* __restrict__ x, const int32_t* __restrict__ mask, int B, int S, int H,
                                                       int pool, int normalize, float* __restrict__ out) {
  extern __shared__ float acc[];   // [H]
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ float red[256];
  float cnt = 0.f;
  if (pool == MRAG_POOL_MEAN) {
    for (int s = 0; s < S; ++s) cnt += mask[(size_t)b * S + s] != 0 ? 1.f : 0.f;
    cnt = fmaxf(cnt, 1e-9f);        // sentence-transformers clamps the token count
  }
  float ss = 0.f;
  for (int i = tid; i < H; i += 256) {
    float v;
    if (pool == MRAG_POOL_CLS) v = (float)x[((size_t)b * S) * H + i];
    else {
      float a = 0.f;
      for (int s = 0; s < S; ++s)
        if (mask[(size_t)b * S + s] != 0) a += (float)x[((size_t)b * S + s) * H + i];
      v = a / cnt;
    }
    acc[i] = v;
    ss += v * v;
  }
  red[tid] = ss;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  const float nrm = normalize ? fmaxf(sqrtf(red[0]), 1e-12f) : 1.f;   // F.normalize eps
  for (int i = tid; i < H; i += 256) out[(size_t)b * H + i] = acc[i] / nrm;
}

// ------------------------------------------------------------------ launchers
static const dim3 kRowBlock(256);                                                              // four waves = four rows per workgroup
static dim3 row_grid(int64_t rows) { return dim3((unsigned)((rows + 3) / 4)); }
// f(E{}) with E the 16-bit element type of dt
template <typename F>
static void with_elem(int dt, F&& f) { if (dt == MRAG_F16) f(_Float16{}); else f(__bf16{}); }

int launch_embed_ln(int dt, const int32_t* ids, int64_t n_tok, int S, int H, int vocab, const float* word, const float* pos, const float* type0,
                    const float* g, const float* b, float eps, uint16_t* out, hipStream_t stream) {
  with_elem(dt, [&](auto z) {
    typedef decltype(z) E;
    hipLaunchKernelGGL((enc_embed_ln_kernel<E>), row_grid(n_tok), kRowBlock, 0, stream, ids, n_tok, S, H, vocab, word, pos, type0, g, b, eps, (E*)out);
  });
  return launched();
}

int launch_ln(int dt, const uint16_t* x, int64_t n_tok, int H, const float* g, const float* b, float eps, uint16_t* out, hipStream_t stream) {
  with_elem(dt, [&](auto z) {
    typedef decltype(z) E;
    if (H % 8 == 0 && H <= 2048)
      hipLaunchKernelGGL((enc_ln_vec_kernel<E>), row_grid(n_tok), kRowBlock, 0, stream, (const E*)x, n_tok, H, g, b, eps, (E*)out);
    else hipLaunchKernelGGL((enc_ln_kernel<E>), row_grid(n_tok), kRowBlock, 0, stream, (const E*)x, n_tok, H, g, b, eps, (E*)out);
  });
  return launched();
}

int launch_ln_stats(const float* partials, int np, int64_t n_tok, int H, float eps, float* stats, hipStream_t stream) {
  hipLaunchKernelGGL(enc_ln_stats_kernel, dim3((unsigned)((n_tok + 255) / 256)), dim3(256), 0, stream, (const float2*)partials, np, n_tok, H, eps,
                     (float2*)stats);
  return launched();
}

int launch_fold_ln(int dt, const uint16_t* W, const float* b, const float* gamma, const float* beta, int N, int K, uint16_t* Wf, float* c,
                   float* svec, hipStream_t stream) {
  with_elem(dt, [&](auto z) {
    typedef decltype(z) E;
    hipLaunchKernelGGL((enc_fold_ln_kernel<E>), row_grid(N), kRowBlock, 0, stream, (const E*)W, b, gamma, beta, N, K, (E*)Wf, c, svec);
  });
  return launched();
}

int launch_add_vec(const float* a, const float* b, int n, float* out, hipStream_t stream) {
  hipLaunchKernelGGL(enc_add_vec_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a, b, n, out);
  return launched();
}

int launch_pool(int dt, const uint16_t* x, const int32_t* mask, int B, int S, int H, int pool, int normalize, float* out, hipStream_t stream) {
  with_elem(dt, [&](auto z) {   // dynamic LDS: the pooled row, before its norm is known
    typedef decltype(z) E;
    hipLaunchKernelGGL((enc_pool_kernel<E>), dim3((unsigned)B), dim3(256), (size_t)H * 4, stream, (const E*)x, mask, B, S, H, pool, normalize, out);
  });
  return launched();
}

}  // namespace mrag
