// K6: BERT-family sentence-encoder forward (MiniLM-L6 / bge-base shapes) -- fills the
// LLMProvider.embed slot of the reference (app/core/providers/base.py:6, called from
// app/core/llm_router.py:115).  The reference itself contains no encoder; the architecture
// follows HF BertModel (embeddings + LN, L x {MHA, erf-GELU FFN, post-LN residuals}), pooling
// (mean over the mask, or CLS) and L2 normalisation as in sentence-transformers.
//
// Kernels (fp16 or bf16 activations/weights, fp32 accumulation and fp32 LN/softmax/GELU math)
//   enc_embed_ln_kernel   gather word + position + type rows, LayerNorm, one wave per token
//   enc_gemm_kernel<EPI>  C = A . W^T + bias on MFMA 16x16x32: 128 x 128 x 64 tiles, 4 waves,
//                         LDS-DMA staged, XOR-swizzled 128-B rows (same scheme as K2); epilogues
//                         fused: bias | bias + erf-GELU | bias + residual
//   enc_attention_kernel  per (batch, head, 64 query rows): flash-style loop over 64-key blocks,
//                         QK^T and PV on MFMA, online softmax in the accumulator layout
//                         (row = (lane>>4)*4+j, reduced over the 16 lanes of a row by shuffles),
//                         P staged through LDS as the next MFMA's A operand, V transposed on store
//   enc_ln_kernel         LayerNorm (the residual add is in the GEMM epilogue)
//   enc_pool_kernel       masked mean or CLS, optional L2 normalisation, fp32 out
// MFMA-bound (~170 MFLOP/token for bge-base); LN/softmax/GELU ride in epilogues.
#include "common.h"

#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include <type_traits>
#include <map>
#include <string>

namespace mrag {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_vptr;
typedef const __attribute__((address_space(1))) void* glb_vptr;

template <int DT> struct EMfma;
template <> struct EMfma<MRAG_F16> {
  typedef f16x8 frag;
  typedef _Float16 elem;
  static __device__ __forceinline__ f32x4 run(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <> struct EMfma<MRAG_BF16> {
  typedef bf16x8 frag;
  typedef __bf16 elem;
  static __device__ __forceinline__ f32x4 run(frag a, frag b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

// erf-GELU (HF "gelu") with erf from Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7; 4.7e-7 on the GELU
// value in fp32, three orders below the fp16 rounding of the stored activation): ~13 VALU ops instead
// of libm erff's ~40 -- at K = 768 the FFN-up epilogue is as long as its MFMA loop otherwise.
__device__ __forceinline__ float gelu_erf(float v) {
  // constants folded: b = |v| sqrt(log2 e / 2) so that exp(-v^2 / 2) = exp2(-b^2) (no separate log2 e multiply), the
  // 0.3275911 of t = 1 / (1 + 0.3275911 |v| / sqrt 2) rescaled to b, the 0.5 of 0.5 erfc folded into the polynomial
  const float b = fabsf(v) * 0.84932180028801904f;                     // sqrt(log2(e) / 2)
  const float t = __builtin_amdgcn_rcpf(fmaf(0.27273748087922250f, b, 1.0f));   // 0.3275911 / sqrt(log2 e)
  float p = fmaf(0.5307027145f, t, -0.7265760135f);
  p = fmaf(p, t, 0.7107068705f);
  p = fmaf(p, t, -0.142248368f);
  p = fmaf(p, t, 0.127414796f);
  const float h = p * t * __builtin_amdgcn_exp2f(-b * b);              // 0.5 * erfc(|v| / sqrt 2)
  // v >= 0: v - v h;  v < 0: v h = -|v| h  ==  max(v, 0) - |v| h for both signs (one fma), without a compare + select per
  // element (a v_cmp into an SGPR pair, a wait state, a v_cndmask)
  return fmaf(-fabsf(v), h, fmaxf(v, 0.f));
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

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

template <typename E>
static void launch_ln(const E* x, int64_t n_tok, int H, const float* g, const float* b, float eps, E* out, dim3 grid, dim3 block,
                      hipStream_t stream) {
  if (H % 8 == 0 && H <= 2048) hipLaunchKernelGGL((enc_ln_vec_kernel<E>), grid, block, 0, stream, x, n_tok, H, g, b, eps, out);
  else hipLaunchKernelGGL((enc_ln_kernel<E>), grid, block, 0, stream, x, n_tok, H, g, b, eps, out);
}

// ------------------------------------------------------------------ GEMM with fused epilogues
constexpr int GM = 128, GN = 128, GK = 64, GTHR = 256;
constexpr int G_A_BYTES = GM * GK * 2;             // 16 KiB
constexpr int G_STAGE = (GM + GN) * GK * 2;        // 32 KiB
enum { EPI_BIAS = 0, EPI_GELU = 1, EPI_RESID = 2 };

// A [M_pad][K], W [N_pad][K] (both K-contiguous, K % 64 == 0, M_pad % 128 == 0, N_pad % 128 == 0),
// C [M_pad][N] (only columns < N are written), R same shape as C.
template <int DT, int EPI>
__global__ __launch_bounds__(GTHR) void enc_gemm_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ W,
                                                        const float* __restrict__ bias, const uint16_t* __restrict__ R,
                                                        uint16_t* __restrict__ C, int M_pad, int N, int K, int n_tiles_n) {
  typedef typename EMfma<DT>::frag frag;
  typedef typename EMfma<DT>::elem elem;
  __shared__ __attribute__((aligned(16))) char sm[2 * G_STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;
  // XCD-aware: consecutive blocks of one XCD walk N first so they share the A row panel in L2
  const int nblk = gridDim.x, b = blockIdx.x;
  const int lin = (nblk % 8 == 0) ? (b & 7) * (nblk / 8) + (b >> 3) : b;   // bijective only when nblk % 8 == 0
  const int tm = lin / n_tiles_n, tn = lin - tm * n_tiles_n;

  int src_off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (4 * w + i) * 8 + (lane >> 3);
    const int kc = (lane & 7) ^ ((r >> 1) & 7);
    src_off[i] = r * K + kc * 8;
  }
  const uint16_t* a0 = A + (size_t)tm * GM * K;
  const uint16_t* w0 = W + (size_t)tn * GN * K;
  auto stage = [&](int kk, int buf) {
    char* la = sm + buf * G_STAGE + (4 * w) * 1024;
    char* lb = la + G_A_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((glb_vptr)(a0 + kk * GK + src_off[i]), (lds_vptr)(la + i * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((glb_vptr)(w0 + kk * GK + src_off[i]), (lds_vptr)(lb + i * 1024), 16, 0, 0);
  };
  const int frow = lane & 15, fsw = frow >> 1;
  const int a_rd = (wm * 64 + frow) * 128, b_rd = G_A_BYTES + (wn * 64 + frow) * 128;
  const int ph0 = ((lane >> 4) ^ fsw) * 16;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nk = K / GK;
  stage(0, 0);
  __syncthreads();
  for (int kk = 0; kk < nk; ++kk) {
    const int buf = kk & 1;
    if (kk + 1 < nk) stage(kk + 1, buf ^ 1);
    const char* sb = sm + buf * G_STAGE;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int ph = ks ? (ph0 ^ 64) : ph0;
      frag af[4], bf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = *(const frag*)(sb + a_rd + i * 2048 + ph);
#pragma unroll
      for (int j = 0; j < 4; ++j) bf[j] = *(const frag*)(sb + b_rd + j * 2048 + ph);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = EMfma<DT>::run(af[i], bf[j], acc[i][j]);
    }
    __syncthreads();
  }
  // epilogue: C[row][col], row = tm*128 + wm*64 + i*16 + (lane>>4)*4 + r, col = tn*128 + wn*64 + j*16 + (lane&15)
  const int row_b = tm * GM + wm * 64 + (lane >> 4) * 4;
  const int col_b = tn * GN + wn * 64 + (lane & 15);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = col_b + j * 16;
    if (col >= N) continue;
    const float bv = bias[col];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t off = (size_t)(row_b + i * 16 + r) * N + col;
        float v = acc[i][j][r] + bv;
        if (EPI == EPI_GELU) v = gelu_erf(v);
        if (EPI == EPI_RESID) { elem rr; __builtin_memcpy(&rr, &R[off], 2); v += (float)rr; }
        const elem o = (elem)v;
        __builtin_memcpy(&C[off], &o, 2);
      }
  }
}

// ------------------------------------------------------------------ skinny GEMM: <= 64 tokens (one question at a time)
// The reference embeds ONE question per call (retrieval_backend.py:227): 16-64 tokens against 170 MB of weights.  With
// 128 x 128 tiles that is 6-24 workgroups per GEMM, each walking K serially (12-48 K steps of one cold round trip each):
// ~85 us per layer.  Here a workgroup owns 16 output columns and its four waves a QUARTER OF K each (fragments straight from
// global memory into the MFMA operand layout, two 3-step chunks in flight), partial sums are added in LDS in wave order
// (deterministic) and the epilogue stores 8-byte groups: N / 16 workgroups (48-192), a handful of round trips each.
template <int DT, int EPI, int NFR>
__global__ __launch_bounds__(256) void enc_gemm_skinny_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ W,
                                                              const float* __restrict__ bias, const uint16_t* __restrict__ R,
                                                              uint16_t* __restrict__ C, int N, int K) {
  typedef typename EMfma<DT>::frag frag;
  typedef typename EMfma<DT>::elem elem;
  typedef elem e4 __attribute__((ext_vector_type(4)));
  constexpr int CH = 3;                                   // K steps (of 32) per chunk; K / 128 is a multiple of 3 for every BERT width
  __shared__ f32x4 part[4][NFR][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane >> 4, i16 = lane & 15;
  const int n0 = blockIdx.x * 16;
  const int ksw = K / 128;                                // K steps of this wave
  const uint16_t* wp = W + (size_t)(n0 + i16) * K + (size_t)w * (K / 4) + g * 8;
  const uint16_t* xp = X + (size_t)i16 * K + (size_t)w * (K / 4) + g * 8;
  f32x4 acc[NFR];
#pragma unroll
  for (int nf = 0; nf < NFR; ++nf) acc[nf] = (f32x4){0.f, 0.f, 0.f, 0.f};
  frag a[2][CH], b[2][CH][NFR];
  auto load = [&](int buf, int c) {
#pragma unroll
    for (int s = 0; s < CH; ++s) {
      a[buf][s] = *(const frag*)(wp + (c * CH + s) * 32);
#pragma unroll
      for (int nf = 0; nf < NFR; ++nf) b[buf][s][nf] = *(const frag*)(xp + (size_t)nf * 16 * K + (c * CH + s) * 32);
    }
  };
  const int nch = ksw / CH;
  load(0, 0);
#pragma unroll 1
  for (int c = 0; c < nch; c += 2) {
    if (c + 1 < nch) load(1, c + 1);
#pragma unroll
    for (int s = 0; s < CH; ++s)
#pragma unroll
      for (int nf = 0; nf < NFR; ++nf) acc[nf] = EMfma<DT>::run(a[0][s], b[0][s][nf], acc[nf]);
    if (c + 1 < nch) {
      if (c + 2 < nch) load(0, c + 2);
#pragma unroll
      for (int s = 0; s < CH; ++s)
#pragma unroll
        for (int nf = 0; nf < NFR; ++nf) acc[nf] = EMfma<DT>::run(a[1][s], b[1][s][nf], acc[nf]);
    }
  }
#pragma unroll
  for (int nf = 0; nf < NFR; ++nf) part[w][nf][lane] = acc[nf];
  __syncthreads();
  // fragment nf is finished by wave nf % 4: partials added in wave order 0..3; lane holds columns n0 + 4 g + r of token 16 nf + i16
  for (int nf = w; nf < NFR; nf += 4) {
    f32x4 v = part[0][nf][lane];
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) { const f32x4 o = part[ww][nf][lane]; v[0] += o[0]; v[1] += o[1]; v[2] += o[2]; v[3] += o[3]; }
    const int n = n0 + 4 * g, token = nf * 16 + i16;
    if (n >= N) continue;
    const float4 bv = *(const float4*)(bias + n);
    float o4[4] = {v[0] + bv.x, v[1] + bv.y, v[2] + bv.z, v[3] + bv.w};
    if (EPI == EPI_GELU) {
#pragma unroll
      for (int r = 0; r < 4; ++r) o4[r] = gelu_erf(o4[r]);
    }
    if (EPI == EPI_RESID) {
      const e4 rr = *(const e4*)(R + (size_t)token * N + n);
#pragma unroll
      for (int r = 0; r < 4; ++r) o4[r] += (float)rr[r];
    }
    e4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = (elem)o4[r];
    *(e4*)(C + (size_t)token * N + n) = o;
  }
}

// ------------------------------------------------------------------ 256 x 256 persistent GEMM (the K2 main loop)
// Used when N_pad % 256 == 0 and M_pad % 256 == 0.  Same structure as the similarity kernel of
// bf_batch.hip: 8 waves (2 x 4), 256 x 256 x 64 stages through LDS-DMA issued from inline asm (scalar
// base + 32-bit voffset, XOR swizzle on the source address), two fragment register sets so that the
// MFMA pipe never waits on a read it has just issued, zero C operand on the first K step of a tile,
// one barrier per K step.  Workgroups are persistent: each walks tiles lin = first, first + stride, ...
// and prefetches the first stage of its next tile during the last K step of the current one.
// The WEIGHT rows are the MFMA A operand and the token rows the B operand, so a lane's four accumulator
// values are four consecutive OUTPUT columns of one token: bias / GELU / residual apply to 8-byte
// groups and the stores are 8 bytes per lane (the 128 x 128 kernel above stores 2 bytes at a time).
constexpr int G2_T = 256, G2_THR = 512;
constexpr int G2_A_BYTES = G2_T * GK * 2;            // 32 KiB: weight rows of a stage
constexpr int G2_STAGE = 2 * G2_A_BYTES;             // 64 KiB
constexpr int G2_PAD = 4096;                          // between the two stage buffers: either buffer + the pad holds the
constexpr int G2_BUF1 = G2_STAGE + G2_PAD;            // epilogue's 128 x 528-byte output slab
constexpr int G2_VEC = 2048;                          // behind the stage buffers: bias / gamma of the tile's 256 columns (LNR epilogue)
constexpr int G2_CPITCH = 528;                        // output row pitch in LDS: 256 columns x 2 B + 16 (bank shift per row)
// Wave roles: waves 0-3 (one per SIMD) issue every LDS-DMA of the K loop, waves 4-7 every global store of the epilogue.
// vmcnt counts a wave's loads and stores in issue order, so a wave that does both sits out its output stores (128 KiB per
// CU, all CUs at once: the HBM write rate) at the next stage wait; with the roles split the loading waves never have a
// store outstanding and the storing waves never wait on vmcnt inside the K loop.
constexpr int G2_CPW = 8;                             // 1-KiB chunks of each operand stage a loading wave fills
constexpr int G2_PS = 2048;                           // the loading waves' LayerNorm partial sums pass through LDS to the storing waves
constexpr int G2_LDS = 2 * G2_STAGE + G2_PAD + G2_VEC + G2_PS;   // 134 KiB

// LayerNorm folded into the GEMMs around it (LNF flags; forward_impl, "fused LayerNorm" flow):
//   1 LNA   the A operand is the PRE-LayerNorm tensor y and W holds gamma-scaled weights W' = gamma o W:
//           out = rstd_t (y W'^T - mu_t s_n) + c_n   with s_n = sum_k W'[n][k], c_n = b_n + sum_k beta_k W[n][k] (in `bias`)
//   2 LNR   the residual R is a pre-LayerNorm tensor: the epilogue adds (R - mu_t) rstd_t gamma_n (beta is folded into `bias`)
//   4 STATS the epilogue also emits, per token, partial (sum, sum of squares) of the values it stores (as rounded)
// so that a LayerNorm between two GEMMs never makes its own pass over HBM (2 x 0.8 GB per layer at H = 768).
struct LnArgs {
  const float* a_stats;   // LNA: (mu, rstd) per token
  const float* s_vec;     // LNA: s_n per output column
  const float* r_stats;   // LNR: (mu, rstd) per token of the residual's LayerNorm
  const float* r_gamma;   // LNR: its gamma
  float* partials;        // STATS: [token][np][2]
  int np;                 // STATS: partial slots per token = 2 x column tiles
};

template <int DT, int EPI, int LNF>
__global__ __launch_bounds__(G2_THR, 2) void enc_gemm256_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ W,
                                                                const float* __restrict__ bias, const uint16_t* __restrict__ R,
                                                                uint16_t* __restrict__ C, int N, int K, int tiles_m, int tiles_n,
                                                                LnArgs ln) {
  typedef typename EMfma<DT>::frag frag;
  typedef typename EMfma<DT>::elem elem;
  typedef elem e4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) char sm2[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 2, wn = w & 3;     // wave tile: 128 weight rows (output columns) x 64 tokens
  const int ksteps = K / GK;
  const int n_tiles = tiles_m * tiles_n;
  // XCD-aware start: the workgroups of one XCD (blockIdx % 8) take consecutive tiles, which walk N first
  // and share the token panel in that XCD's L2
  const int nwg = gridDim.x;
  const int first = (nwg % 8 == 0) ? (int)(blockIdx.x & 7) * (nwg / 8) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  const uint32_t row_b = (uint32_t)K * 2u;
  const uint32_t voff_e = (uint32_t)(lane >> 3) * row_b + (uint32_t)(((lane & 7) ^ (lane >> 4)) * 16);
  const uint32_t voff_o = (uint32_t)(lane >> 3) * row_b + (uint32_t)(((lane & 7) ^ (4 + (lane >> 4))) * 16);
  const uint32_t chunk_b = 8u * row_b;
  const bool loader = w < 4;                             // (wave-uniform)
  const bool storer = w >= 4;
  const size_t wave_off = (size_t)(G2_CPW * (w & 3)) * chunk_b;     // loading wave w fills 1-KiB chunks 8w..8w+7 of each operand
  auto tile_ptrs = [&](int lin, const char*& a, const char*& b) {
    const int tm = lin / tiles_n, tn = lin - tm * tiles_n;
    a = (const char*)(W + (size_t)tn * G2_T * K) + wave_off;
    b = (const char*)(X + (size_t)tm * G2_T * K) + wave_off;
  };
  auto stage = [&](const char* a, const char* b, int buf) {
    if (!loader) return;
#pragma unroll
    for (int op = 0; op < 2; ++op) {
      const char* base = op ? b : a;
#pragma unroll
      for (int i = 0; i < G2_CPW; i += 2) {
        const uint32_t la = (uint32_t)(buf * G2_BUF1 + op * G2_A_BYTES + (G2_CPW * (w & 3) + i) * 1024);
        const char* c0 = base + (size_t)i * chunk_b;
        const char* c1 = c0 + chunk_b;
        uint32_t keep;
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\t"
            "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %4\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(voff_e), "v"(voff_o), "s"(c0), "s"(c1), "s"(la)
            : "memory", "scc");
      }
    }
  };
  const int frow = lane & 15, fsw = frow >> 1;
  const int a_rd = (wm * 128 + frow) * 128;
  const int b_rd = G2_A_BYTES + (wn * 64 + frow) * 128;
  const int ph0 = ((lane >> 4) ^ fsw) * 16;
  f32x4 acc[8][4];
  frag f1a[8], f1b[4];

  // prefetch cursor over the flattened (tile, k step) sequence of this workgroup
  int pf_lin = first, pf_kk = 0;
  const char *pf_a = nullptr, *pf_b = nullptr;
  if (pf_lin < n_tiles) tile_ptrs(pf_lin, pf_a, pf_b);
  int buf = 0;
  auto prefetch = [&](int into) {
    if (pf_lin >= n_tiles) return;
    stage(pf_a + pf_kk * (GK * 2), pf_b + pf_kk * (GK * 2), into);
    if (++pf_kk == ksteps) {
      pf_kk = 0;
      pf_lin += nwg;
      if (pf_lin < n_tiles) tile_ptrs(pf_lin, pf_a, pf_b);
    }
  };
  prefetch(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  auto kstep = [&](auto pending_tag) {
    constexpr bool PENDING = decltype(pending_tag)::value;
    prefetch(buf ^ 1);
    const char* sb = sm2 + buf * G2_BUF1;
    buf ^= 1;
    const int ph1 = ph0 ^ 64;
    frag f0a[8], f0b[4];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) f0b[nf] = *(const frag*)(sb + b_rd + nf * 2048 + ph0);
#pragma unroll
    for (int mf = 0; mf < 8; ++mf) f0a[mf] = *(const frag*)(sb + a_rd + mf * 2048 + ph0);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (PENDING) {
#pragma unroll
      for (int mf = 0; mf < 8; ++mf)
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) acc[mf][nf] = EMfma<DT>::run(f1a[mf], f1b[nf], acc[mf][nf]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) f1b[nf] = *(const frag*)(sb + b_rd + nf * 2048 + ph1);
#pragma unroll
    for (int mf = 0; mf < 8; ++mf) f1a[mf] = *(const frag*)(sb + a_rd + mf * 2048 + ph1);
#pragma unroll
    for (int mf = 0; mf < 8; ++mf)
#pragma unroll
      for (int nf = 0; nf < 4; ++nf)
        acc[mf][nf] = EMfma<DT>::run(f0a[mf], f0b[nf], PENDING ? acc[mf][nf] : (f32x4){0.f, 0.f, 0.f, 0.f});
#define MRAG_SGB(n_rd) __builtin_amdgcn_sched_group_barrier(0x008, 4, 0); __builtin_amdgcn_sched_group_barrier(0x100, n_rd, 0);
    MRAG_SGB(2) MRAG_SGB(1) MRAG_SGB(2) MRAG_SGB(1) MRAG_SGB(2) MRAG_SGB(1) MRAG_SGB(2) MRAG_SGB(1)
#undef MRAG_SGB
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  auto kstep_sync = [&]() {
    if (loader) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the storing waves' output stores stay in flight
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  for (int lin = first; lin < n_tiles; lin += nwg) {
    kstep(std::false_type{});
    for (int kk = 1; kk < ksteps; ++kk) {
      kstep_sync();
      kstep(std::true_type{});
    }
#pragma unroll
    for (int mf = 0; mf < 8; ++mf)
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) acc[mf][nf] = EMfma<DT>::run(f1a[mf], f1b[nf], acc[mf][nf]);
    // the next tile's first stage is in flight: make sure it has landed BEFORE this tile's stores are
    // issued (vmcnt counts in order), so that the barrier below does not wait for the stores
    if (loader) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // ---- epilogue: n = tn*256 + wm*128 + mf*16 + (lane>>4)*4 + r, token = tm*256 + wn*64 + nf*16 + (lane&15).
    // The tile goes out through LDS in two passes of 128 tokens (nf = 2p, 2p+1): every lane writes its
    // 8-byte groups into a [token][column] slab (the stage buffer just consumed + the pad), then all 512
    // threads store the slab as 16-byte pieces of whole 512-byte rows.  Storing the 8-byte groups
    // straight from the accumulator layout touches 16 cache lines per instruction (QKV GEMM 1.15 -> 1.01 ms).
    const int tm = lin / tiles_n, tn = lin - tm * tiles_n;
    char* slab = sm2 + ((buf ^ 1) ? G2_STAGE : 0);          // free buffer: buffer 0 + pad, or pad + buffer 1
    const int n_l = wm * 128 + (lane >> 4) * 4;             // + mf*16: column inside the tile
    const int n_b = tn * G2_T + n_l;
    const int t_b = tm * G2_T + wn * 64 + (lane & 15);
    // Every global load of the epilogue is issued HERE, back to back, and waited for once: written inside the
    // passes, hipcc puts an s_waitcnt vmcnt(0) behind each of them (8 bias + 32 residual loads = up to 40 serial
    // L2 round trips per tile), and in pass 1 that wait also sits out pass 0's stores (vmcnt counts in order).
    constexpr bool VEC_LDS = (LNF & 2) != 0;     // LNR: bias and gamma of the tile's columns live in LDS (the register budget:
                                                 // 128 accumulators + the 64 residual registers leave no room for two more vectors)
    float* vec = (float*)(sm2 + 2 * G2_STAGE + G2_PAD);
    if (VEC_LDS && tid < 128) {
      const int n0 = tn * G2_T + (tid & 63) * 4;
      float4 t4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n0 < N) t4 = *(const float4*)((tid < 64 ? bias : ln.r_gamma) + n0);
      *(float4*)(vec + (tid >> 6) * 256 + (tid & 63) * 4) = t4;     // (visible after the barrier below)
    }
    float4 bv[VEC_LDS ? 1 : 8];
    float4 xv[((LNF & 3) && !VEC_LDS) ? 8 : 1];  // LNA: s_n (LNR: gamma_n, in LDS)
    e4 rr[8][4];
    float2 tst[(LNF & 3) ? 4 : 1];              // (mu, rstd) of this lane's four tokens
    float ps1[(LNF & 4) ? 4 : 1], ps2[(LNF & 4) ? 4 : 1];
    if (LNF & 3) {
      const float2* st = (const float2*)((LNF & 1) ? ln.a_stats : ln.r_stats);
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) tst[nf] = st[t_b + nf * 16];
    }
    if (LNF & 4) {
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) { ps1[nf] = 0.f; ps2[nf] = 0.f; }
    }
#pragma unroll
    for (int mf = 0; mf < 8; ++mf) {
      const int n0 = n_b + mf * 16;
      if (!VEC_LDS) {
        bv[mf] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n0 < N) bv[mf] = *(const float4*)(bias + n0);
      }
      if ((LNF & 3) && !VEC_LDS) {
        xv[mf] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n0 < N) xv[mf] = *(const float4*)(ln.s_vec + n0);
      }
      if (EPI == EPI_RESID) {
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
          rr[mf][nf] = (e4){(elem)0.f, (elem)0.f, (elem)0.f, (elem)0.f};
          if (n0 < N) rr[mf][nf] = *(const e4*)(R + (size_t)(t_b + nf * 16) * N + n0);
        }
      }
    }
    if (VEC_LDS) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the bias / gamma vectors are in LDS before anyone passes the barrier
    __builtin_amdgcn_s_barrier();   // every wave has read its last fragments out of the buffer the slab reuses (lgkmcnt(0) in kstep)
    asm volatile("" ::: "memory");
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
      for (int mf = 0; mf < 8; ++mf) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int nf = pass * 2 + h;
          const float4 b4 = VEC_LDS ? *(const float4*)(vec + n_l + mf * 16) : bv[VEC_LDS ? 0 : mf];
          const float bq[4] = {b4.x, b4.y, b4.z, b4.w};
          float v[4];
          if (LNF & 1) {
            const float xq[4] = {xv[mf].x, xv[mf].y, xv[mf].z, xv[mf].w};
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = tst[nf].y * (acc[mf][nf][r] - tst[nf].x * xq[r]) + bq[r];
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[mf][nf][r] + bq[r];
          }
          if (EPI == EPI_GELU) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = gelu_erf(v[r]);
          }
          if (EPI == EPI_RESID) {
            if (LNF & 2) {
              const float4 g4 = *(const float4*)(vec + 256 + n_l + mf * 16);
              const float xq[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
              for (int r = 0; r < 4; ++r) v[r] += ((float)rr[mf][nf][r] - tst[nf].x) * tst[nf].y * xq[r];
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r) v[r] += (float)rr[mf][nf][r];
            }
          }
          e4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = (elem)v[r];
          if ((LNF & 4) && n_b + mf * 16 < N) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float f = (float)o[r]; ps1[nf] += f; ps2[nf] += f * f; }
          }
          const int tl = wn * 32 + h * 16 + (lane & 15);    // token row inside the pass
          *(e4*)(slab + tl * G2_CPITCH + (n_l + mf * 16) * 2) = o;
        }
      }
      // raw barriers behind LDS-only waits: the global stores below stay in flight across them (a
      // __syncthreads() here drains them: a full HBM write round trip per pass with every CU storing at once)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      // roles: the 256 threads of waves 4-7 store the slab, 16 pieces each.  Thread -> (row r0 + 8 i, piece): the piece and r0
      // are fixed per thread, so every store is lane offset + a wave-uniform base (no per-store address registers: the
      // hoisted 64-bit addresses of a plain store loop spill).  The stores are asm so that hipcc neither counts them nor waits.
      if (storer) {
        const int r0 = (tid - 256) >> 5, piece = tid & 31;
        const int n0 = tn * G2_T + piece * 8;
        const uint32_t lane_off = ((uint32_t)r0 * (uint32_t)N + (uint32_t)(piece * 8)) * 2u;
        const char* srow = slab + r0 * G2_CPITCH + piece * 16;
        if (n0 < N) {
#pragma unroll
          for (int g = 0; g < 16; g += 4) {          // four slab reads in flight, then their four stores
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            u32x4 vv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const uint4 val = *(const uint4*)(srow + (g + j) * 8 * G2_CPITCH);
              vv[j] = (u32x4){val.x, val.y, val.z, val.w};
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int i = g + j;
              const int tok0 = tm * G2_T + (i >> 2) * 64 + pass * 32 + 8 * (i & 3);      // + r0: in lane_off
              const char* base = (const char*)(C + (size_t)tok0 * N + (size_t)tn * G2_T);
              // non-temporal: the output is streamed once, it must not evict the operand panels from L2
              asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 nt\n\ts_nop 1" ::"v"(lane_off), "v"(vv[j]), "s"(base) : "memory");
            }
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // slab reads done (pass 1 rewrites it; after pass 1 the next stage lands in it)
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
    if (LNF & 4) {
      // the four lane groups (lane >> 4) of a wave hold different columns of the SAME tokens: add them up, then one lane per
      // token writes the wave's partial -- slot 2 tn + wm of the token (finalised by enc_ln_stats_kernel in slot order)
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) {
        ps1[nf] += __shfl_xor(ps1[nf], 16); ps1[nf] += __shfl_xor(ps1[nf], 32);
        ps2[nf] += __shfl_xor(ps2[nf], 16); ps2[nf] += __shfl_xor(ps2[nf], 32);
      }
      // waves w and w + 4 hold the two column halves (wm = 0 / 1) of the same 64 tokens: the loading wave hands its sums
      // over through LDS and the storing wave writes both slots (the loading waves issue no global store at all)
      float2* psl = (float2*)(sm2 + 2 * G2_STAGE + G2_PAD + G2_VEC);
      if (!storer && lane < 16) {
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) psl[wn * 64 + nf * 16 + lane] = make_float2(ps1[nf], ps2[nf]);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (storer && lane < 16) {
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
          float2* dst = (float2*)ln.partials + (size_t)(t_b + nf * 16) * ln.np + 2 * tn;
          dst[0] = psl[wn * 64 + nf * 16 + lane];
          dst[1] = make_float2(ps1[nf], ps2[nf]);
        }
      }
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

// ------------------------------------------------------------------ attention
constexpr float ENC_NO_KEY = -3.0e38f;   // score bias of a key slot beyond the sequence (finite: exp(ENC_NO_KEY - max) == 0 for any max >= -1e30)
// QKV [M_pad][3H] (q | k | v per token), mask [B][S] (1 = token), out [M_pad][H].
// grid = B * heads * ceil(S/64); 256 threads: wave w owns query rows 16w..16w+15 of the block.
// NW waves = 16 * NW query rows per workgroup; the launcher uses 8 waves (128 rows), so that 128 queries stage their
// K / V blocks once instead of once per 64-row half (attention 0.59 -> see DESIGN).
template <int DT, int DH, int NW>
__global__ __launch_bounds__(64 * NW) void enc_attention_kernel(const uint16_t* __restrict__ qkv, const int32_t* __restrict__ mask,
                                                                uint16_t* __restrict__ out, int B, int S, int H, int heads, float scale) {
  constexpr int QB = 16 * NW, NT_ = 64 * NW;
  typedef typename EMfma<DT>::frag frag;
  typedef typename EMfma<DT>::elem elem;
  constexpr int KB = 64;                       // keys per block
  constexpr int NK = DH / 32;                  // k-steps of the QK^T contraction
  constexpr int ND = DH / 16;                  // 16-column groups of the output
  __shared__ __attribute__((aligned(16))) elem sK[KB][DH + 8];       // [key][dh]   (+8: 16-B pad against bank conflicts)
  __shared__ __attribute__((aligned(16))) elem sVt[DH][KB + 8];      // [dh][key]
  __shared__ __attribute__((aligned(16))) elem sP[NW][16][KB + 8];   // per wave [q row][key]
  __shared__ float sBias[KB];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nqb = (S + QB - 1) / QB;
  const int qb = blockIdx.x % nqb;
  const int hh = (blockIdx.x / nqb) % heads;
  const int bb = blockIdx.x / (nqb * heads);
  const size_t ld = (size_t)3 * H;
  const uint16_t* base = qkv + (size_t)bb * S * ld;
  const int q_row = qb * QB + w * 16 + (lane & 15);           // A operand row of this lane
  // Q fragments: lane holds Q[q_row][k = 32*ks + 8*(lane>>4) + j]
  frag qf[NK];
#pragma unroll
  for (int ks = 0; ks < NK; ++ks) {
    frag z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (elem)0.f;
    if (q_row < S) z = *(const frag*)(base + (size_t)q_row * ld + hh * DH + ks * 32 + (lane >> 4) * 8);
    qf[ks] = z;
  }
  f32x4 o[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) o[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m_run[4], l_run[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_run[r] = -1e30f; l_run[r] = 0.f; }

  for (int k0 = 0; k0 < S; k0 += KB) {
    __syncthreads();
    // stage K (row-major) and V (transposed) of this key block; 256 threads x 16 B = one 64 x 32 slab per pass
    for (int e = tid; e < KB * (DH / 8); e += NT_) {
      const int key = e / (DH / 8), c = e % (DH / 8);
      frag kv, vv;
#pragma unroll
      for (int j = 0; j < 8; ++j) { kv[j] = (elem)0.f; vv[j] = (elem)0.f; }
      if (k0 + key < S) {
        kv = *(const frag*)(base + (size_t)(k0 + key) * ld + H + hh * DH + c * 8);
        vv = *(const frag*)(base + (size_t)(k0 + key) * ld + 2 * H + hh * DH + c * 8);
      }
      *(frag*)&sK[key][c * 8] = kv;
#pragma unroll
      for (int j = 0; j < 8; ++j) sVt[c * 8 + j][key] = vv[j];
    }
    // masked keys get -1e30 (a row with no valid key attends all S of them evenly, as the oracle does); slots beyond S get
    // ENC_NO_KEY, far enough below that to vanish from that row's softmax as well
    if (tid < KB) sBias[tid] = k0 + tid >= S ? ENC_NO_KEY : mask[(size_t)bb * S + k0 + tid] != 0 ? 0.f : -1e30f;
    __syncthreads();
    // S = Q K^T  (16 q rows x 64 keys per wave): B operand lane holds K[key = 16*nf + (lane&15)][k chunk]
    f32x4 sc[4];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      sc[nf] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NK; ++ks) {
        const frag kf = *(const frag*)&sK[nf * 16 + (lane & 15)][ks * 32 + (lane >> 4) * 8];
        sc[nf] = EMfma<DT>::run(qf[ks], kf, sc[nf]);
      }
    }
    // online softmax: this lane's rows are (lane>>4)*4 + r, its columns 16*nf + (lane&15)
    float p[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = -1e30f;
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) {
        const float v = sc[nf][r] * scale + sBias[nf * 16 + (lane & 15)];
        p[nf][r] = v;
        mx = fmaxf(mx, v);
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
      const float m_new = fmaxf(m_run[r], mx);
      const float alpha = __expf(m_run[r] - m_new);
      float rs = 0.f;
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) {
        const float e = __expf(p[nf][r] - m_new);
        p[nf][r] = e;
        rs += e;
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) rs += __shfl_xor(rs, off);
      l_run[r] = l_run[r] * alpha + rs;
      m_run[r] = m_new;
#pragma unroll
      for (int d = 0; d < ND; ++d) o[d][r] *= alpha;
    }
    // P -> LDS (this wave's 16 x 64 slab), then O += P V
#pragma unroll
    for (int nf = 0; nf < 4; ++nf)
#pragma unroll
      for (int r = 0; r < 4; ++r) sP[w][(lane >> 4) * 4 + r][nf * 16 + (lane & 15)] = (elem)p[nf][r];
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's own LDS writes are visible to its reads
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ks = 0; ks < KB / 32; ++ks) {
      const frag pf = *(const frag*)&sP[w][lane & 15][ks * 32 + (lane >> 4) * 8];
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const frag vf = *(const frag*)&sVt[d * 16 + (lane & 15)][ks * 32 + (lane >> 4) * 8];
        o[d] = EMfma<DT>::run(pf, vf, o[d]);
      }
    }
  }
  // out[row][hh*DH + 16*d + (lane&15)], row = qb*QB + w*16 + (lane>>4)*4 + r.  The wave's 16 x DH block goes
  // through its (now idle) P slab so that it leaves as 16-byte pieces of whole DH-wide rows instead of
  // sixteen 2-byte stores per lane.
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float inv = 1.0f / l_run[r];
#pragma unroll
    for (int d = 0; d < ND; ++d) sP[w][(lane >> 4) * 4 + r][d * 16 + (lane & 15)] = (elem)(o[d][r] * inv);
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
  constexpr int PIECES = DH / 8;                 // 16-byte pieces per row
  for (int e = lane; e < 16 * PIECES; e += 64) {
    const int rr = e / PIECES, pc = e % PIECES;
    const int row = qb * QB + w * 16 + rr;
    if (row < S) *(frag*)&out[((size_t)bb * S + row) * H + hh * DH + pc * 8] = *(const frag*)&sP[w][rr][pc * 8];
  }
}

// ------------------------------------------------------------------ attention, sequences of <= 256 tokens
// One workgroup (4 waves) per (batch, head): K and V of the head are staged ONCE, row-major, with all global loads in flight
// together; every wave then owns 32 query rows (two 16-row MFMA groups) against all 128 (padded) keys -- no key-block loop, no
// online-softmax rescaling, no per-block barriers.  The two operands whose contraction index runs along LDS ROWS come from
// gfx950's transposing LDS read (ds_read_b64_tr_b16, cdna_hip_programming.md T10):
//   V  [key][dh]  -> B operand of P V   (lane n = dh column, 8 consecutive keys): two reads of a 4-key x 16-column block
//   P^T[key][row] -> A operand of P V   (lane m = query row, 8 consecutive keys): the accumulator layout of Q K^T already holds
//                    4 consecutive rows of one key per lane, so P goes to LDS as ONE 8-byte store per accumulator (the
//                    generic kernel above writes sixteen 2-byte stores per lane and block, and eight per V chunk).
// Row reductions of the softmax stay inside a 16-lane DPP row (row_ror), no LDS permutes.
typedef short tr_s4 __attribute__((ext_vector_type(4)));
template <typename F>
__device__ __forceinline__ F tr_read_pair(const void* lo_ptr, const void* hi_ptr) {
  typedef __attribute__((address_space(3))) tr_s4* lp;
  union { tr_s4 h[2]; F f; } u;
  u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)lo_ptr);
  u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)hi_ptr);
  return u.f;
}
template <int N>
__device__ __forceinline__ float dpp_ror16(float x) {   // value of the lane N places further round its 16-lane row
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x120 + N, 0xF, 0xF, false));
}
__device__ __forceinline__ float row16_max(float x) {
  x = fmaxf(x, dpp_ror16<8>(x)); x = fmaxf(x, dpp_ror16<4>(x)); x = fmaxf(x, dpp_ror16<2>(x)); return fmaxf(x, dpp_ror16<1>(x));
}
__device__ __forceinline__ float row16_sum(float x) {
  x += dpp_ror16<8>(x); x += dpp_ror16<4>(x); x += dpp_ror16<2>(x); return x + dpp_ror16<1>(x);
}

// SP = padded key count (64 / 128 / 256), NW waves; every wave owns SP / NW query rows (groups of 16).
template <int DT, int DH, int SP, int NW>
__global__ __launch_bounds__(64 * NW) void enc_attention_s128_kernel(const uint16_t* __restrict__ qkv, const int32_t* __restrict__ mask,
                                                                     uint16_t* __restrict__ out, int B, int S, int H, int heads, float scale) {
  typedef typename EMfma<DT>::frag frag;
  typedef typename EMfma<DT>::elem elem;
  typedef elem e4 __attribute__((ext_vector_type(4)));
  constexpr int NT_ = 64 * NW;
  constexpr int NK = DH / 32;                  // k steps of Q K^T
  constexpr int ND = DH / 16;                  // 16-column groups of the output
  constexpr int NFK = SP / 16;                 // 16-key groups
  constexpr int KS = SP / 32;                  // k steps of P V
  constexpr int GROUPS = SP / (NW * 16);       // 16-row groups per wave
  constexpr bool HOIST = KS * ND <= 16;        // V fragments kept in registers across the wave's row groups (<= 64 VGPRs)
  constexpr int KP = DH + 8;                   // row pitch of the K / V images (elements): 16-byte pad
  constexpr int PIECES = DH / 8;               // 16-byte pieces per row
  constexpr int LOADS = SP * PIECES / NT_;
  __shared__ __attribute__((aligned(16))) elem sK[SP][KP];
  __shared__ __attribute__((aligned(16))) elem sV[SP][KP];
  __shared__ __attribute__((aligned(16))) elem sPt[NW][SP][16];    // per wave: P^T [key][query row]; afterwards its [16][DH] output slab
  __shared__ float sBias[SP];
  constexpr int SLP = SP >= KP ? KP : DH;      // row pitch of the output slab inside the wave's P^T area (SP x 16 elements)
  static_assert(SP * 16 >= 16 * SLP, "output slab must fit the wave's P^T area");
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int hh = blockIdx.x % heads, bb = blockIdx.x / heads;
  const size_t ld = (size_t)3 * H;
  const uint16_t* base = qkv + (size_t)bb * S * ld;
  {
    frag kv[LOADS], vv[LOADS];
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      const int e = tid + i * NT_, key = e / PIECES, c = e % PIECES;
#pragma unroll
      for (int j = 0; j < 8; ++j) { kv[i][j] = (elem)0.f; vv[i][j] = (elem)0.f; }
      if (key < S) {
        kv[i] = *(const frag*)(base + (size_t)key * ld + H + hh * DH + c * 8);
        vv[i] = *(const frag*)(base + (size_t)key * ld + 2 * H + hh * DH + c * 8);
      }
    }
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      const int e = tid + i * NT_, key = e / PIECES, c = e % PIECES;
      *(frag*)&sK[key][c * 8] = kv[i];
      *(frag*)&sV[key][c * 8] = vv[i];
    }
  }
  for (int i = tid; i < SP; i += NT_) sBias[i] = i >= S ? ENC_NO_KEY : mask[(size_t)bb * S + i] != 0 ? 0.f : -1e30f;   // (as above)
  __syncthreads();
  const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;   // tr read: lane 4q+p of a 16-lane group addresses row q, columns 4p..4p+3
  auto v_frag = [&](int ks, int d) -> frag {     // V[keys 32 ks + 8 g .. +7][dh 16 d + i16]
    return tr_read_pair<frag>(&sV[ks * 32 + 8 * g + tq][d * 16 + 4 * tp], &sV[ks * 32 + 8 * g + 4 + tq][d * 16 + 4 * tp]);
  };
  frag vf[HOIST ? KS : 1][ND];
  if (HOIST) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int d = 0; d < ND; ++d) vf[ks][d] = v_frag(ks, d);
  }
  float bias[NFK];
#pragma unroll
  for (int nf = 0; nf < NFK; ++nf) bias[nf] = sBias[nf * 16 + i16];
#pragma unroll 1
  for (int rg = 0; rg < GROUPS; ++rg) {
    const int row0 = (w * GROUPS + rg) * 16;
    if (row0 >= S) break;                                                  // (wave-uniform)
    const int q_row = row0 + i16;
    frag qf[NK];
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      frag z;
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = (elem)0.f;
      if (q_row < S) z = *(const frag*)(base + (size_t)q_row * ld + hh * DH + ks * 32 + g * 8);
      qf[ks] = z;
    }
    // scores: lane holds rows 4 g + r, key 16 nf + i16
    f32x4 sc[NFK];
#pragma unroll
    for (int nf = 0; nf < NFK; ++nf) {
      sc[nf] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NK; ++ks) {
        const frag kf = *(const frag*)&sK[nf * 16 + i16][ks * 32 + g * 8];
        sc[nf] = EMfma<DT>::run(qf[ks], kf, sc[nf]);
      }
    }
    float inv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = -1e30f;
#pragma unroll
      for (int nf = 0; nf < NFK; ++nf) { sc[nf][r] = sc[nf][r] * scale + bias[nf]; mx = fmaxf(mx, sc[nf][r]); }
      mx = row16_max(mx);
      float rs = 0.f;
#pragma unroll
      for (int nf = 0; nf < NFK; ++nf) { const float e = __expf(sc[nf][r] - mx); sc[nf][r] = e; rs += e; }
      inv[r] = 1.0f / row16_sum(rs);
    }
    // P^T -> LDS: one 8-byte store per accumulator (4 consecutive query rows of one key)
#pragma unroll
    for (int nf = 0; nf < NFK; ++nf) {
      e4 pk;
#pragma unroll
      for (int r = 0; r < 4; ++r) pk[r] = (elem)sc[nf][r];
      *(e4*)&sPt[w][nf * 16 + i16][4 * g] = pk;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's own LDS writes are visible to its reads
    __builtin_amdgcn_wave_barrier();
    f32x4 o[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) o[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const frag pf = tr_read_pair<frag>(&sPt[w][ks * 32 + 8 * g + tq][4 * tp], &sPt[w][ks * 32 + 8 * g + 4 + tq][4 * tp]);
#pragma unroll
      for (int d = 0; d < ND; ++d) o[d] = EMfma<DT>::run(pf, HOIST ? vf[HOIST ? ks : 0][d] : v_frag(ks, d), o[d]);
    }
    // out[row][hh*DH + 16 d + i16], row = row0 + 4 g + r: through the wave's (now idle) P^T area as a [16][DH] slab, so that it
    // leaves as 16-byte pieces of whole rows
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    elem* slab = &sPt[w][0][0];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int d = 0; d < ND; ++d) slab[(4 * g + r) * SLP + d * 16 + i16] = (elem)(o[d][r] * inv[r]);
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    for (int e = lane; e < 16 * PIECES; e += 64) {
      const int rr = e / PIECES, pc = e % PIECES;
      const int row = row0 + rr;
      if (row < S) *(frag*)&out[((size_t)bb * S + row) * H + hh * DH + pc * 8] = *(const frag*)&slab[rr * SLP + pc * 8];
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
  }
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

// ------------------------------------------------------------------ host side
struct Linear {
  uint16_t* w = nullptr;   // [N_pad][K]
  float* b = nullptr;      // [N_pad]
  int N = 0, K = 0, N_pad = 0;
};

struct Layer {
  Linear qkv, attn_out, ffn_in, ffn_out;
  float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
  // fused-LayerNorm flow (built lazily by fold_layernorms): the Linears that CONSUME a LayerNorm with gamma folded into the
  // weights (c_n in .b, s_n beside it), and the biases of the Linears whose RESIDUAL is a LayerNorm output with its beta added
  Linear qkv_f, ffn_in_f;
  float *qkv_s = nullptr, *ffn_in_s = nullptr, *attn_out_bf = nullptr, *ffn_out_bf = nullptr;
};

struct Encoder : Object {
  mrag_encoder_config cfg;
  float *word = nullptr, *pos = nullptr, *type = nullptr, *eln_g = nullptr, *eln_b = nullptr;
  std::vector<Layer> layers;
  std::map<std::string, bool> have;
  std::vector<void*> allocs;
  DevBuf ids, mask, x, y, qkv, ctx, ffn, out, stage;
  DevBuf y2, partials, st1, st2;           // fused-LayerNorm flow: second pre-LayerNorm buffer, partial sums, (mu, rstd) per token
  bool folded = false;                     // fold_layernorms done for the current parameters
  hipEvent_t ev[2] = {nullptr, nullptr};   // device work of the last forward (embeddings .. pooling), on its stream
  bool timed = false;
  ~Encoder() override {
    for (auto& v : ev) if (v) (void)hipEventDestroy(v);
    for (void* p : allocs) (void)hipFree(p);
    for (DevBuf* b : {&ids, &mask, &x, &y, &qkv, &ctx, &ffn, &out, &stage, &y2, &partials, &st1, &st2}) b->release();
  }
};

static int dev_alloc(Encoder* e, void** p, size_t bytes) {
  hipError_t err = hipMalloc(p, bytes);
  if (err != hipSuccess) return fail(MRAG_ERR_OOM, "hipMalloc(%zu) failed", bytes);
  (void)hipMemset(*p, 0, bytes);
  e->allocs.push_back(*p);
  return MRAG_OK;
}

static int alloc_linear(Encoder* e, Linear& l, int N, int K) {
  l.N = N; l.K = K; l.N_pad = (int)round_up(N, N >= G2_T ? G2_T : GN);   // 256-row padding lets the 256 x 256 kernel serve it
  // The fused-LayerNorm flow runs the 256 x 256 kernel on every Linear, those with N < 256 included (hidden 64 / 128: N_pad 128),
  // and that kernel stages whole 256-row weight tiles: the allocation always holds a full tile of (zero) rows, whatever N_pad says.
  const size_t rows = (size_t)round_up(N, G2_T);
  MRAG_TRY(dev_alloc(e, (void**)&l.w, rows * K * 2));
  MRAG_TRY(dev_alloc(e, (void**)&l.b, rows * 4));
  return MRAG_OK;
}

static std::vector<std::string> expected_params(const mrag_encoder_config& c) {
  std::vector<std::string> v = {"embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight",
                                "embeddings.token_type_embeddings.weight", "embeddings.LayerNorm.weight",
                                "embeddings.LayerNorm.bias"};
  for (int i = 0; i < c.layers; ++i) {
    const std::string p = "encoder.layer." + std::to_string(i) + ".";
    for (const char* s : {"attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense",
                          "intermediate.dense", "output.dense"}) {
      v.push_back(p + s + ".weight");
      v.push_back(p + s + ".bias");
    }
    for (const char* s : {"attention.output.LayerNorm", "output.LayerNorm"}) {
      v.push_back(p + s + ".weight");
      v.push_back(p + s + ".bias");
    }
  }
  return v;
}

// fp32 [rows][K] -> storage dtype at dst rows [row0, row0+rows) of a [N_pad][K] matrix
static int upload_matrix(Encoder* e, const float* src, int is_device, int rows, int K, uint16_t* dst, int row0, hipStream_t stream) {
  const void* s = src;
  if (!is_device) {
    MRAG_TRY(e->stage.ensure((size_t)rows * K * 4));
    MRAG_HIP(hipMemcpyAsync(e->stage.p, src, (size_t)rows * K * 4, hipMemcpyHostToDevice, stream));
    s = e->stage.p;
  }
  MRAG_TRY(launch_prep_rows(s, MRAG_F32, rows, K, dst + (size_t)row0 * K, K, e->cfg.compute_dtype, 0, stream));
  MRAG_HIP(hipStreamSynchronize(stream));
  return MRAG_OK;
}

static int upload_f32(const float* src, int is_device, int64_t n, float* dst, hipStream_t stream) {
  MRAG_HIP(hipMemcpyAsync(dst, src, (size_t)n * 4, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
  MRAG_HIP(hipStreamSynchronize(stream));
  return MRAG_OK;
}

static int device_cus() {   // CU count of the current device, read once
  static int n = 0;
  if (!n) { hipDeviceProp_t pr; int dev = 0; n = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256; }
  return n;
}

template <int DT, int NFR>
static void launch_skinny(const uint16_t* A, const Linear& l, const uint16_t* R, uint16_t* C, int epi, hipStream_t stream) {
  const dim3 grid((unsigned)(l.N_pad / 16)), block(256);
  if (epi == EPI_BIAS) hipLaunchKernelGGL((enc_gemm_skinny_kernel<DT, EPI_BIAS, NFR>), grid, block, 0, stream, A, l.w, l.b, R, C, l.N, l.K);
  else if (epi == EPI_GELU) hipLaunchKernelGGL((enc_gemm_skinny_kernel<DT, EPI_GELU, NFR>), grid, block, 0, stream, A, l.w, l.b, R, C, l.N, l.K);
  else hipLaunchKernelGGL((enc_gemm_skinny_kernel<DT, EPI_RESID, NFR>), grid, block, 0, stream, A, l.w, l.b, R, C, l.N, l.K);
}

template <int DT>
static int run_gemm(const uint16_t* A, const Linear& l, const uint16_t* R, uint16_t* C, int M, int M_pad, int epi, hipStream_t stream) {
  if (M <= 64 && l.K % 384 == 0 && l.N % 4 == 0) {
    if (M <= 16) launch_skinny<DT, 1>(A, l, R, C, epi, stream);
    else if (M <= 32) launch_skinny<DT, 2>(A, l, R, C, epi, stream);
    else launch_skinny<DT, 4>(A, l, R, C, epi, stream);
    MRAG_HIP(hipGetLastError());
    return MRAG_OK;
  }
  // 256 x 256 tiles only when they fill the chip: a small batch (the reference embeds one question, then candidates 50 at a
  // time) leaves most CUs idle with 9-72 such tiles, the 128 x 128 kernel gives it four times the workgroups
  const int n_cus = device_cus();
  const bool fills = (int64_t)(M_pad / G2_T) * (l.N_pad / G2_T) >= n_cus / 2;
  if (M_pad % G2_T == 0 && l.N_pad % G2_T == 0 && fills) {
    typedef void (*Fn)(const uint16_t*, const uint16_t*, const float*, const uint16_t*, uint16_t*, int, int, int, int, LnArgs);
    const Fn fn = epi == EPI_BIAS ? (Fn)enc_gemm256_kernel<DT, EPI_BIAS, 0> : epi == EPI_GELU ? (Fn)enc_gemm256_kernel<DT, EPI_GELU, 0>
                                                                                             : (Fn)enc_gemm256_kernel<DT, EPI_RESID, 0>;
    static std::map<const void*, bool> attr_done;
    if (!attr_done[(const void*)fn]) {
      MRAG_HIP(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, G2_LDS));
      attr_done[(const void*)fn] = true;
    }
    const int tm2 = M_pad / G2_T, tn2 = l.N_pad / G2_T;
    const int cus = device_cus();
    const int nwg = std::min(tm2 * tn2, cus);
    // (starting the XCDs an eighth of a tile apart did not shorten the store phase -- 960 -> 970 -> 984 us for the QKV GEMM
    // at 0 / 4500 / 12000 cycles per XCD; non-temporal stores did, see the epilogue)
    hipLaunchKernelGGL(fn, dim3((unsigned)nwg), dim3(G2_THR), G2_LDS, stream, A, l.w, l.b, R, C, l.N, l.K, tm2, tn2, LnArgs{});
    MRAG_HIP(hipGetLastError());
    return MRAG_OK;
  }
  const int tiles_m = M_pad / GM, tiles_n = l.N_pad / GN;
  const dim3 grid((unsigned)(tiles_m * tiles_n)), block(GTHR);
  if (epi == EPI_BIAS) hipLaunchKernelGGL((enc_gemm_kernel<DT, EPI_BIAS>), grid, block, 0, stream, A, l.w, l.b, R, C, M_pad, l.N, l.K, tiles_n);
  else if (epi == EPI_GELU) hipLaunchKernelGGL((enc_gemm_kernel<DT, EPI_GELU>), grid, block, 0, stream, A, l.w, l.b, R, C, M_pad, l.N, l.K, tiles_n);
  else hipLaunchKernelGGL((enc_gemm_kernel<DT, EPI_RESID>), grid, block, 0, stream, A, l.w, l.b, R, C, M_pad, l.N, l.K, tiles_n);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

// 256 x 256 GEMM of the fused-LayerNorm flow: weights / bias given explicitly (folded or plain), LNF = LnArgs flags
template <int DT, int EPI, int LNF>
static int run_gemm_ln(const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* R, uint16_t* C, int N, int N_pad, int K,
                       int M_pad, const LnArgs& ln, hipStream_t stream) {
  const void* fn = (const void*)enc_gemm256_kernel<DT, EPI, LNF>;
  static bool attr_done = false;
  if (!attr_done) { MRAG_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, G2_LDS)); attr_done = true; }
  const int tm2 = M_pad / G2_T, tn2 = N_pad / G2_T;
  const int cus = device_cus();   // (cached: this launcher runs ~48 times per bge-base forward)
  const int nwg = std::min(tm2 * tn2, cus);
  hipLaunchKernelGGL((enc_gemm256_kernel<DT, EPI, LNF>), dim3((unsigned)nwg), dim3(G2_THR), G2_LDS, stream, A, W, bias, R, C, N, K, tm2, tn2, ln);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

// gamma-scaled weights, s / c vectors and beta-augmented biases of the fused-LayerNorm flow, from the plain parameters
template <int DT>
static int fold_layernorms(Encoder* e, hipStream_t stream) {
  typedef typename EMfma<DT>::elem elem;
  const mrag_encoder_config& c = e->cfg;
  const int H = c.hidden;
  auto fold = [&](const Linear& src, Linear& dst, float*& svec, const float* g, const float* b) -> int {
    if (!dst.w) {
      dst.N = src.N; dst.K = src.K; dst.N_pad = src.N_pad;
      const size_t rows = (size_t)round_up(src.N, G2_T);   // whole 256-row tiles, as alloc_linear (intermediate 64 / 128: N_pad 128)
      MRAG_TRY(dev_alloc(e, (void**)&dst.w, rows * dst.K * 2));
      MRAG_TRY(dev_alloc(e, (void**)&dst.b, rows * 4));
      MRAG_TRY(dev_alloc(e, (void**)&svec, rows * 4));
    }
    hipLaunchKernelGGL((enc_fold_ln_kernel<elem>), dim3((unsigned)((src.N + 3) / 4)), dim3(256), 0, stream, (const elem*)src.w, src.b, g, b,
                       src.N, src.K, (elem*)dst.w, dst.b, svec);
    MRAG_HIP(hipGetLastError());
    return MRAG_OK;
  };
  auto add = [&](const float* bias, const float* beta, float*& out) -> int {
    if (!out) MRAG_TRY(dev_alloc(e, (void**)&out, (size_t)round_up(H, G2_T) * 4));
    hipLaunchKernelGGL(enc_add_vec_kernel, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, stream, bias, beta, H, out);
    MRAG_HIP(hipGetLastError());
    return MRAG_OK;
  };
  for (int li = 0; li < c.layers; ++li) {
    Layer& L = e->layers[li];
    MRAG_TRY(fold(L.ffn_in, L.ffn_in_f, L.ffn_in_s, L.ln1_g, L.ln1_b));
    MRAG_TRY(add(L.ffn_out.b, L.ln1_b, L.ffn_out_bf));
    if (li > 0) {
      Layer& P = e->layers[li - 1];
      MRAG_TRY(fold(L.qkv, L.qkv_f, L.qkv_s, P.ln2_g, P.ln2_b));
      MRAG_TRY(add(L.attn_out.b, P.ln2_b, L.attn_out_bf));
    }
  }
  e->folded = true;
  return MRAG_OK;
}

template <int DT>
static int forward_impl(Encoder* e, int B, int S, float* d_out, int pool, int normalize, hipStream_t stream) {
  typedef typename EMfma<DT>::elem elem;
  const mrag_encoder_config& c = e->cfg;
  const int H = c.hidden, I = c.intermediate;
  const int64_t M = (int64_t)B * S;
  const int M_pad = (int)round_up(M, M >= 2 * G2_T ? G2_T : GM);
  MRAG_TRY(e->x.ensure((size_t)M_pad * H * 2));
  MRAG_TRY(e->y.ensure((size_t)M_pad * H * 2));
  MRAG_TRY(e->qkv.ensure((size_t)M_pad * 3 * H * 2));
  MRAG_TRY(e->ctx.ensure((size_t)M_pad * H * 2));
  MRAG_TRY(e->ffn.ensure((size_t)M_pad * I * 2));
  uint16_t *x = (uint16_t*)e->x.p, *y = (uint16_t*)e->y.p, *qkv = (uint16_t*)e->qkv.p, *ctx = (uint16_t*)e->ctx.p, *ffn = (uint16_t*)e->ffn.p;
  if (M_pad > M) {   // padding rows feed the GEMMs: keep them finite
    MRAG_HIP(hipMemsetAsync(x + (size_t)M * H, 0, (size_t)(M_pad - M) * H * 2, stream));
    MRAG_HIP(hipMemsetAsync(ctx + (size_t)M * H, 0, (size_t)(M_pad - M) * H * 2, stream));
  }
  const dim3 tok_grid((unsigned)((M + 3) / 4)), tok_block(256);
  hipLaunchKernelGGL((enc_embed_ln_kernel<elem>), tok_grid, tok_block, 0, stream, (const int32_t*)e->ids.p, M, S, H, c.vocab_size,
                     e->word, e->pos, e->type, e->eln_g, e->eln_b, c.layer_norm_eps, (elem*)x);
  MRAG_HIP(hipGetLastError());
  const int dh = H / c.heads;
  const float scale = 1.0f / sqrtf((float)dh);
  // Fused-LayerNorm flow (large batches: every GEMM of a layer on the 256 x 256 kernel): the two LayerNorms of a layer never
  // run as kernels -- the GEMM before one emits per-token partial sums, a tiny kernel turns them into (mu, rstd), and the GEMMs
  // after it take the PRE-LayerNorm tensor as operand / residual (LnArgs above).  Only the last layer's output LayerNorm is
  // materialised, for the pooling.  MRAG_ENC_NO_FUSED_LN=1 keeps the plain flow (A/B, and the path small batches always take).
  // (read per forward, not once per process: the A/B test flips it between two calls)
  const bool fused_off = [] { const char* v = getenv("MRAG_ENC_NO_FUSED_LN"); return v && atoi(v) != 0; }();
  const int n_cus_f = device_cus();
  const bool fused = !fused_off && M_pad % G2_T == 0 && H % 16 == 0 && round_up(H, G2_T) / G2_T * (M_pad / G2_T) >= n_cus_f / 2;
  uint16_t *y1 = y, *y2 = nullptr;
  float2 *st1 = nullptr, *st2 = nullptr;
  float* partials = nullptr;
  const int np = 2 * (int)(round_up(H, G2_T) / G2_T);
  if (fused) {
    if (!e->folded) MRAG_TRY(fold_layernorms<DT>(e, stream));
    MRAG_TRY(e->y2.ensure((size_t)M_pad * H * 2));
    MRAG_TRY(e->partials.ensure((size_t)M_pad * np * 8));
    MRAG_TRY(e->st1.ensure((size_t)M_pad * 8));
    MRAG_TRY(e->st2.ensure((size_t)M_pad * 8));
    y2 = (uint16_t*)e->y2.p; st1 = (float2*)e->st1.p; st2 = (float2*)e->st2.p; partials = (float*)e->partials.p;
  }
  const int H_pad = (int)round_up(H, G2_T), I_pad = (int)round_up(I, G2_T), Q_pad = (int)round_up(3 * H, G2_T);
  auto finalize_stats = [&](float2* st) -> int {
    hipLaunchKernelGGL(enc_ln_stats_kernel, dim3((unsigned)((M_pad + 255) / 256)), dim3(256), 0, stream, (const float2*)partials, np, (int64_t)M_pad, H,
                       c.layer_norm_eps, st);
    MRAG_HIP(hipGetLastError());
    return MRAG_OK;
  };
  for (int li = 0; li < c.layers; ++li) {
    Layer& L = e->layers[li];
    if (fused && li > 0) {
      LnArgs a{}; a.a_stats = (const float*)st2; a.s_vec = L.qkv_s;
      MRAG_TRY((run_gemm_ln<DT, EPI_BIAS, 1>(y2, L.qkv_f.w, L.qkv_f.b, nullptr, qkv, 3 * H, Q_pad, H, M_pad, a, stream)));
    } else
    MRAG_TRY(run_gemm<DT>(x, L.qkv, nullptr, qkv, (int)M, M_pad, EPI_BIAS, stream));
    const int32_t* am = (const int32_t*)e->mask.p;
    if (dh != 32 && dh != 64) return fail(MRAG_ERR_UNSUPPORTED, "head dim %d not supported (32 or 64)", dh);
    if (S <= 256) {
      // whole-sequence kernel: K / V of a head staged once, keys padded to 64 / 128 / 256
      const dim3 g128((unsigned)(B * c.heads));
#define MRAG_ATTN(DHV, SPV, NWV) hipLaunchKernelGGL((enc_attention_s128_kernel<DT, DHV, SPV, NWV>), g128, dim3(64 * NWV), 0, stream, qkv, am, ctx, B, S, H, c.heads, scale)
      if (dh == 32) { if (S <= 64) MRAG_ATTN(32, 64, 4); else if (S <= 128) MRAG_ATTN(32, 128, 4); else MRAG_ATTN(32, 256, 8); }
      else { if (S <= 64) MRAG_ATTN(64, 64, 4); else if (S <= 128) MRAG_ATTN(64, 128, 4); else MRAG_ATTN(64, 256, 8); }
#undef MRAG_ATTN
    } else {
      // longer sequences: 128 query rows per workgroup, keys in blocks of 64 with an online softmax
      const dim3 agrid((unsigned)(B * c.heads * ((S + 127) / 128)));
      if (dh == 32) hipLaunchKernelGGL((enc_attention_kernel<DT, 32, 8>), agrid, dim3(512), 0, stream, qkv, am, ctx, B, S, H, c.heads, scale);
      else hipLaunchKernelGGL((enc_attention_kernel<DT, 64, 8>), agrid, dim3(512), 0, stream, qkv, am, ctx, B, S, H, c.heads, scale);
    }
    MRAG_HIP(hipGetLastError());
    if (fused) {
      LnArgs a{}; a.partials = partials; a.np = np;
      if (li == 0) {                                                       // y1 = ctx Wo + b + x                      (+ stats of y1)
        MRAG_TRY((run_gemm_ln<DT, EPI_RESID, 4>(ctx, L.attn_out.w, L.attn_out.b, x, y1, H, H_pad, H, M_pad, a, stream)));
      } else {                                                             // y1 = ctx Wo + (b + beta2') + LN2'(y2)     (+ stats)
        a.r_stats = (const float*)st2; a.r_gamma = e->layers[li - 1].ln2_g;
        MRAG_TRY((run_gemm_ln<DT, EPI_RESID, 6>(ctx, L.attn_out.w, L.attn_out_bf, y2, y1, H, H_pad, H, M_pad, a, stream)));
      }
      MRAG_TRY(finalize_stats(st1));
      LnArgs f{}; f.a_stats = (const float*)st1; f.s_vec = L.ffn_in_s;     // ffn = gelu(LN1(y1) W1 + b1), LN1 folded
      MRAG_TRY((run_gemm_ln<DT, EPI_GELU, 1>(y1, L.ffn_in_f.w, L.ffn_in_f.b, nullptr, ffn, I, I_pad, H, M_pad, f, stream)));
      LnArgs d{}; d.partials = partials; d.np = np; d.r_stats = (const float*)st1; d.r_gamma = L.ln1_g;
      MRAG_TRY((run_gemm_ln<DT, EPI_RESID, 6>(ffn, L.ffn_out.w, L.ffn_out_bf, y1, y2, H, H_pad, I, M_pad, d, stream)));   // y2 = ffn W2 + (b2 + beta1) + LN1(y1)
      MRAG_TRY(finalize_stats(st2));
      if (li + 1 == c.layers)                                              // the encoder's output: the one LayerNorm that is materialised
        launch_ln<elem>((const elem*)y2, M, H, L.ln2_g, L.ln2_b, c.layer_norm_eps, (elem*)x, tok_grid, tok_block, stream);
      MRAG_HIP(hipGetLastError());
      continue;
    }
    MRAG_TRY(run_gemm<DT>(ctx, L.attn_out, x, y, (int)M, M_pad, EPI_RESID, stream));                    // y = ctx Wo + b + x
    launch_ln<elem>((const elem*)y, M, H, L.ln1_g, L.ln1_b, c.layer_norm_eps, (elem*)x, tok_grid, tok_block, stream);
    MRAG_TRY(run_gemm<DT>(x, L.ffn_in, nullptr, ffn, (int)M, M_pad, EPI_GELU, stream));                  // ffn = gelu(x W1 + b1)
    MRAG_TRY(run_gemm<DT>(ffn, L.ffn_out, x, y, (int)M, M_pad, EPI_RESID, stream));                      // y = ffn W2 + b2 + x
    launch_ln<elem>((const elem*)y, M, H, L.ln2_g, L.ln2_b, c.layer_norm_eps, (elem*)x, tok_grid, tok_block, stream);
    MRAG_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL((enc_pool_kernel<elem>), dim3((unsigned)B), dim3(256), (size_t)H * 4, stream, (const elem*)x, (const int32_t*)e->mask.p, B, S, H,
                     pool, normalize, d_out);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

}  // namespace mrag

using namespace mrag;

extern "C" {

int mrag_encoder_create(const mrag_encoder_config* cfg, int device, mrag_handle* out) {
  if (!cfg || !out) return fail(MRAG_ERR_INVALID, "NULL argument");
  const mrag_encoder_config& c = *cfg;
  if (c.hidden <= 0 || c.hidden % 64 || c.heads <= 0 || c.hidden % c.heads || c.layers <= 0 || c.intermediate <= 0 ||
      c.intermediate % 64 || c.vocab_size <= 0 || c.max_position <= 0 || c.type_vocab_size <= 0)
    return fail(MRAG_ERR_INVALID, "bad encoder config (hidden and intermediate must be multiples of 64)");
  const int dh = c.hidden / c.heads;
  if (dh != 32 && dh != 64) return fail(MRAG_ERR_UNSUPPORTED, "head dim %d not supported (32 or 64)", dh);
  if (c.compute_dtype != MRAG_F16 && c.compute_dtype != MRAG_BF16) return fail(MRAG_ERR_INVALID, "compute dtype must be fp16 or bf16");
  MRAG_TRY(use_device(device));
  Encoder* e = new Encoder();
  e->kind = KIND_ENCODER; e->device = device; e->cfg = c;
  int st = MRAG_OK;
  const int H = c.hidden;
  if (st == MRAG_OK) st = dev_alloc(e, (void**)&e->word, (size_t)c.vocab_size * H * 4);
  if (st == MRAG_OK) st = dev_alloc(e, (void**)&e->pos, (size_t)c.max_position * H * 4);
  if (st == MRAG_OK) st = dev_alloc(e, (void**)&e->type, (size_t)c.type_vocab_size * H * 4);
  if (st == MRAG_OK) st = dev_alloc(e, (void**)&e->eln_g, (size_t)H * 4);
  if (st == MRAG_OK) st = dev_alloc(e, (void**)&e->eln_b, (size_t)H * 4);
  e->layers.resize(c.layers);
  for (int i = 0; i < c.layers && st == MRAG_OK; ++i) {
    Layer& L = e->layers[i];
    if (st == MRAG_OK) st = alloc_linear(e, L.qkv, 3 * H, H);
    if (st == MRAG_OK) st = alloc_linear(e, L.attn_out, H, H);
    if (st == MRAG_OK) st = alloc_linear(e, L.ffn_in, c.intermediate, H);
    if (st == MRAG_OK) st = alloc_linear(e, L.ffn_out, H, c.intermediate);
    for (float** p : {&L.ln1_g, &L.ln1_b, &L.ln2_g, &L.ln2_b})
      if (st == MRAG_OK) st = dev_alloc(e, (void**)p, (size_t)H * 4);
  }
  if (st != MRAG_OK) { delete e; return st; }
  *out = register_object(e);
  return MRAG_OK;
}

int mrag_encoder_destroy(mrag_handle h) {
  Object* o = take(h, KIND_ENCODER);
  if (!o) return MRAG_ERR_INVALID;
  (void)hipSetDevice(o->device);
  (void)hipDeviceSynchronize();
  delete o;
  return MRAG_OK;
}

int mrag_encoder_set_param(mrag_handle h, const char* name, const float* data, int64_t numel, int is_device, void* stream_) {
  Encoder* e = (Encoder*)lookup(h, KIND_ENCODER);
  if (!e) return MRAG_ERR_INVALID;
  if (!name || !data) return fail(MRAG_ERR_INVALID, "NULL argument");
  MRAG_TRY(use_device(e->device));
  hipStream_t stream = (hipStream_t)stream_;
  const mrag_encoder_config& c = e->cfg;
  const int H = c.hidden, I = c.intermediate;
  const std::string n(name);
  auto need = [&](int64_t want) -> int {
    return numel == want ? MRAG_OK : fail(MRAG_ERR_INVALID, "%s: expected %lld elements, got %lld", name, (long long)want, (long long)numel);
  };
  int st = MRAG_OK;
  if (n == "embeddings.word_embeddings.weight") { MRAG_TRY(need((int64_t)c.vocab_size * H)); st = upload_f32(data, is_device, numel, e->word, stream); }
  else if (n == "embeddings.position_embeddings.weight") { MRAG_TRY(need((int64_t)c.max_position * H)); st = upload_f32(data, is_device, numel, e->pos, stream); }
  else if (n == "embeddings.token_type_embeddings.weight") { MRAG_TRY(need((int64_t)c.type_vocab_size * H)); st = upload_f32(data, is_device, numel, e->type, stream); }
  else if (n == "embeddings.LayerNorm.weight") { MRAG_TRY(need(H)); st = upload_f32(data, is_device, numel, e->eln_g, stream); }
  else if (n == "embeddings.LayerNorm.bias") { MRAG_TRY(need(H)); st = upload_f32(data, is_device, numel, e->eln_b, stream); }
  else if (n.rfind("encoder.layer.", 0) == 0) {
    const size_t dot = n.find('.', 14);
    if (dot == std::string::npos) return fail(MRAG_ERR_INVALID, "unknown parameter %s", name);
    const int li = atoi(n.substr(14, dot - 14).c_str());
    if (li < 0 || li >= c.layers) return fail(MRAG_ERR_INVALID, "%s: layer out of range", name);
    Layer& L = e->layers[li];
    const std::string r = n.substr(dot + 1);
    auto qkv_part = [&](int part, bool is_w) -> int {
      if (is_w) { MRAG_TRY(need((int64_t)H * H)); return upload_matrix(e, data, is_device, H, H, L.qkv.w, part * H, stream); }
      MRAG_TRY(need(H));
      return upload_f32(data, is_device, H, L.qkv.b + part * H, stream);
    };
    if (r == "attention.self.query.weight") st = qkv_part(0, true);
    else if (r == "attention.self.query.bias") st = qkv_part(0, false);
    else if (r == "attention.self.key.weight") st = qkv_part(1, true);
    else if (r == "attention.self.key.bias") st = qkv_part(1, false);
    else if (r == "attention.self.value.weight") st = qkv_part(2, true);
    else if (r == "attention.self.value.bias") st = qkv_part(2, false);
    else if (r == "attention.output.dense.weight") { MRAG_TRY(need((int64_t)H * H)); st = upload_matrix(e, data, is_device, H, H, L.attn_out.w, 0, stream); }
    else if (r == "attention.output.dense.bias") { MRAG_TRY(need(H)); st = upload_f32(data, is_device, H, L.attn_out.b, stream); }
    else if (r == "attention.output.LayerNorm.weight") { MRAG_TRY(need(H)); st = upload_f32(data, is_device, H, L.ln1_g, stream); }
    else if (r == "attention.output.LayerNorm.bias") { MRAG_TRY(need(H)); st = upload_f32(data, is_device, H, L.ln1_b, stream); }
    else if (r == "intermediate.dense.weight") { MRAG_TRY(need((int64_t)I * H)); st = upload_matrix(e, data, is_device, I, H, L.ffn_in.w, 0, stream); }
    else if (r == "intermediate.dense.bias") { MRAG_TRY(need(I)); st = upload_f32(data, is_device, I, L.ffn_in.b, stream); }
    else if (r == "output.dense.weight") { MRAG_TRY(need((int64_t)H * I)); st = upload_matrix(e, data, is_device, H, I, L.ffn_out.w, 0, stream); }
    else if (r == "output.dense.bias") { MRAG_TRY(need(H)); st = upload_f32(data, is_device, H, L.ffn_out.b, stream); }
    else if (r == "output.LayerNorm.weight") { MRAG_TRY(need(H)); st = upload_f32(data, is_device, H, L.ln2_g, stream); }
    else if (r == "output.LayerNorm.bias") { MRAG_TRY(need(H)); st = upload_f32(data, is_device, H, L.ln2_b, stream); }
    else return fail(MRAG_ERR_INVALID, "unknown parameter %s", name);
  } else {
    return fail(MRAG_ERR_INVALID, "unknown parameter %s", name);
  }
  if (st == MRAG_OK) { e->have[n] = true; e->folded = false; }
  return st;
}

int mrag_encoder_missing_params(mrag_handle h, int* out_missing) {
  Encoder* e = (Encoder*)lookup(h, KIND_ENCODER);
  if (!e) return MRAG_ERR_INVALID;
  if (!out_missing) return fail(MRAG_ERR_INVALID, "out_missing is NULL");
  int miss = 0;
  std::string first;
  for (const std::string& n : expected_params(e->cfg))
    if (!e->have.count(n)) { if (!miss) first = n; ++miss; }
  if (miss) set_error("%d parameters missing, first: %s", miss, first.c_str());
  *out_missing = miss;
  return MRAG_OK;
}

int mrag_encoder_forward(mrag_handle h, const int32_t* ids, const int32_t* mask, int B, int S, float* out, int pool, int normalize,
                         int io_is_device, void* stream_) {
  Encoder* e = (Encoder*)lookup(h, KIND_ENCODER);
  if (!e) return MRAG_ERR_INVALID;
  if (B < 0 || S <= 0) return fail(MRAG_ERR_INVALID, "bad batch shape B=%d S=%d", B, S);
  if (S > e->cfg.max_position) return fail(MRAG_ERR_INVALID, "sequence length %d exceeds max_position %d", S, e->cfg.max_position);
  if (pool != MRAG_POOL_MEAN && pool != MRAG_POOL_CLS) return fail(MRAG_ERR_INVALID, "unknown pooling %d", pool);
  if (B == 0) return MRAG_OK;
  if (!ids || !mask || !out) return fail(MRAG_ERR_INVALID, "NULL buffer");
  if ((int64_t)B * S > (1ll << 30)) return fail(MRAG_ERR_UNSUPPORTED, "batch too large; split it");
  int miss = 0;
  MRAG_TRY(mrag_encoder_missing_params(h, &miss));
  if (miss) return fail(MRAG_ERR_INVALID, "encoder has %d unset parameters (%s)", miss, mrag_last_error());
  MRAG_TRY(use_device(e->device));
  hipStream_t stream = (hipStream_t)stream_;
  const size_t nb = (size_t)B * S * 4;
  MRAG_TRY(e->ids.ensure(nb));
  MRAG_TRY(e->mask.ensure(nb));
  const hipMemcpyKind kin = io_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  MRAG_HIP(hipMemcpyAsync(e->ids.p, ids, nb, kin, stream));
  MRAG_HIP(hipMemcpyAsync(e->mask.p, mask, nb, kin, stream));
  float* d_out = out;
  if (!io_is_device) { MRAG_TRY(e->out.ensure((size_t)B * e->cfg.hidden * 4)); d_out = (float*)e->out.p; }
  e->timed = false;
  for (auto& v : e->ev)
    if (!v) MRAG_HIP(hipEventCreate(&v));
  MRAG_HIP(hipEventRecord(e->ev[0], stream));
  if (e->cfg.compute_dtype == MRAG_F16) MRAG_TRY(forward_impl<MRAG_F16>(e, B, S, d_out, pool, normalize, stream));
  else MRAG_TRY(forward_impl<MRAG_BF16>(e, B, S, d_out, pool, normalize, stream));
  MRAG_HIP(hipEventRecord(e->ev[1], stream));
  e->timed = true;
  if (!io_is_device) {
    MRAG_HIP(hipMemcpyAsync(out, d_out, (size_t)B * e->cfg.hidden * 4, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipStreamSynchronize(stream));
  }
  return MRAG_OK;
}

int mrag_encoder_last_timing(mrag_handle h, float* out_ms) {
  Encoder* e = (Encoder*)lookup(h, KIND_ENCODER);
  if (!e) return MRAG_ERR_INVALID;
  if (!e->timed) return fail(MRAG_ERR_INVALID, "no completed forward to time");
  if (!out_ms) return fail(MRAG_ERR_INVALID, "out_ms is NULL");
  MRAG_TRY(use_device(e->device));
  MRAG_HIP(hipEventSynchronize(e->ev[1]));
  MRAG_HIP(hipEventElapsedTime(out_ms, e->ev[0], e->ev[1]));
  return MRAG_OK;
}

}  // extern "C"
