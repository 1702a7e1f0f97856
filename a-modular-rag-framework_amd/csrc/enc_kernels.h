// What the encoder sources (enc_rowwise, enc_gemm, enc_gemm256, enc_attention, encoder) share among themselves: the MFMA
// wrapper and vector types, the erf-GELU and the wave sum, the epilogue enum, the LayerNorm-folding arguments, the tile
// constants host code needs and the plain host launchers each source exports.  Kernel templates and the choice of their
// instance stay inside the source that owns them.  Internal to those sources; what other translation units use is in common.h.
#pragma once
#include "common.h"

#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include <type_traits>

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

// ---- tile geometry host code needs (padding of activations and weights, the regime rules of encoder.hip) ----
constexpr int GM = 128, GN = 128, GK = 64;   // 128 x 128 kernel: token rows x weight rows per tile; K elements per stage (both tiled kernels)
constexpr int G2_T = 256;                    // 256 x 256 kernel: rows per tile, tokens and weight rows alike
enum { EPI_BIAS = 0, EPI_GELU = 1, EPI_RESID = 2 };

// LayerNorm folded into the GEMMs around it (LNF flags of enc_gemm256_kernel; layer_fused in encoder.hip):
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

// how every launcher below ends: the status of the launch it has just issued
static inline int launched() {
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

// ---- host launchers the encoder sources export to each other (every pointer is a device pointer; dt = MRAG_F16 | MRAG_BF16,
// activations and weights are 16-bit in that dtype; each returns the launch status) ----
// enc_rowwise.hip: one wave per token / row
int launch_embed_ln(int dt, const int32_t* ids, int64_t n_tok, int S, int H, int vocab, const float* word, const float* pos, const float* type0,
                    const float* g, const float* b, float eps, uint16_t* out, hipStream_t stream);
// LayerNorm of n_tok rows: enc_ln_vec_kernel when H % 8 == 0 and H <= 2048, else the scalar enc_ln_kernel
int launch_ln(int dt, const uint16_t* x, int64_t n_tok, int H, const float* g, const float* b, float eps, uint16_t* out, hipStream_t stream);
// (mu, rstd) of n_tok tokens from the np partial-sum slots a STATS GEMM left per token
int launch_ln_stats(const float* partials, int np, int64_t n_tok, int H, float eps, float* stats, hipStream_t stream);
// W [N][K], b -> Wf = gamma o W, c = b + W beta, svec = row sums of Wf (the LNA operands of LnArgs)
int launch_fold_ln(int dt, const uint16_t* W, const float* b, const float* gamma, const float* beta, int N, int K, uint16_t* Wf, float* c,
                   float* svec, hipStream_t stream);
int launch_add_vec(const float* a, const float* b, int n, float* out, hipStream_t stream);
int launch_pool(int dt, const uint16_t* x, const int32_t* mask, int B, int S, int H, int pool, int normalize, float* out, hipStream_t stream);
// enc_gemm.hip: C = epi(A W^T + bias [+ R]).  Skinny: M <= 64 tokens, K % 384 == 0, N % 4 == 0 (NFR = 1 / 2 / 4 token
// fragments for M <= 16 / 32 / 64).  128: M_pad % 128 == 0, N_pad % 128 == 0, K % 64 == 0.
int launch_gemm_skinny(int dt, int epi, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* R, uint16_t* C, int M, int N,
                       int N_pad, int K, hipStream_t stream);
int launch_gemm128(int dt, int epi, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* R, uint16_t* C, int M_pad, int N,
                   int N_pad, int K, hipStream_t stream);
// enc_gemm256.hip: the persistent 256 x 256 kernel, instance (dt, epi, lnf); lnf = the LNF flags of LnArgs (0: plain).  M_pad % 256 == 0;
// W holds whole 256-row tiles up to round_up(N, 256) rows.  min(tiles, CUs) workgroups.
int launch_gemm256(int dt, int epi, int lnf, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* R, uint16_t* C, int M_pad,
                   int N, int K, const LnArgs& ln, hipStream_t stream);
int enc_device_cus();   // CU count of the current device, read once (enc_gemm256.hip)
// enc_attention.hip: QKV [M_pad][3H] -> ctx [M_pad][H]; S <= 256: enc_attention_s128_kernel with the keys padded to 64 / 128 / 256,
// longer: enc_attention_kernel with 128 query rows per workgroup.  dh = 32 | 64, anything else is MRAG_ERR_UNSUPPORTED.
int launch_attention(int dt, int dh, const uint16_t* qkv, const int32_t* mask, uint16_t* ctx, int B, int S, int H, int heads, hipStream_t stream);

}  // namespace mrag
