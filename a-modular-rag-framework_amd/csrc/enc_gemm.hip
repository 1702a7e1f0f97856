// K6, the encoder's two small-batch GEMMs: C = A . W^T + bias on MFMA 16x16x32 with the epilogue fused
// (bias | bias + erf-GELU | bias + residual).
//   enc_gemm_kernel<DT, EPI>              128 x 128 x 64 tiles, 4 waves, LDS-DMA staged, XOR-swizzled 128-B rows (same scheme as
//                                         K2); one workgroup per tile
//   enc_gemm_skinny_kernel<DT, EPI, NFR>  <= 64 tokens (one question): a workgroup owns 16 output columns, its four waves a
//                                         quarter of K each, 16 NFR token rows
// launch_gemm128 / launch_gemm_skinny pick the instance; which GEMM a Linear takes is run_gemm's decision (encoder.hip).
#include "enc_kernels.h"

namespace mrag {

// ------------------------------------------------------------------ GEMM with fused epilogues
constexpr int GTHR = 256;
constexpr int G_A_BYTES = GM * GK * 2;             // 16 KiB
constexpr int G_STAGE = (GM + GN) * GK * 2;        // 32 KiB

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

// ------------------------------------------------------------------ launchers: (dtype, epilogue[, token fragments]) -> instance
typedef void (*Gemm128Fn)(const uint16_t*, const uint16_t*, const float*, const uint16_t*, uint16_t*, int, int, int, int);
template <int DT>
static Gemm128Fn gemm128_instance(int epi) {
  return epi == EPI_BIAS ? enc_gemm_kernel<DT, EPI_BIAS> : epi == EPI_GELU ? enc_gemm_kernel<DT, EPI_GELU> : enc_gemm_kernel<DT, EPI_RESID>;
}

int launch_gemm128(int dt, int epi, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* R, uint16_t* C, int M_pad, int N,
                   int N_pad, int K, hipStream_t stream) {
  const Gemm128Fn fn = dt == MRAG_F16 ? gemm128_instance<MRAG_F16>(epi) : gemm128_instance<MRAG_BF16>(epi);
  const int tiles_m = M_pad / GM, tiles_n = N_pad / GN;
  hipLaunchKernelGGL(fn, dim3((unsigned)(tiles_m * tiles_n)), dim3(GTHR), 0, stream, A, W, bias, R, C, M_pad, N, K, tiles_n);
  return launched();
}

typedef void (*SkinnyFn)(const uint16_t*, const uint16_t*, const float*, const uint16_t*, uint16_t*, int, int);
template <int DT, int NFR>
static SkinnyFn skinny_epilogue(int epi) {
  return epi == EPI_BIAS ? enc_gemm_skinny_kernel<DT, EPI_BIAS, NFR>
         : epi == EPI_GELU ? enc_gemm_skinny_kernel<DT, EPI_GELU, NFR> : enc_gemm_skinny_kernel<DT, EPI_RESID, NFR>;
}
template <int DT>
static SkinnyFn skinny_instance(int M, int epi) {
  return M <= 16 ? skinny_epilogue<DT, 1>(epi) : M <= 32 ? skinny_epilogue<DT, 2>(epi) : skinny_epilogue<DT, 4>(epi);
}

int launch_gemm_skinny(int dt, int epi, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* R, uint16_t* C, int M, int N,
                       int N_pad, int K, hipStream_t stream) {
  const SkinnyFn fn = dt == MRAG_F16 ? skinny_instance<MRAG_F16>(M, epi) : skinny_instance<MRAG_BF16>(M, epi);
  hipLaunchKernelGGL(fn, dim3((unsigned)(N_pad / 16)), dim3(256), 0, stream, A, W, bias, R, C, N, K);
  return launched();
}

}  // namespace mrag
