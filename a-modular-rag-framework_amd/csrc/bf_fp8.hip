// fp8 scan copy + exact re-rank (mrag_index_search_fp8; contract in include/mrag.h)
//   rows8 [cap_rows][ld8] = e4m3fn(clamp(256 * stored 16-bit value, +-448)), ld8 = dim rounded up to 128, pads zero.
//   A search quantises each prepared query with its own power of two (max |q~| in [128, 256)), picks the top-`refine`
//   rows by fp8 score with the fp8 instances of K2 / K2s + the unchanged merges, then re-scores those rows exactly.
// This file: the two quantisers, the re-rank and their launchers (declared in common.h; the IVF index uses them too).
#include "bf_kernels.h"

namespace mrag {

static_assert(FP8_MAX_REFINE == KMAX, "the refine pool is the batch kernel's list limit");

__device__ __forceinline__ float bits_f32(uint16_t b, int is_bf16) {
  if (is_bf16) return __uint_as_float((uint32_t)b << 16);
  _Float16 h;
  __builtin_memcpy(&h, &b, 2);
  return (float)h;
}
// four floats -> four OCP e4m3fn bytes (v_cvt_pk_fp8_f32: round to nearest even); the inputs are clamped to +-448 first
__device__ __forceinline__ uint32_t e4m3x4(float a, float b, float c, float d) {
  a = fminf(fmaxf(a, -448.f), 448.f); b = fminf(fmaxf(b, -448.f), 448.f);
  c = fminf(fmaxf(c, -448.f), 448.f); d = fminf(fmaxf(d, -448.f), 448.f);
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (uint32_t)w;
}

// corpus rows [0, n) of a 16-bit matrix (pitch ld) -> the fp8 copy (pitch ld8 bytes, columns >= ld zero); 4 bytes per thread
__global__ void quant_rows_fp8_kernel(const uint16_t* __restrict__ src, int ld, int is_bf16, int64_t n,
                                      uint8_t* __restrict__ dst, int ld8) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per = ld8 / 4;
  if (i >= n * per) return;
  const int64_t r = i / per;
  const int c = (int)(i - r * per) * 4;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (c < ld) {   // ld % 64 == 0: all four columns are inside the 16-bit row
    const uint2 b = *(const uint2*)(src + (size_t)r * ld + c);
    v[0] = bits_f32((uint16_t)b.x, is_bf16); v[1] = bits_f32((uint16_t)(b.x >> 16), is_bf16);
    v[2] = bits_f32((uint16_t)b.y, is_bf16); v[3] = bits_f32((uint16_t)(b.y >> 16), is_bf16);
  }
  *(uint32_t*)(dst + (size_t)r * ld8 + c) = e4m3x4(v[0] * 256.f, v[1] * 256.f, v[2] * 256.f, v[3] * 256.f);
}

// one wave per prepared query row: q~ = e4m3fn(q * 2^e) with max |q * 2^e| in [128, 256) (exact: a power of two); a zero
// row stays zero.  A positive per-query factor leaves that query's ranking unchanged, so the candidate kernels need no
// epilogue scaling.
__global__ __launch_bounds__(64) void quant_queries_fp8_kernel(const uint16_t* __restrict__ src, int ld, int is_bf16,
                                                               uint8_t* __restrict__ dst, int ld8) {
  const int lane = threadIdx.x;
  const uint16_t* row = src + (size_t)blockIdx.x * ld;
  float amax = 0.f;
  for (int c = lane; c < ld; c += 64) amax = fmaxf(amax, fabsf(bits_f32(row[c], is_bf16)));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off));
  int ex = 0;
  if (amax > 0.f) { (void)frexpf(amax, &ex); ex = 8 - ex; }   // amax = m * 2^E, m in [0.5, 1): amax * 2^(8-E) in [128, 256)
  uint8_t* out = dst + (size_t)blockIdx.x * ld8;
  for (int c = lane * 4; c < ld8; c += 256) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (c < ld) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = ldexpf(bits_f32(row[c + j], is_bf16), ex);
    }
    *(uint32_t*)(out + c) = e4m3x4(v[0], v[1], v[2], v[3]);
  }
}

// one workgroup per query: the fp32 dot product of the 16-bit query with the stored 16-bit row of each of its <= 64
// candidates (16 lanes per candidate, 8 elements per lane and pass), then the k best in (score desc, row asc) order,
// + id_base.  Candidate slots without a row (-1) are skipped; output slots past the candidates found are (-inf, -1).
__global__ __launch_bounds__(256) void fp8_rerank_kernel(const uint16_t* __restrict__ rows, const uint16_t* __restrict__ queries,
                                                         int ld, int is_bf16, const int64_t* __restrict__ cand, int refine, int k,
                                                         int64_t id_base, float* __restrict__ out_sc, int64_t* __restrict__ out_id) {
  __shared__ float s_sc[FP8_MAX_REFINE];
  __shared__ int s_row[FP8_MAX_REFINE];
  const int tid = threadIdx.x, grp = tid >> 4, gl = tid & 15;
  const int64_t q = blockIdx.x;
  const uint16_t* qr = queries + (size_t)q * ld;
  for (int c = grp; c < refine; c += 16) {
    const int64_t r = cand[q * refine + c];
    float acc = 0.f;
    if (r >= 0) {
      const uint16_t* rr = rows + (size_t)r * ld;
      for (int e = gl * 8; e < ld; e += 128) {
        const uint4 a = *(const uint4*)(rr + e), b = *(const uint4*)(qr + e);
        const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc = fmaf(bits_f32((uint16_t)aw[j], is_bf16), bits_f32((uint16_t)bw[j], is_bf16), acc);
          acc = fmaf(bits_f32((uint16_t)(aw[j] >> 16), is_bf16), bits_f32((uint16_t)(bw[j] >> 16), is_bf16), acc);
        }
      }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off);   // within the 16-lane group
    if (gl == 0) { s_sc[c] = acc; s_row[c] = r < 0 ? -1 : (int)r; }
  }
  __syncthreads();
  if (tid >= 64) return;
  const bool valid = tid < refine && s_row[tid] >= 0;
  const uint64_t my = valid ? make_key(__float_as_uint(s_sc[tid]), (uint32_t)s_row[tid]) : 0ull;
  int rank = 0;
  for (int j = 0; j < refine; ++j) {
    const uint64_t kj = s_row[j] >= 0 ? make_key(__float_as_uint(s_sc[j]), (uint32_t)s_row[j]) : 0ull;
    rank += kj > my ? 1 : 0;
  }
  const int nvalid = __popcll(__ballot(valid));
  if (valid && rank < k) { out_sc[q * k + rank] = s_sc[tid]; out_id[q * k + rank] = id_base + s_row[tid]; }
  if (tid >= nvalid && tid < k) { out_sc[q * k + tid] = -INFINITY; out_id[q * k + tid] = -1; }
}

int launch_quant_rows_fp8(const uint16_t* src, int ld, int is_bf16, int64_t n, uint8_t* dst, int ld8, hipStream_t stream) {
  const int64_t tot = n * (ld8 / 4);
  if (tot <= 0) return MRAG_OK;
  hipLaunchKernelGGL(quant_rows_fp8_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, src, ld, is_bf16, n, dst, ld8);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

int launch_quant_queries_fp8(const uint16_t* src, int ld, int is_bf16, int64_t n, uint8_t* dst, int ld8, hipStream_t stream) {
  if (n <= 0) return MRAG_OK;
  hipLaunchKernelGGL(quant_queries_fp8_kernel, dim3((unsigned)n), dim3(64), 0, stream, src, ld, is_bf16, dst, ld8);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

int launch_fp8_rerank(const uint16_t* rows, const uint16_t* queries, int ld, int is_bf16, const int64_t* cand, int64_t nq, int refine,
                      int k, int64_t id_base, float* out_sc, int64_t* out_id, hipStream_t stream) {
  if (nq <= 0) return MRAG_OK;
  hipLaunchKernelGGL(fp8_rerank_kernel, dim3((unsigned)nq), dim3(256), 0, stream, rows, queries, ld, is_bf16, cand, refine, k, id_base,
                     out_sc, out_id);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

}  // namespace mrag
