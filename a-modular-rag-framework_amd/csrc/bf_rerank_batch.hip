// The candidate lookups of the dense index: mrag_index_score_rows (one question, score_rows_kernel) and the batched
// mrag_index_score_rows_batch (include/mrag_rerank_batch.h): the scores of a ragged batch of (question, stored row) pairs
// in one launch.  Here are both kernels, the host plan that cuts the lists into descriptors and the two entry points.
//
// What stays from score_rows_kernel, because fp64 accumulation is not order-independent for bf16 rows
// or un-normalised rows and the batch must return the single call's bits: one wave per row, lane l accumulates the
// exact products of columns l, l + 64, ... in that order in fp64, then the __shfl_xor butterfly at 32 .. 1.
// What is new is everything around it: one 256-thread workgroup per descriptor (question, first entry, <= 64 entries),
// so the load is balanced whatever the skew of the lists and no launch dimension depends on the longest one; a wave
// widens its question's query columns once into registers (ld <= 1024: <= 16 per lane) and walks the descriptor's
// rows wave-strided two at a time, both rows' loads issued before the first is reduced.
//
// A row is read as 2 bytes per lane per instruction -- one 128-byte line per wave instruction -- which is what the
// fixed assignment of columns to lanes gives without a transpose through LDS.
#include "bf_index.h"

namespace mrag {

// one wave per listed row: score = <prepared query, stored row> (fp64 accumulation of the exact 16-bit products)
__global__ __launch_bounds__(256) void score_rows_kernel(const uint16_t* __restrict__ rows, const uint16_t* __restrict__ q, int ld,
                                                         int is_bf16, const int64_t* __restrict__ ids, int64_t n, int64_t n_rows,
                                                         float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  const int64_t r = ids[i];
  if (r < 0 || r >= n_rows) { if (lane == 0) out[i] = 0.0f; return; }   // unknown row: the reference's 0.0 for an unusable vector
  const uint16_t* row = rows + (size_t)r * ld;
  double acc = 0.0;
  for (int c = lane; c < ld; c += 64) {
    float a, b;
    if (is_bf16) { a = __uint_as_float((uint32_t)row[c] << 16); b = __uint_as_float((uint32_t)q[c] << 16); }
    else { _Float16 ha, hb; __builtin_memcpy(&ha, &row[c], 2); __builtin_memcpy(&hb, &q[c], 2); a = (float)ha; b = (float)hb; }
    acc += (double)a * (double)b;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane == 0) out[i] = (float)acc;
}

// One workgroup of the batch kernel scores one descriptor: entries [first, first + count) of the flat id list, all of
// question `question`, count <= RERANK_ROWS (bf_kernels.h).
struct RerankDesc {
  int64_t question, first;
  int32_t count, pad;
};

namespace {

constexpr int RERANK_QREG = 16;                        // query columns a lane keeps in registers
constexpr int RERANK_REG_LD = RERANK_QREG * 64;        // widest row whose query is register-held
constexpr int64_t RERANK_GRID_X = 2147483647;          // HIP's limit on gridDim.x

template <bool BF16>
__device__ __forceinline__ float widen16(uint16_t b) {
  if (BF16) return __uint_as_float((uint32_t)b << 16);
  _Float16 h;
  __builtin_memcpy(&h, &b, 2);
  return (float)h;
}

// a wave-uniform int64 as a scalar, so that the row base is not a per-lane address computation
__device__ __forceinline__ int64_t uniform64(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ double wave_sum_xor(double acc) {   // score_rows_kernel's butterfly
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  return acc;
}

// REG: ld <= RERANK_REG_LD, the query columns of a lane live in registers; else the query is re-read (from L2) per row pair
template <bool BF16, bool REG>
__global__ __launch_bounds__(256) void rerank_batch_kernel(const uint16_t* __restrict__ rows, const uint16_t* __restrict__ queries,
                                                           int ld, const RerankDesc* __restrict__ desc,
                                                           const int64_t* __restrict__ ids, int64_t n_rows, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const RerankDesc d = desc[blockIdx.x];
  const int count = d.count;
  if (wave >= count) return;
  const uint16_t* q = queries + (size_t)d.question * ld;
  const int64_t* id = ids + d.first;
  float* o = out + d.first;
  const int steps = ld >> 6;                           // ld is a multiple of 64: every lane has `steps` columns
  float qv[RERANK_QREG];
  if (REG) {
#pragma unroll
    for (int i = 0; i < RERANK_QREG; ++i) qv[i] = i < steps ? widen16<BF16>(q[lane + 64 * i]) : 0.f;
  }
  for (int j0 = wave; j0 < count; j0 += 8) {
    const int j1 = j0 + 4;
    const bool has1 = j1 < count;
    const int64_t r0 = uniform64(id[j0]), r1 = has1 ? uniform64(id[j1]) : -1;
    const bool ok0 = r0 >= 0 && r0 < n_rows, ok1 = r1 >= 0 && r1 < n_rows;
    // a row outside the index scores 0.0: its loads go to the query row (memory that is there) and are dropped
    const uint16_t* a0 = ok0 ? rows + (size_t)r0 * ld : q;
    const uint16_t* a1 = ok1 ? rows + (size_t)r1 * ld : q;
    double s0 = 0.0, s1 = 0.0;
    if (REG) {
      uint16_t x0[RERANK_QREG], x1[RERANK_QREG];
#pragma unroll
      for (int i = 0; i < RERANK_QREG; ++i) x0[i] = i < steps ? a0[lane + 64 * i] : (uint16_t)0;
#pragma unroll
      for (int i = 0; i < RERANK_QREG; ++i) x1[i] = i < steps ? a1[lane + 64 * i] : (uint16_t)0;
#pragma unroll
      for (int i = 0; i < RERANK_QREG; ++i)
        if (i < steps) s0 += (double)widen16<BF16>(x0[i]) * (double)qv[i];
#pragma unroll
      for (int i = 0; i < RERANK_QREG; ++i)
        if (i < steps) s1 += (double)widen16<BF16>(x1[i]) * (double)qv[i];
    } else {
      // four column steps at a time: their twelve loads are issued before the first product, the sums keep column order
      int i = 0;
      for (; i + 4 <= steps; i += 4) {
        uint16_t x0[4], x1[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = lane + 64 * (i + u);
          x0[u] = a0[c]; x1[u] = a1[c]; b[u] = q[c];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const double bd = (double)widen16<BF16>(b[u]);
          s0 += (double)widen16<BF16>(x0[u]) * bd;
          s1 += (double)widen16<BF16>(x1[u]) * bd;
        }
      }
      for (; i < steps; ++i) {
        const int c = lane + 64 * i;
        const uint16_t x0 = a0[c], x1 = a1[c];
        const double bd = (double)widen16<BF16>(q[c]);
        s0 += (double)widen16<BF16>(x0) * bd;
        s1 += (double)widen16<BF16>(x1) * bd;
      }
    }
    s0 = wave_sum_xor(s0);
    s1 = wave_sum_xor(s1);
    if (lane == 0) {
      o[j0] = ok0 ? (float)s0 : 0.0f;
      if (has1) o[j1] = ok1 ? (float)s1 : 0.0f;
    }
  }
}

}  // namespace

// the descriptors of row_ptr [n_questions + 1] (validated by the caller), in question order; empty questions get none
static int rerank_batch_plan(int64_t n_questions, const int64_t* row_ptr, std::vector<RerankDesc>& desc) {
  int64_t n_desc = 0;
  for (int64_t g = 0; g < n_questions; ++g) n_desc += (row_ptr[g + 1] - row_ptr[g] + RERANK_ROWS - 1) / RERANK_ROWS;
  try {
    desc.clear();
    desc.reserve((size_t)n_desc);
    for (int64_t g = 0; g < n_questions; ++g)
      for (int64_t e = row_ptr[g]; e < row_ptr[g + 1]; e += RERANK_ROWS)
        desc.push_back(RerankDesc{g, e, (int32_t)std::min<int64_t>(RERANK_ROWS, row_ptr[g + 1] - e), 0});
  } catch (const std::bad_alloc&) {
    return fail(MRAG_ERR_OOM, "no host memory for %lld re-rank descriptors", (long long)n_desc);
  }
  return MRAG_OK;
}

// out[e] = <queries[question of e], rows[ids[e]]> for every entry the n_desc descriptors cover (0.0 for an id outside
// [0, n_rows)); prepared queries at pitch ld; every pointer is a device pointer; one launch per 2^31 - 1 descriptors
static int launch_rerank_batch(const uint16_t* rows, const uint16_t* queries, int ld, int is_bf16, const RerankDesc* desc, int64_t n_desc,
                        const int64_t* ids, int64_t n_rows, float* out, hipStream_t stream) {
  if (ld <= 0 || ld % 64) return fail(MRAG_ERR_INVALID, "re-rank batch: row pitch %d is not a positive multiple of 64", ld);
  const bool reg = ld <= RERANK_REG_LD;
  for (int64_t first = 0; first < n_desc; first += RERANK_GRID_X) {      // one launch in every realistic case
    const int64_t n = std::min<int64_t>(RERANK_GRID_X, n_desc - first);
    if (n <= 0 || n > RERANK_GRID_X) return fail(MRAG_ERR_HIP, "re-rank batch launch grid (%lld) outside HIP's limits", (long long)n);
    const dim3 grid((unsigned)n), block(256);
    const RerankDesc* d = desc + first;
    if (is_bf16) {
      if (reg) hipLaunchKernelGGL((rerank_batch_kernel<true, true>), grid, block, 0, stream, rows, queries, ld, d, ids, n_rows, out);
      else hipLaunchKernelGGL((rerank_batch_kernel<true, false>), grid, block, 0, stream, rows, queries, ld, d, ids, n_rows, out);
    } else {
      if (reg) hipLaunchKernelGGL((rerank_batch_kernel<false, true>), grid, block, 0, stream, rows, queries, ld, d, ids, n_rows, out);
      else hipLaunchKernelGGL((rerank_batch_kernel<false, false>), grid, block, 0, stream, rows, queries, ld, d, ids, n_rows, out);
    }
    MRAG_HIP(hipGetLastError());
  }
  return MRAG_OK;
}

}  // namespace mrag

using namespace mrag;

extern "C" {

int mrag_index_score_rows(mrag_handle h, const void* query, int q_dtype, int normalize, const int64_t* row_ids, int64_t n,
                          float* out_scores, void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (n < 0) return fail(MRAG_ERR_INVALID, "n < 0");
  if (n == 0) return MRAG_OK;
  if (!query || !row_ids || !out_scores) return fail(MRAG_ERR_INVALID, "NULL buffer");
  const size_t esz = dtype_size(q_dtype);
  if (!esz) return fail(MRAG_ERR_INVALID, "unknown query dtype %d", q_dtype);
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  // staging: [query src | row ids | scores]; prepared query in qbuf (one row)
  const size_t qb = round_up((int64_t)(ix->dim * esz), 256), ib = round_up(n * 8, 256), ob = (size_t)n * 4;
  MRAG_TRY(ix->stage_in.ensure(qb + ib + ob));
  MRAG_TRY(ix->qbuf.ensure((size_t)(TQ + SQ) * ix->ld * 2));
  char* st = (char*)ix->stage_in.p;
  // (the uploads read the caller's host buffers asynchronously)
  return run_synced(stream, [&]() -> int {
    MRAG_HIP(hipMemcpyAsync(st, query, (size_t)ix->dim * esz, hipMemcpyHostToDevice, stream));
    MRAG_HIP(hipMemcpyAsync(st + qb, row_ids, (size_t)n * 8, hipMemcpyHostToDevice, stream));
    MRAG_TRY(launch_prep_rows(st, q_dtype, 1, ix->dim, ix->qbuf.p, ix->ld, ix->dtype,
                              normalize && ix->metric == MRAG_METRIC_COSINE, stream));
    if (ix->qbuf.p == ix->q_cleared_buf) ix->q_dirty_rows = std::max<int64_t>(ix->q_dirty_rows, 1);   // row 0 of the query buffer was written
    hipLaunchKernelGGL(score_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, ix->rows, (const uint16_t*)ix->qbuf.p,
                       ix->ld, ix->dtype == MRAG_BF16 ? 1 : 0, (const int64_t*)(st + qb), n, ix->n, (float*)(st + qb + ib));
    MRAG_HIP(hipGetLastError());
    MRAG_HIP(hipMemcpyAsync(out_scores, st + qb + ib, ob, hipMemcpyDeviceToHost, stream));
    return MRAG_OK;
  });
}

int mrag_index_score_rows_batch(mrag_handle h, const void* queries, int q_dtype, int normalize, int64_t n_questions,
                                const int64_t* row_ptr, const int64_t* row_ids, float* out_scores, void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (n_questions < 0) return fail(MRAG_ERR_INVALID, "n_questions < 0");
  if (n_questions == 0) return MRAG_OK;
  if (!row_ptr) return fail(MRAG_ERR_INVALID, "row_ptr is NULL");
  MRAG_TRY(check_csr(row_ptr, n_questions, "row_ptr", "question"));
  const int64_t n = row_ptr[n_questions];
  if (n == 0) return MRAG_OK;                 // a batch of empty questions
  if (!queries || !row_ids || !out_scores) return fail(MRAG_ERR_INVALID, "NULL buffer");
  const size_t esz = dtype_size(q_dtype);
  if (!esz) return fail(MRAG_ERR_INVALID, "unknown query dtype %d", q_dtype);
  std::vector<RerankDesc> desc;
  MRAG_TRY(rerank_batch_plan(n_questions, row_ptr, desc));
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  // staging: [query src | descriptors | row ids | scores]; prepared queries in rr_q
  const size_t qbytes = (size_t)n_questions * ix->dim * esz, dbytes = desc.size() * sizeof(RerankDesc);
  const size_t qb = round_up((int64_t)qbytes, 256), db = round_up((int64_t)dbytes, 256), ib = round_up(n * 8, 256), ob = (size_t)n * 4;
  MRAG_TRY(ix->stage_in.ensure(qb + db + ib + ob));
  MRAG_TRY(ix->rr_q.ensure((size_t)n_questions * ix->ld * 2));
  if ((n_questions + 3) / 4 > 2147483647ll)   // (out of reach: the two buffers above do not fit any device at this size)
    return fail(MRAG_ERR_HIP, "row preparation grid for %lld questions outside HIP's limits", (long long)n_questions);
  char* st = (char*)ix->stage_in.p;
  // (the uploads read `desc` and the caller's host buffers asynchronously)
  return run_synced(stream, [&]() -> int {
    MRAG_HIP(hipMemcpyAsync(st, queries, qbytes, hipMemcpyHostToDevice, stream));
    MRAG_HIP(hipMemcpyAsync(st + qb, desc.data(), dbytes, hipMemcpyHostToDevice, stream));
    MRAG_HIP(hipMemcpyAsync(st + qb + db, row_ids, (size_t)n * 8, hipMemcpyHostToDevice, stream));
    // the single call's preparation of its one row, for every row (row g's source keeps the 16-byte alignment of row 0
    // wherever launch_prep_rows asks for it: dim % 8 == 0 there)
    MRAG_TRY(launch_prep_rows(st, q_dtype, n_questions, ix->dim, ix->rr_q.p, ix->ld, ix->dtype,
                              normalize && ix->metric == MRAG_METRIC_COSINE, stream));
    MRAG_TRY(launch_rerank_batch(ix->rows, (const uint16_t*)ix->rr_q.p, ix->ld, ix->dtype == MRAG_BF16 ? 1 : 0,
                                 (const RerankDesc*)(st + qb), (int64_t)desc.size(), (const int64_t*)(st + qb + db), ix->n,
                                 (float*)(st + qb + db + ib), stream));
    MRAG_HIP(hipMemcpyAsync(out_scores, st + qb + db + ib, ob, hipMemcpyDeviceToHost, stream));
    return MRAG_OK;
  });
}

}  // extern "C"
