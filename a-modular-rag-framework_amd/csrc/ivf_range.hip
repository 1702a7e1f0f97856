// IVF range search and self-join: rows scoring >= a floor, with one excluded row per query given as an original row and
// turned into its stored position here.  State: IvfRangeState (ivf_index.h).
#include "ivf_index.h"

namespace mrag {

// ---- range search: the excluded rows as stored positions --------------------------------------------------------
// inv[row_ids[p]] = p over the stored positions (padding positions hold -1)
__global__ void ivf_inverse_pos_kernel(const int64_t* __restrict__ row_ids, int64_t n_sorted, int64_t n, int64_t* __restrict__ inv) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_sorted) return;
  const int64_t r = row_ids[p];
  if (r >= 0 && r < n) inv[r] = p;
}
// query i excludes row rows[i] (rows == nullptr: row0 + i, the self-join) -> its stored position, -1 for none / not a row
__global__ void ivf_excl_pos_kernel(const int64_t* __restrict__ rows, int64_t row0, int64_t nq, int64_t n,
                                    const int64_t* __restrict__ inv, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const int64_t r = rows ? rows[i] : row0 + i;
  out[i] = (r >= 0 && r < n) ? inv[r] : -1;
}

int ivf_ensure_inv_pos(IvfIndex* ix, hipStream_t stream) {
  IvfRangeState& w = ix->range;
  if (w.inv_valid) return MRAG_OK;
  MRAG_TRY(w.inv_pos.ensure((size_t)std::max<int64_t>(ix->n, 1) * 8));
  hipLaunchKernelGGL(ivf_inverse_pos_kernel, dim3((unsigned)((ix->n_sorted + 255) / 256)), dim3(256), 0, stream,
                     (const int64_t*)ix->row_ids, ix->n_sorted, ix->n, (int64_t*)w.inv_pos.p);
  MRAG_HIP(hipGetLastError());
  w.inv_valid = true;
  return MRAG_OK;
}

static int ivf_check_range_args(int64_t nq, int k, int nprobe, float min_score, const void* out_counts) {
  if (nq < 0 || k <= 0 || nprobe <= 0) return fail(MRAG_ERR_INVALID, "bad nq / k / nprobe");
  if (k > 256) return fail(MRAG_ERR_INVALID, "range search: k = %d, supported are 1..256 (the per-query selection's limit)", k);
  if (!std::isfinite(min_score)) return fail(MRAG_ERR_INVALID, "min_score must be finite");
  if (nq > 0 && !out_counts) return fail(MRAG_ERR_INVALID, "out_counts is NULL");
  return MRAG_OK;
}

int IvfSearch::run_range(const int64_t* d_excl_rows, int64_t self_row0) {
  MRAG_TRY(refuse_fused());
  MRAG_TRY(start());
  if (d_excl_rows || self_row0 >= 0) {
    MRAG_TRY(ivf_ensure_inv_pos(ix, stream));
    int64_t* d_pos = (int64_t*)ix->range.excl.p + nq;
    hipLaunchKernelGGL(ivf_excl_pos_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, d_excl_rows, self_row0, nq, ix->n,
                       (const int64_t*)ix->range.inv_pos.p, d_pos);
    MRAG_HIP(hipGetLastError());
    excl_pos = d_pos;
  }
  return run_chunks();
}

}  // namespace mrag

using namespace mrag;

extern "C" {

int mrag_ivf_search_range(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device,
                          int nprobe, int k, float min_score, const int64_t* exclude_rows, int exclude_is_device,
                          float* out_scores, int64_t* out_ids, int64_t* out_counts, int out_is_device, void* stream_) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  MRAG_TRY(ivf_check_range_args(nq, k, nprobe, min_score, out_counts));
  IvfSearch s{ix, (hipStream_t)stream_, nq, k, nprobe, queries, q_dtype, normalize, queries_is_device, out_scores, out_ids, out_is_device};
  s.mode = IVF_RANGE; s.floor = min_score; s.out_counts = out_counts;
  MRAG_TRY(s.begin());
  if (nq == 0) return MRAG_OK;
  const int64_t* d_excl = nullptr;
  if (exclude_rows) {
    MRAG_TRY(ix->range.excl.ensure((size_t)nq * 16));
    if (exclude_is_device) {
      d_excl = exclude_rows;
    } else {
      for (int64_t i = 0; i < nq; ++i)
        if (exclude_rows[i] < -1 || exclude_rows[i] >= ix->n)
          return fail(MRAG_ERR_INVALID, "exclude_rows[%lld] = %lld: a local row 0..%lld or -1", (long long)i, (long long)exclude_rows[i], (long long)ix->n - 1);
      MRAG_HIP(hipMemcpyAsync(ix->range.excl.p, exclude_rows, (size_t)nq * 8, hipMemcpyHostToDevice, s.stream));
      d_excl = (const int64_t*)ix->range.excl.p;
    }
  }
  MRAG_TRY(s.run_range(d_excl, -1));
  return s.finish(!out_is_device || !queries_is_device || (exclude_rows && !exclude_is_device));
}

int mrag_ivf_self_join(mrag_handle h, int64_t row0, int64_t n, int nprobe, int k, float min_score, float* out_scores, int64_t* out_ids,
                       int64_t* out_counts, void* stream_) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  MRAG_TRY(ivf_check_range_args(n, k, nprobe, min_score, out_counts));
  if (row0 < 0 || row0 + n > ix->n) return fail(MRAG_ERR_INVALID, "self-join rows [%lld, %lld) outside the %lld stored rows", (long long)row0, (long long)(row0 + n), (long long)ix->n);
  const void* rows = n ? (const void*)(ix->raw + (size_t)row0 * ix->ld) : nullptr;
  IvfSearch s{ix, (hipStream_t)stream_, n, k, nprobe, rows, ix->dtype, 0, 1, out_scores, out_ids, 1};
  s.mode = IVF_RANGE; s.floor = min_score; s.out_counts = out_counts; s.stored_rows = true;
  MRAG_TRY(s.begin());
  if (n == 0) return MRAG_OK;
  MRAG_TRY(ix->range.excl.ensure((size_t)n * 16));
  MRAG_TRY(s.run_range(nullptr, row0));
  return s.finish(false);   // (everything on the device: never synchronises)
}

}  // extern "C"
