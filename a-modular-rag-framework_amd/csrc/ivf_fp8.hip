// The fp8 scan copy of the IVF-flat index: built next to the regrouped rows, scanned by mrag_ivf_search_fp8 and re-ranked
// exactly against the 16-bit rows.  State: IvfFp8State (ivf_index.h).
#include "ivf_index.h"

namespace mrag {

// fp8 bytes of the original rows [row0, row0 + n) (mrag_ivf_get_rows_fp8): out [n][dim] from the regrouped copy through inv
__global__ void gather_rows8_kernel(const uint8_t* __restrict__ sorted8, int ld8, const int64_t* __restrict__ inv, int64_t row0,
                                    int64_t n, int dim, uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * dim) return;
  const int64_t r = i / dim;
  out[i] = sorted8[(size_t)inv[row0 + r] * ld8 + (i - r * dim)];
}

// every byte of dst [n_sorted][ld8] is written (pad rows of `sorted` are zero, pad columns are zeroed by the kernel)
int ivf_build_sorted8(IvfIndex* ix, const uint16_t* sorted, int64_t n_sorted, DevArray<uint8_t>& dst, hipStream_t stream) {
  MRAG_TRY(dst.alloc((size_t)n_sorted * ix->f8.ld8, "the fp8 rows"));
  return launch_quant_rows_fp8(sorted, ix->ld, ix->dtype == MRAG_BF16 ? 1 : 0, n_sorted, dst, ix->f8.ld8, stream);
}

}  // namespace mrag

using namespace mrag;

extern "C" {

// ---- fp8 scan copy + exact re-rank (contract in include/mrag.h) ---------------------------------------------------
int mrag_ivf_enable_fp8(mrag_handle h) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (ix->metric != MRAG_METRIC_COSINE) return fail(MRAG_ERR_INVALID, "the fp8 scan copy serves cosine indexes only");
  if (ix->f8.on) return MRAG_OK;
  MRAG_TRY(use_device(ix->device));
  ix->f8.on = true;
  if (ix->n > 0) {
    // rows already stored (adds and searches on any stream): settle them, build the copy on the null stream -- with the
    // regroup when that is due anyway --, finish it here (a one-off), then move it into place
    DevArray<uint8_t> sorted8;
    int st = hipDeviceSynchronize() == hipSuccess ? MRAG_OK : fail(MRAG_ERR_HIP, "hipDeviceSynchronize failed");
    if (st == MRAG_OK) st = ix->dirty ? ivf_finalize(ix, nullptr) : ivf_build_sorted8(ix, ix->sorted, ix->n_sorted, sorted8, nullptr);
    if (st == MRAG_OK && hipStreamSynchronize(nullptr) != hipSuccess) st = fail(MRAG_ERR_HIP, "building the fp8 rows failed");
    if (st != MRAG_OK) { ix->f8.on = false; return st; }
    if (sorted8) ix->f8.sorted8.swap(sorted8);
  }
  return MRAG_OK;
}

int mrag_ivf_get_rows_fp8(mrag_handle h, int64_t row0, int64_t n, uint8_t* out, int out_is_device, void* stream_) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (!ix->f8.on) return fail(MRAG_ERR_INVALID, "no fp8 scan copy (mrag_ivf_enable_fp8)");
  if (row0 < 0 || n < 0 || row0 + n > ix->n) return fail(MRAG_ERR_INVALID, "row range [%lld,%lld) outside [0,%lld)", (long long)row0, (long long)(row0 + n), (long long)ix->n);
  if (n == 0) return MRAG_OK;
  if (!out) return fail(MRAG_ERR_INVALID, "out is NULL");
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  MRAG_TRY(ivf_finalize(ix, stream));
  MRAG_TRY(ivf_wait_previous(ix, stream));
  MRAG_TRY(ivf_ensure_inv_pos(ix, stream));
  const int64_t tot = n * ix->dim;
  uint8_t* d_out = out;
  DevBuf tmp;
  if (!out_is_device) { MRAG_TRY(tmp.ensure((size_t)tot)); d_out = (uint8_t*)tmp.p; }
  hipLaunchKernelGGL(gather_rows8_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, (const uint8_t*)ix->f8.sorted8, ix->f8.ld8,
                     (const int64_t*)ix->range.inv_pos.p, row0, n, ix->dim, d_out);
  MRAG_HIP(hipGetLastError());
  if (!out_is_device) {
    MRAG_HIP(hipMemcpyAsync(out, d_out, (size_t)tot, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipStreamSynchronize(stream));
  }
  ix->timed = false;
  return ivf_record_end(ix, stream);   // (inv_pos is in use on `stream` until here)
}

int mrag_ivf_search_fp8(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device, int nprobe,
                        int k, int refine, float* out_scores, int64_t* out_ids, int out_is_device, void* stream_) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (!ix->f8.on) return fail(MRAG_ERR_INVALID, "no fp8 scan copy on this index (mrag_ivf_enable_fp8)");
  if (nq < 0 || nprobe <= 0) return fail(MRAG_ERR_INVALID, "bad nq / nprobe");
  if (k < 1 || k > FP8_MAX_REFINE) return fail(MRAG_ERR_INVALID, "fp8 search serves 1 <= k <= %d, got %d", FP8_MAX_REFINE, k);
  if (refine == 0) MRAG_TRY(mrag_index_fp8_default_refine(k, &refine));
  if (refine < k || refine > FP8_MAX_REFINE) return fail(MRAG_ERR_INVALID, "refine = %d outside k..%d (k = %d)", refine, FP8_MAX_REFINE, k);
  IvfSearch s{ix, (hipStream_t)stream_, nq, k, nprobe, queries, q_dtype, normalize, queries_is_device, out_scores, out_ids, out_is_device};
  s.mode = IVF_FP8; s.refine = refine;
  MRAG_TRY(s.begin());
  if (nq == 0) return MRAG_OK;
  MRAG_TRY(s.refuse_fused());
  MRAG_TRY(s.start());
  MRAG_TRY(s.run_chunks());
  MRAG_TRY(s.finish(!out_is_device || !queries_is_device));
  ix->f8.last_refine = refine;
  return MRAG_OK;
}

int mrag_ivf_last_fp8(mrag_handle h, int* out_refine) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (ix->f8.last_refine < 0) return fail(MRAG_ERR_INVALID, "no completed fp8 search on this index");
  if (out_refine) *out_refine = ix->f8.last_refine;
  return MRAG_OK;
}

}  // extern "C"
