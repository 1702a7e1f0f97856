// Filtered IVF search: the allow-set's image over the stored positions, the live lists, AUTO's choice between path P (probe
// the live lists) and path E (the dense filtered search over the rows in arrival order).  State: IvfFilterState (ivf_index.h).
#include "ivf_index.h"

namespace mrag {

// ---- filtered search (path P) -------------------------------------------------------------------------------------
// allow-set over the original rows -> bitset over the stored positions (bit p = row_ids[p] >= 0 && allowed, one ballot per
// 64 positions) + allowed rows per list.  One workgroup per list: a list's positions start on a whole tile and its tiles are
// its own, so it writes only its own words and its count needs no atomics (the same count every run).
__global__ __launch_bounds__(256) void ivf_allow_stored_kernel(const uint32_t* __restrict__ allow, const int64_t* __restrict__ row_ids,
                                                               const int* __restrict__ list_count, const int* __restrict__ list_tile_lo,
                                                               uint32_t* __restrict__ stored, int* __restrict__ counts) {
  __shared__ int part[4];
  const int l = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int lc = list_count[l];
  const int64_t p0 = (int64_t)list_tile_lo[l] * 256;
  int c = 0;
  for (int base = 0; base < lc; base += 256) {          // (covers the list's padding positions too: their bits are 0)
    const int64_t pos = p0 + base + tid;
    const int64_t r = base + tid < lc ? row_ids[pos] : -1;
    const bool a = r >= 0 && ((allow[r >> 5] >> (r & 31)) & 1u);
    const unsigned long long b = __ballot(a);
    if (lane == 0) stored[pos >> 5] = (uint32_t)b;
    if (lane == 32) stored[pos >> 5] = (uint32_t)(b >> 32);
    if (lane == 0) c += __popcll(b);
  }
  if (lane == 0) part[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) counts[l] = part[0] + part[1] + part[2] + part[3];
}

// per-list allowed counts -> live-list bitset (bit l = counts[l] > 0), zero words up to whole 256-list tiles (the dense
// kernels over the centroids read whole tiles); *n_live (zeroed by the caller) += live lists
__global__ void ivf_live_bits_kernel(const int* __restrict__ counts, int nlist, uint32_t* __restrict__ live, int* __restrict__ n_live) {
  const int l = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const unsigned long long b = __ballot(l < nlist && counts[l] > 0);
  if (lane == 0) { live[l >> 5] = (uint32_t)b; if (b) atomicAdd(n_live, (int)__popcll(b)); }
  if (lane == 32) live[l >> 5] = (uint32_t)(b >> 32);
}

// ---- AUTO's choice between path P (probe the live lists) and path E (filtered brute force) ------------------------------
// P scans ~ nprobe * n / nlist rows per query whatever the allow-set; E scans the m allowed rows (the dense filtered search
// over ix->raw, itself masked or compacted).  E when m <= c * nprobe * n / nlist: c_batch for batches, c_stream for a few
// queries (the streaming regime, HBM-bound).  Constants from tools/perf_ivf_filter.py (DESIGN.md "Filtered IVF search").
constexpr double IVF_FILTER_C_BATCH = 8.0;     // 10 000 queries: E and P cross at 5-10 % of the rows (c ~ 9)
constexpr double IVF_FILTER_C_STREAM = 24.0;   // 1 and 16 queries: they cross at ~20-25 % (c ~ 25)
constexpr int64_t IVF_FILTER_STREAM_NQ = 16;   // batches up to this many queries count as the streaming regime
// (k and dim do not enter: both paths pay them alike, the dot products per row and the top-k per query)
static int ivf_choose_filter_path(int64_t nq, int nprobe, int nlist, int64_t n, int64_t m) {
  if (nprobe >= nlist) return MRAG_IVF_FILTER_EXACT;
  const double probed = (double)nprobe * (double)n / (double)nlist;
  return (double)m <= (nq <= IVF_FILTER_STREAM_NQ ? IVF_FILTER_C_STREAM : IVF_FILTER_C_BATCH) * probed ? MRAG_IVF_FILTER_EXACT : MRAG_IVF_FILTER_PROBE;
}

// (after filter_upload) the allow-set's image over the stored positions and the allowed rows per list
static int ivf_filter_stored(IvfIndex* ix, hipStream_t stream) {
  IvfFilterState& w = ix->filter;
  MRAG_TRY(w.fstored.ensure((size_t)(ix->n_sorted / 32) * 4));
  MRAG_TRY(w.flist.ensure(((size_t)2 * ix->nlist + 4 + (size_t)bf_round_rows(ix->nlist) / 32) * 4));
  hipLaunchKernelGGL(ivf_allow_stored_kernel, dim3((unsigned)ix->nlist), dim3(256), 0, stream, (const uint32_t*)w.fw.fbits.p,
                     (const int64_t*)ix->row_ids, (const int*)ix->d_list_count.p, (const int*)ix->d_list_tile_lo.p,
                     (uint32_t*)w.fstored.p, w.counts());
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

static int check_ivf_allow_args(IvfIndex* ix, const void* allow, int64_t allow_rows, int allow_format, int path) {
  MRAG_TRY(check_allow_args(allow_rows, ix->n, allow_format, path, "IVF filter"));
  if (!allow && ix->n > 0) return fail(MRAG_ERR_INVALID, "allow is NULL");
  return MRAG_OK;
}

// The allow-set of a filtered search, uploaded; *chosen = the path it runs, *m = its allowed rows (-1: path P, known on the
// device only).  ev_begin, the search's start, is recorded in filter_upload: behind the host-side packing of a host allow-set.
static int ivf_filter_upload(const IvfSearch& s, const void* allow, int allow_format, int allow_is_device, int path, int* chosen, int64_t* m) {
  IvfIndex* ix = s.ix;
  // path P runs the score-segment regime only, every chunk without a host round trip (IvfChunk::plan's no_sync case);
  // where that does not hold (nprobe == nlist, MRAG_IVF_SCORES_MB = 0, segments too big) the search runs path E
  const int64_t cap = ivf_scores_cap();
  const bool probe_fits = cap > 0 && s.nprobe < ix->nlist && s.chunk * s.nprobe * ivfs_pitch(ix->max_list_rows) * 4 <= cap;
  MRAG_TRY(filter_upload(ix->filter.fw, allow, ix->n, allow_format, allow_is_device, path != MRAG_IVF_FILTER_PROBE, m, ix->ev_begin, s.stream));
  *chosen = path != MRAG_IVF_FILTER_AUTO ? path : ivf_choose_filter_path(s.nq, s.nprobe, ix->nlist, ix->n, *m);
  if (!probe_fits) *chosen = MRAG_IVF_FILTER_EXACT;
  if (*chosen == MRAG_IVF_FILTER_EXACT && *m < 0) {   // (forced P that cannot run as P, device allow-set: E needs the count)
    int hm = 0;
    MRAG_HIP(hipMemcpyAsync(&hm, ix->filter.fw.fwork.p, sizeof(int), hipMemcpyDeviceToHost, s.stream));
    MRAG_HIP(hipStreamSynchronize(s.stream));
    *m = hm;
  }
  return MRAG_OK;
}

// Path E, or the empty result of an allow-set without rows (m == 0): one chunk, whatever nq -- its outputs, its queries,
// its scan events cev[0..1].
static int ivf_filtered_exact(IvfSearch& s, int64_t m) {
  IvfIndex* ix = s.ix;
  s.chunk = s.nq;
  IvfChunk e(s, 0);
  MRAG_TRY(e.stage_outputs());
  if (m == 0) {                      // nothing allowed: no search kernel
    MRAG_HIP(hipEventRecord(e.ev_scan0, s.stream));
    MRAG_TRY(launch_fill_empty(e.d_sc, e.d_id, s.nq * s.k, s.stream));
    MRAG_HIP(hipEventRecord(e.ev_scan1, s.stream));
  } else {
    // the dense filtered search over the rows in arrival order (ix->raw: whole zeroed 256-row tiles), ids = row + id_base
    MRAG_TRY(e.prepare_queries());
    BfLaunch a = ivf_launch(ix, ix->raw, ix->n, ix->qbuf.p, s.nq, s.stream);
    a.k = s.k; a.out_scores = e.d_sc; a.out_ids = e.d_id; a.id_base = ix->id_base;
    a.ev_k2_begin = e.ev_scan0; a.ev_k2_end = e.ev_scan1;
    MRAG_TRY(filter_search(ix->filter.fw, a, filter_choose_path(s.nq, s.k, ix->n, m, ix->ld), m, s.stream));
  }
  ix->n_chunks = 1;
  return e.copy_back();
}

// Path P: allow-set -> stored positions + per-list counts; liveness from those counts or the caller's (sharded: global)
static int ivf_filtered_probe(IvfSearch& s, const int32_t* list_allowed, int allow_is_device) {
  IvfIndex* ix = s.ix;
  IvfFilterState& w = ix->filter;
  const int nlist = ix->nlist;
  hipStream_t stream = s.stream;
  MRAG_TRY(ivf_filter_stored(ix, stream));
  const int* cnt = w.counts();
  if (list_allowed && allow_is_device) {        // (list_allowed lives where the allow-set does)
    cnt = list_allowed;
  } else if (list_allowed) {
    if (!w.ev_lallow) MRAG_TRY(w.ev_lallow.create(false));
    else MRAG_HIP(hipEventSynchronize(w.ev_lallow));   // the previous copy out of the staging buffer is done
    MRAG_TRY(w.h_lallow.ensure((size_t)nlist * 4));
    memcpy(w.h_lallow.p, list_allowed, (size_t)nlist * 4);
    MRAG_HIP(hipMemcpyAsync(w.caller(nlist), w.h_lallow.p, (size_t)nlist * 4, hipMemcpyHostToDevice, stream));
    MRAG_HIP(hipEventRecord(w.ev_lallow, stream));
    cnt = w.caller(nlist);
  }
  MRAG_HIP(hipMemsetAsync(w.nlive(nlist), 0, 4, stream));
  hipLaunchKernelGGL(ivf_live_bits_kernel, dim3((unsigned)(bf_round_rows(nlist) / 256)), dim3(256), 0, stream, cnt, nlist, w.live(nlist),
                     w.nlive(nlist));
  MRAG_HIP(hipGetLastError());
  s.mode = IVF_FILTERED; s.live_bits = w.live(nlist); s.stored_bits = (const uint32_t*)w.fstored.p;
  MRAG_TRY(s.run_chunks());
  // the figures last_filter reports, kept apart from the words the next call overwrites (no sync here)
  MRAG_TRY(w.flast.ensure(8));
  MRAG_HIP(hipMemcpyAsync(w.flast.p, w.fw.fwork.p, 4, hipMemcpyDeviceToDevice, stream));
  MRAG_HIP(hipMemcpyAsync((int*)w.flast.p + 1, w.nlive(nlist), 4, hipMemcpyDeviceToDevice, stream));
  return MRAG_OK;
}

}  // namespace mrag

using namespace mrag;

extern "C" {

int mrag_ivf_choose_filter_path(int64_t nq, int k, int nprobe, int nlist, int64_t total_rows, int64_t allowed_rows, int dim, int* out_path) {
  if (!out_path) return fail(MRAG_ERR_INVALID, "out_path is NULL");
  if (nq < 0 || k <= 0 || nprobe <= 0 || nlist <= 0 || total_rows < 0 || allowed_rows < 0 || allowed_rows > total_rows || dim <= 0)
    return fail(MRAG_ERR_INVALID, "bad nq / k / nprobe / nlist / rows / dim");
  *out_path = ivf_choose_filter_path(nq, nprobe, nlist, total_rows, allowed_rows);
  return MRAG_OK;
}

int mrag_ivf_allowed_per_list(mrag_handle h, const void* allow, int64_t allow_rows, int allow_format, int allow_is_device,
                              int32_t* out_counts, int out_is_device, void* stream_) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  MRAG_TRY(check_ivf_allow_args(ix, allow, allow_rows, allow_format, MRAG_IVF_FILTER_AUTO));
  if (!out_counts) return fail(MRAG_ERR_INVALID, "out_counts is NULL");
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  MRAG_TRY(ivf_finalize(ix, stream));
  MRAG_TRY(ivf_wait_previous(ix, stream));
  int64_t m = -1;
  MRAG_TRY(filter_upload(ix->filter.fw, allow, ix->n, allow_format, allow_is_device, false, &m, ix->ev_count_begin, stream));
  MRAG_TRY(ivf_filter_stored(ix, stream));
  MRAG_HIP(hipMemcpyAsync(out_counts, ix->filter.counts(), (size_t)ix->nlist * 4, out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
  ix->timed = false;
  MRAG_TRY(ivf_record_end(ix, stream));
  if (!out_is_device || !allow_is_device) MRAG_HIP(hipStreamSynchronize(stream));
  return MRAG_OK;
}

int mrag_ivf_search_filtered(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device, int nprobe,
                             int k, const void* allow, int64_t allow_rows, int allow_format, int allow_is_device,
                             const int32_t* list_allowed, int path, float* out_scores, int64_t* out_ids, int out_is_device,
                             void* stream_) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  MRAG_TRY(ivf_check_nq_k(nq, k, nprobe));
  MRAG_TRY(check_ivf_allow_args(ix, allow, allow_rows, allow_format, path));
  IvfSearch s{ix, (hipStream_t)stream_, nq, k, nprobe, queries, q_dtype, normalize, queries_is_device, out_scores, out_ids, out_is_device};
  MRAG_TRY(s.begin());
  if (nq == 0) return MRAG_OK;
  IvfFilterState& w = ix->filter;
  w.last_fpath = -1;
  int chosen = 0;
  int64_t m = -1;
  MRAG_TRY(ivf_filter_upload(s, allow, allow_format, allow_is_device, path, &chosen, &m));
  MRAG_TRY(s.start(false));
  MRAG_TRY(ivf_grow_cev(ix, 1));
  const bool exact = chosen == MRAG_IVF_FILTER_EXACT || m == 0;
  MRAG_TRY(exact ? ivf_filtered_exact(s, m) : ivf_filtered_probe(s, list_allowed, allow_is_device));
  MRAG_TRY(s.finish(!out_is_device || !queries_is_device));
  w.last_fpath = chosen;
  w.last_fallowed = m;
  w.last_flive = !exact ? -1 : m == 0 ? 0 : -2;   // (P: on the device; nothing allowed: no live list; E: not computed)
  return MRAG_OK;
}

int mrag_ivf_last_filter(mrag_handle h, int* out_path, int64_t* out_allowed, int* out_live_lists) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  IvfFilterState& w = ix->filter;
  if (w.last_fpath < 0) return fail(MRAG_ERR_INVALID, "no completed filtered search on this index");
  MRAG_TRY(use_device(ix->device));
  if (w.last_fallowed < 0 || w.last_flive == -1) {   // path P: still on the device
    MRAG_HIP(hipEventSynchronize(ix->ev_end));
    int h[2] = {0, 0};
    MRAG_HIP(hipMemcpy(h, w.flast.p, 8, hipMemcpyDeviceToHost));
    if (w.last_fallowed < 0) w.last_fallowed = h[0];
    if (w.last_flive == -1) w.last_flive = h[1];
  }
  if (out_path) *out_path = w.last_fpath;
  if (out_allowed) *out_allowed = w.last_fallowed;
  if (out_live_lists) *out_live_lists = w.last_flive;
  return MRAG_OK;
}

}  // extern "C"
