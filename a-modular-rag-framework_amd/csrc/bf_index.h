// The host side of the dense index, for the bf_*.hip sources that hold an mrag_index_* entry point: the BfIndex object, the
// DenseSearch call object, the two internal searches over an index pointer (bf_index.hip) and the small pieces the composite
// searches are built from -- argument checks, ListScratch, OutTriple, scatter_rows, LastCall.  Host only; the
// kernels' shared declarations are in bf_kernels.h.
#pragma once
#include "bf_kernels.h"

namespace mrag {

// ---- argument checks ----
// nq and k of the exact dense searches
static inline int check_nq_k(int64_t nq, int k) {
  if (nq < 0) return fail(MRAG_ERR_INVALID, "nq < 0");
  if (k <= 0) return fail(MRAG_ERR_INVALID, "k must be positive");
  if (k > KMAX_WIDE) return fail(MRAG_ERR_UNSUPPORTED, "k = %d exceeds the top-k limit %d (see mrag_index_max_k)", k, KMAX_WIDE);
  return MRAG_OK;
}

// The buffers (null_buffer: one of the call's mandatory pointers is NULL), the query dtype and the batch size of a call
// over nq > 0 query rows, which `noun` names ("queries" / "questions"); *esz = bytes per query element.
static inline int check_query_args(bool null_buffer, int q_dtype, int64_t nq, const char* noun, size_t* esz) {
  if (null_buffer) return fail(MRAG_ERR_INVALID, "NULL buffer");
  *esz = dtype_size(q_dtype);
  if (!*esz) return fail(MRAG_ERR_INVALID, "unknown query dtype %d", q_dtype);
  if (nq > (1ll << 26)) return fail(MRAG_ERR_UNSUPPORTED, "nq too large for one call; batch the %s", noun);
  return MRAG_OK;
}

// A CSR pointer array ptr[0 .. n]: starts at 0, never decreases.  `name` is the array's, `unit` what one entry stands for.
static inline int check_csr(const int64_t* ptr, int64_t n, const char* name, const char* unit) {
  if (ptr[0] != 0) return fail(MRAG_ERR_INVALID, "%s[0] = %lld, not 0 (%s 0)", name, (long long)ptr[0], unit);
  for (int64_t i = 0; i < n; ++i)
    if (ptr[i + 1] < ptr[i])
      return fail(MRAG_ERR_INVALID, "%s decreases at %s %lld (%lld -> %lld)", name, unit, (long long)i, (long long)ptr[i], (long long)ptr[i + 1]);
  return MRAG_OK;
}

// ---- pieces of a call ----
// n (id, score) list entries in one device buffer, laid out (int64 ids | float scores)
struct ListScratch {
  int64_t* ids = nullptr;
  float* scores = nullptr;
  int bind(DevBuf& buf, size_t n) {
    MRAG_TRY(buf.ensure(std::max<size_t>(n, 1) * 12));
    ids = (int64_t*)buf.p;
    scores = (float*)(ids + n);
    return MRAG_OK;
  }
};

// The device side of n (score, id, optional int32 third) outputs: the caller's device buffers, or `scratch` laid out
// (ids | scores | third) with one copy_back for a caller on the host.  keep_third: the third array is kept on the device
// (in scratch) also when the caller does not ask for it.
struct OutTriple {
  float* scores = nullptr;
  int64_t* ids = nullptr;
  int32_t* third = nullptr;     // NULL: not wanted
  size_t n = 0;
  float* h_scores = nullptr;    // host outputs to copy back to (h_third may be NULL); all NULL for device outputs
  int64_t* h_ids = nullptr;
  int32_t* h_third = nullptr;

  int bind(DevBuf& scratch, size_t n_, float* out_scores, int64_t* out_ids, int32_t* out_third, int out_is_device, bool keep_third) {
    n = n_;
    scores = out_scores; ids = out_ids; third = out_third;
    if (out_is_device && !keep_third) return MRAG_OK;
    MRAG_TRY(scratch.ensure(n * 16));
    int32_t* s_third = (int32_t*)((char*)scratch.p + n * 12);
    if (!out_is_device) {
      h_scores = out_scores; h_ids = out_ids; h_third = out_third;
      ids = (int64_t*)scratch.p;
      scores = (float*)(ids + n);
      third = nullptr;
    }
    if (!third && (out_third || keep_third)) third = s_third;
    return MRAG_OK;
  }

  // host outputs: copied back, the call returns when they have landed
  int copy_back(hipStream_t stream) const {
    if (!h_scores) return MRAG_OK;
    MRAG_HIP(hipMemcpyAsync(h_scores, scores, n * 4, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipMemcpyAsync(h_ids, ids, n * 8, hipMemcpyDeviceToHost, stream));
    if (h_third) MRAG_HIP(hipMemcpyAsync(h_third, third, n * 4, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipStreamSynchronize(stream));
    return MRAG_OK;
  }
};

// result rows g = 0 .. n (k entries each, on the host) -> rows order[g] of the caller's outputs
template <class Index>
static inline void scatter_rows(const Index* order, int64_t n, int k, const float* scores, const int64_t* ids, float* out_scores,
                                int64_t* out_ids) {
  for (int64_t g = 0; g < n; ++g) {
    const size_t q = (size_t)order[g];
    memcpy(out_scores + q * k, scores + (size_t)g * k, (size_t)k * 4);
    memcpy(out_ids + q * k, ids + (size_t)g * k, (size_t)k * 8);
  }
}

// Three figures of an entry point's last completed call.  open() where the call starts to change the index: from there
// until close() there is nothing to read; a call refused before open() leaves the previous record readable.
struct LastCall {
  int64_t v[3] = {-1, -1, -1};
  void open() { v[0] = -1; }
  void close(int64_t a, int64_t b, int64_t c) { v[0] = a; v[1] = b; v[2] = c; }
  int read(const char* what, int64_t* a, int64_t* b, int64_t* c) const {
    if (v[0] < 0) return fail(MRAG_ERR_INVALID, "no completed %s on this index", what);
    if (a) *a = v[0];
    if (b) *b = v[1];
    if (c) *c = v[2];
    return MRAG_OK;
  }
};

// ---- what each composite search keeps on the index ----
// per-question allow-sets (mrag_index_search_sets, bf_filter_batch.hip)
struct SetsState {
  DevBuf q;          // prepared queries + one zero row (not qbuf, as rr_q)
  DevBuf plan;       // the uploaded plan (descriptors | question list | segment table)
  DevBuf rows;       // the scanned sets' rows
  DevBuf S;          // the score segments
  LastCall last;     // scanned questions, routed questions, descriptors
};

// grouped queries (mrag_index_search_groups, bf_groups.hip)
struct GroupsState {
  DevBuf in;                    // the search's [nq][k] lists
  DevBuf ptr;                   // group_ptr on the device, uploaded from `host`, which outlives the call
  DevBuf out;                   // the merged rows of a call with host outputs (ids | scores | which)
  std::vector<int64_t> host;
  LastCall last;                // queries, questions, entries of the largest question
};

// neighbour expansion (mrag_index_expand_neighbors, bf_neighbors.hip); its row keys are CollapseState's
struct NeighborsState {
  DevBuf seeds;                 // host seeds on the device
  DevBuf out;                   // the rows of a call with host outputs (ids | scores | dist | seed) ...
  std::vector<char> host;       // ... and their host copy, downloaded in one piece
  LastCall last;                // questions, entries of the largest question, window
};

// collapsed search (mrag_index_search_collapsed, bf_collapse.hip)
struct CollapseState {
  DevBuf keys;                            // the row keys on the device
  int64_t n = -1, m = 0, distinct = 0;    // the rows they were set for (-1 = none), the largest number of rows that share a
                                          // key and the distinct keys (counted on the host when the keys are set)
  DevBuf in, redo;                        // round 0's [nq][scan_k] lists and a redo round's one list
  DevBuf mask;                            // the redo allow-set bitset
  DevBuf words;                           // the per-query {heads, valid} words, with their host copy:
  std::vector<int32_t> host;
  DevBuf out;                             // the [nq][k] results (ids | scores | keys) the caller's buffers do not hold
  LastCall last;                          // scan_k, redone queries, redo searches
};

struct BfIndex : Object {
  int dim = 0, ld = 0, metric = 0, dtype = MRAG_F16;
  int64_t n = 0, cap_rows = 0, id_base = 0;
  DevArray<uint16_t> rows;                  // [cap_rows][ld]
  DevBuf qbuf, lists, counts, stage_in, out_sc, out_id, clock;
  DevBuf rslots, out_cnt;                   // range search: per-(workgroup, query) count slots; counts for host outputs
  FilterWork fw;                            // filtered search: allow bitset, counts, compacted rows
  int last_fpath = -1;                      // path of the last filtered search (MRAG_FILTER_MASK / _COMPACT), -1 = none
  int64_t last_fallowed = -1;               // its allowed-row count; -1 = still on the device (fwork word 0, read on demand)
  Event ev[4];
  bool timed = false, want_clock = false;
  void* q_cleared_buf = nullptr;            // query buffer bookkeeping: rows [q_dirty_rows, q_cleared_rows) are known to be zero
  int64_t q_cleared_rows = 0, q_dirty_rows = 0;
  // fp8 scan copy (mrag_index_enable_fp8): rows8 [cap_rows][ld8], kept in step with `rows` by add / reserve
  bool fp8 = false;
  int ld8 = 0;
  DevArray<uint8_t> rows8;
  DevBuf qbuf8, cand;                       // quantised queries [nq padded][ld8]; candidates (fp8 scores | local rows)
  int last_refine = -1, last_regime = -1;   // of the last mrag_index_search_fp8
  DevBuf rr_q;                              // batched re-rank: its prepared queries [n_questions][ld] -- not qbuf, whose zero-padding
                                            // bookkeeping (q_cleared_*, q_dirty_rows) a 10 000-question re-rank must not disturb
  SetsState sets;
  GroupsState groups;
  NeighborsState neighbors;
  CollapseState collapse;
};

// One call of a dense search entry point: the plumbing bf_search, search_allowed and mrag_index_search_fp8 share around
// their own work.
struct DenseSearch {
  BfIndex* ix;
  int64_t nq;
  int k;
  float* out_scores;
  int64_t* out_ids;
  int out_is_device;
  hipStream_t stream;
  int64_t* out_counts = nullptr;   // range search only: per-query counts [nq], in the memory space of the other outputs
  size_t esz = 0;             // bytes per query element
  float* d_sc = nullptr;      // the results on the device: the caller's buffers, or out_sc / out_id for host outputs
  int64_t* d_id = nullptr;
  int64_t* d_cnt = nullptr;   // (range search) the counts on the device: out_counts, or out_cnt for host outputs

  // After the entry point's own argument checks, for nq > 0: the buffers (allow_null: a filtered search's NULL allow-set
  // over a non-empty index), the query dtype and the batch size, then the device.  `last` (the entry point's record of its
  // last search) reads -1 from here until the search completes.
  int begin(const void* queries, int q_dtype, bool allow_null = false, int* last = nullptr) {
    // error precedence as ever: "NULL buffer" wins over "allow is NULL", which wins over the dtype and batch-size errors --
    // so the allow check stands in front of check_query_args but passes a NULL buffer on to it
    const bool null_buffer = !queries || !out_scores || !out_ids;
    if (!null_buffer && allow_null) return fail(MRAG_ERR_INVALID, "allow is NULL");
    MRAG_TRY(check_query_args(null_buffer, q_dtype, nq, "queries", &esz));
    MRAG_TRY(use_device(ix->device));
    ix->timed = false;
    if (last) *last = -1;
    d_sc = out_scores;
    d_id = out_ids;
    d_cnt = out_counts;
    if (!out_is_device) {
      MRAG_TRY(ix->out_sc.ensure((size_t)nq * k * 4));
      MRAG_TRY(ix->out_id.ensure((size_t)nq * k * 8));
      d_sc = (float*)ix->out_sc.p;
      d_id = (int64_t*)ix->out_id.p;
      if (out_counts) {
        MRAG_TRY(ix->out_cnt.ensure((size_t)nq * 8));
        d_cnt = (int64_t*)ix->out_cnt.p;
      }
    }
    return MRAG_OK;
  }

  // An empty result: every slot (-inf, -1); the K2 events bracket nothing.
  int fill_empty() {
    MRAG_TRY(launch_fill_empty(d_sc, d_id, nq * k, stream));
    if (d_cnt) MRAG_HIP(hipMemsetAsync(d_cnt, 0, (size_t)nq * 8, stream));
    MRAG_HIP(hipEventRecord(ix->ev[1], stream));
    MRAG_HIP(hipEventRecord(ix->ev[2], stream));
    return MRAG_OK;
  }

  // queries -> storage dtype in ix->qbuf, zero padded to bf_query_rows(nq) rows
  int prep_queries(const void* queries, int q_dtype, int normalize, int queries_is_device) {
    const int64_t nq_pad = bf_query_rows(nq);
    const size_t qbytes = (size_t)nq_pad * ix->ld * 2;
    MRAG_TRY(ix->qbuf.ensure(qbytes));
    const void* qsrc = queries;
    if (!queries_is_device) {
      const size_t bytes = (size_t)nq * ix->dim * esz;
      MRAG_TRY(ix->stage_in.ensure(bytes));
      MRAG_HIP(hipMemcpyAsync(ix->stage_in.p, queries, bytes, hipMemcpyHostToDevice, stream));
      qsrc = ix->stage_in.p;
    }
    // rows [nq, nq_pad) must be zero; only rows an earlier (larger) batch wrote need clearing again, so a stream of
    // equal-sized searches (the online regime: one question per call) pays the fill launch once
    if (ix->qbuf.p != ix->q_cleared_buf || nq_pad > ix->q_cleared_rows) {
      MRAG_HIP(hipMemsetAsync(ix->qbuf.p, 0, qbytes, stream));
      ix->q_cleared_buf = ix->qbuf.p; ix->q_cleared_rows = nq_pad; ix->q_dirty_rows = 0;
    } else if (ix->q_dirty_rows > nq) {
      MRAG_HIP(hipMemsetAsync((char*)ix->qbuf.p + (size_t)nq * ix->ld * 2, 0, (size_t)(ix->q_dirty_rows - nq) * ix->ld * 2, stream));
      ix->q_dirty_rows = nq;
    }
    ix->q_dirty_rows = std::max<int64_t>(ix->q_dirty_rows, nq);
    return launch_prep_rows(qsrc, q_dtype, nq, ix->dim, ix->qbuf.p, ix->ld, ix->dtype,
                            normalize && ix->metric == MRAG_METRIC_COSINE, stream);
  }

  // the launch of a search for k_launch results per query over all stored rows (prepared queries in ix->qbuf)
  BfLaunch launch(int k_launch, float* sc, int64_t* ids) const {
    BfLaunch a;
    a.corpus = ix->rows;
    a.queries = (const uint16_t*)ix->qbuf.p;
    a.ld = ix->ld; a.dtype = ix->dtype; a.k = k_launch;
    a.nq = nq; a.n_rows = ix->n;
    a.id_base = ix->id_base;
    a.out_scores = sc; a.out_ids = ids;
    a.lists = &ix->lists; a.counts = &ix->counts;
    a.stream = stream;
    a.ev_k2_begin = ix->ev[1]; a.ev_k2_end = ix->ev[2];
    return a;
  }

  // the exact search's launch, with the batch kernel's clock stamps when they are asked for (mrag_index_measure_clock)
  int exact_launch(BfLaunch* a) {
    *a = launch(k, d_sc, d_id);
    if (ix->want_clock) {
      MRAG_TRY(ix->clock.ensure(64));
      MRAG_HIP(hipMemsetAsync(ix->clock.p, 0, 64, stream));
      a->clock = (long long*)ix->clock.p;
    }
    return MRAG_OK;
  }

  // the search's device work is done: ev[3], the search is timed
  int end() {
    MRAG_HIP(hipEventRecord(ix->ev[3], stream));
    ix->timed = true;
    return MRAG_OK;
  }

  // host outputs: copied back, the call returns when they have landed
  int copy_back() const {
    if (out_is_device) return MRAG_OK;
    MRAG_HIP(hipMemcpyAsync(out_scores, d_sc, (size_t)nq * k * 4, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipMemcpyAsync(out_ids, d_id, (size_t)nq * k * 8, hipMemcpyDeviceToHost, stream));
    if (out_counts) MRAG_HIP(hipMemcpyAsync(out_counts, d_cnt, (size_t)nq * 8, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipStreamSynchronize(stream));
    return MRAG_OK;
  }
};

// ---- the two searches the entry points and the composite searches share (bf_index.hip) ----
// the body of mrag_index_search
int bf_search(BfIndex* ix, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device, int k,
              float* out_scores, int64_t* out_ids, int out_is_device, hipStream_t stream);
// mrag_index_search_filtered (floor NULL) and mrag_index_search_range (floor = &min_score).  The filtered search needs an
// allow-set over a non-empty index; the range search takes NULL for "every row" and then runs the plain search, and
// records its filter path only when it had an allow-set.
int search_allowed(BfIndex* ix, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device, int k,
                   const float* floor, const void* allow, int64_t allow_rows, int allow_format, int allow_is_device, int path,
                   float* out_scores, int64_t* out_ids, int64_t* out_counts, int out_is_device, hipStream_t stream);

}  // namespace mrag
