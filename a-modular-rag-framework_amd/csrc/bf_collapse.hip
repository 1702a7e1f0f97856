// Collapsed search (mrag_index_search_collapsed): the top-k KEYS of a query, each key by its best row.  Every stored row
// carries one int32 key (key_of[row], 0 <= key < 2^31).  A search leaves a query's list of <= scan_k (score, id) entries in
// the index's declared order (score desc, row asc), padded with (-inf, -1); the two kernels here turn lists into heads:
//
//   collapse_heads_kernel   one workgroup (256 threads = 4 waves) per query, thread e owns entry e of the list (scan_k <= 256).
//       key[e]   = key_of[id - id_base] for a valid entry, -1 for padding (and for a row outside the index, which the search
//                  never returns: the bound is checked before key_of is read)
//       head[e]  = valid and no earlier entry of the list has key[e]: the list is sorted, so the first entry of a key is its
//                  representative.  The test walks the earlier entries in LDS at a WAVE-UNIFORM address j (every lane reads
//                  the same word: a broadcast, conflict free), up to the last entry its wave owns, and masks j < e per lane.
//       position = heads before e = popcount of the wave's 64-BIT ballot below the lane + the totals of the earlier waves
//                  (gfx950 waves are 64 wide: a 32-bit mask would be right up to entry 31 and wrong behind it).
//       output   = head e goes to slot prev + position of the query's [k] outputs when that slot is < k (prev: the heads
//                  earlier rounds wrote, 0 in round 0); round 0 also writes (-inf, -1, -1) into the slots behind its heads.
//       words[q] = {prev + heads of this list, valid entries of this list}: the host reads these to decide on a redo.
//       LDS: 256 keys + 2 x 4 wave totals = 1 056 bytes, static; 20 VGPRs, no scratch.  A query's outputs depend on its own
//       list alone.
//
//   collapse_mask_kernel    the allow-set of a redo round: bit r = row r's key is not among the query's found keys.  One
//       thread per row, the <= 255 found keys in LDS (again read at a uniform address), one ballot per 64 rows written as two
//       32-bit words by lanes 0 and 32 -- the bitset form of bf_filter.hip (bit r % 32 of word r / 32).  Rows >= n of the
//       last 256-row block are disallowed, so the words cover whole tiles as the filtered search expects.  LDS 1 024 bytes,
//       20 VGPRs, no scratch.
#include "bf_index.h"

namespace mrag {

static_assert(COLLAPSE_MAX_SCAN == 256, "one thread per list entry, one workgroup of 256 threads per query");

__global__ __launch_bounds__(256) void collapse_heads_kernel(const float* __restrict__ in_sc, const int64_t* __restrict__ in_id,
                                                             int scan_k, const int32_t* __restrict__ key_of, int64_t n_rows,
                                                             int64_t id_base, int k, int64_t q0, int append,
                                                             int32_t* __restrict__ words, float* __restrict__ out_sc,
                                                             int64_t* __restrict__ out_id, int32_t* __restrict__ out_key) {
  __shared__ int32_t s_key[COLLAPSE_MAX_SCAN];
  __shared__ int s_heads[4], s_valid[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t q = q0 + blockIdx.x;
  const size_t li = (size_t)blockIdx.x * scan_k;
  const int prev = append ? words[2 * q] : 0;

  float sc = -INFINITY;
  int64_t id = -1;
  int32_t key = -1;
  if (tid < scan_k) {
    sc = in_sc[li + tid];
    id = in_id[li + tid];
    if (!(id == -1 && sc == -INFINITY)) {
      const int64_t row = id - id_base;
      if (row >= 0 && row < n_rows) key = key_of[row];
    }
  }
  s_key[tid] = key;
  __syncthreads();

  bool head = key >= 0;
  const int j_end = min(scan_k, (wv + 1) * 64);      // wave-uniform: the entries up to the last one this wave owns
  for (int j = 0; j < j_end; ++j) {
    const int32_t kj = s_key[j];                     // uniform address: a broadcast
    if (j < tid && kj == key) head = false;
  }
  const unsigned long long hb = __ballot(head), vb = __ballot(key >= 0);
  if (lane == 0) { s_heads[wv] = __popcll(hb); s_valid[wv] = __popcll(vb); }
  __syncthreads();
  int pos = __popcll(hb & ((1ull << lane) - 1ull)), heads = 0, valid = 0;
  for (int w = 0; w < 4; ++w) {
    if (w < wv) pos += s_heads[w];
    heads += s_heads[w];
    valid += s_valid[w];
  }

  const size_t o = (size_t)q * k;
  if (head && prev + pos < k) {
    out_sc[o + prev + pos] = sc;
    out_id[o + prev + pos] = id;
    out_key[o + prev + pos] = key;
  }
  if (!append && tid < k && tid >= heads) {          // round 0: the slots past the heads (k <= 256 = the threads)
    out_sc[o + tid] = -INFINITY;
    out_id[o + tid] = -1;
    out_key[o + tid] = -1;
  }
  if (tid == 0) {                                    // (every thread read `prev` before the barriers above)
    words[2 * q] = prev + heads;
    words[2 * q + 1] = valid;
  }
}

__global__ __launch_bounds__(256) void collapse_mask_kernel(const int32_t* __restrict__ key_of, int64_t n_rows,
                                                            const int32_t* __restrict__ found, const int32_t* __restrict__ word,
                                                            int k, uint32_t* __restrict__ bits) {
  __shared__ int32_t s_found[COLLAPSE_MAX_SCAN];
  const int tid = threadIdx.x, lane = tid & 63;
  const int nf = max(0, min(word[0], k));            // found keys: the query's outputs so far (a redone query has < k)
  s_found[tid] = tid < nf ? found[tid] : -1;
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 256 + tid;
  bool allowed = false;
  if (r < n_rows) {
    const int32_t key = key_of[r];
    allowed = true;
    for (int j = 0; j < nf; ++j)
      if (s_found[j] == key) allowed = false;        // uniform address: a broadcast
  }
  const unsigned long long b = __ballot(allowed);
  if (lane == 0) bits[r >> 5] = (uint32_t)b;
  if (lane == 32) bits[r >> 5] = (uint32_t)(b >> 32);
}

// nq >= 1 lists of scan_k entries each, consecutive behind in_sc / in_id, the lists of the queries q0 .. q0 + nq; words is
// [.][2] and out_* are [.][k], indexed by query.  append = 0: round 0 (slots past the heads become tails); 1: a redo round.
static int launch_collapse_heads(const float* in_sc, const int64_t* in_id, int64_t nq, int scan_k, const int32_t* key_of, int64_t n_rows,
                          int64_t id_base, int k, int64_t q0, int append, int32_t* words, float* out_sc, int64_t* out_id,
                          int32_t* out_key, hipStream_t stream) {
  if (scan_k < 1 || scan_k > COLLAPSE_MAX_SCAN || k < 1 || k > COLLAPSE_MAX_SCAN)
    return fail(MRAG_ERR_UNSUPPORTED, "collapse of %d entries to k = %d: both must lie in [1, %d]", scan_k, k, COLLAPSE_MAX_SCAN);
  if (nq > 2147483647ll) return fail(MRAG_ERR_UNSUPPORTED, "%lld queries exceed one launch", (long long)nq);
  hipLaunchKernelGGL(collapse_heads_kernel, dim3((unsigned)nq), dim3(256), 0, stream, in_sc, in_id, scan_k, key_of, n_rows, id_base, k,
                     q0, append, words, out_sc, out_id, out_key);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

// bits: collapse_mask_words(n_rows) words
static int64_t collapse_mask_words(int64_t n_rows) { return round_up(std::max<int64_t>(n_rows, 1), TM) / 32; }

static int launch_collapse_mask(const int32_t* key_of, int64_t n_rows, const int32_t* found, const int32_t* word, int k, uint32_t* bits,
                         hipStream_t stream) {
  hipLaunchKernelGGL(collapse_mask_kernel, dim3((unsigned)(collapse_mask_words(n_rows) / 8)), dim3(256), 0, stream, key_of, n_rows,
                     found, word, k, bits);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

// The default scan depth of the collapsed search.  With m rows per key at most, the first (k - 1) * m + 1 rows of the
// declared order hold k keys, so at that depth no query is ever redone; the search serves 256 at most, and a depth beyond
// the rows (or below k) buys nothing.  Nobody has measured whether this depth or a shallower scan with an occasional redo
// is faster: tools/perf_search_collapsed.py times both (DESIGN.md §3 "Collapsed search").
static int collapse_default_scan_k(int k, int64_t m, int64_t n) {
  const int64_t safe = std::max<int64_t>(k, (int64_t)(k - 1) * m + 1);
  return (int)std::max<int64_t>(k, std::min<int64_t>(std::min<int64_t>(KMAX_WIDE, n), safe));
}

// scan_k and the row keys of a collapsed search (behind nq and k)
static int collapse_check_args(const BfIndex* ix, int k, int scan_k) {
  if (scan_k != 0 && (scan_k < k || scan_k > KMAX_WIDE))
    return fail(MRAG_ERR_INVALID, "scan_k = %d lies outside [k, %d] = [%d, %d] (0 picks the default)", scan_k, KMAX_WIDE, k, KMAX_WIDE);
  const CollapseState& w = ix->collapse;
  if (w.n < 0 && ix->n > 0) return fail(MRAG_ERR_INVALID, "no row keys set on this index (mrag_index_set_row_keys)");
  if (w.n >= 0 && w.n != ix->n)
    return fail(MRAG_ERR_INVALID, "row keys were set for %lld rows, the index holds %lld: set them again", (long long)w.n, (long long)ix->n);
  return MRAG_OK;
}

// One collapsed search, as its rounds see it
struct CollapseCall {
  BfIndex* ix;
  const void* queries;
  int64_t nq;
  int q_dtype, normalize, queries_is_device, k, scan;
  size_t esz;
  hipStream_t stream;
  OutTriple out;                     // the [nq][k] heads: scores, ids, keys
  int32_t* words = nullptr;          // per query {heads so far, valid entries of its last list}, on the device
  int32_t* hw = nullptr;             // and their host copy, read back after every round
  const int32_t* key_of = nullptr;   // (NULL only over an empty index: no list entry is valid)

  int read_words() const {
    MRAG_HIP(hipMemcpyAsync(hw, words, (size_t)nq * 8, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipStreamSynchronize(stream));
    return MRAG_OK;
  }
  // fewer than k keys, and the list was full (rows may stand behind it)
  bool incomplete(int64_t q) const { return hw[2 * q] < k && hw[2 * q + 1] >= scan; }
};

// ---- round 0: one search of all queries at depth `scan` into `in`, one collapse launch, the words read back -> the incomplete queries
static int collapse_round0(const CollapseCall& c, const ListScratch& in, std::vector<int64_t>& todo) {
  BfIndex* ix = c.ix;
  MRAG_TRY(bf_search(ix, c.queries, c.nq, c.q_dtype, c.normalize, c.queries_is_device, c.scan, in.scores, in.ids, 1, c.stream));
  MRAG_TRY(launch_collapse_heads(in.scores, in.ids, c.nq, c.scan, c.key_of, ix->n, ix->id_base, c.k, 0, 0, c.words, c.out.scores, c.out.ids,
                                 c.out.third, c.stream));
  MRAG_TRY(c.read_words());
  for (int64_t q = 0; q < c.nq; ++q)
    if (c.incomplete(q)) todo.push_back(q);
  return MRAG_OK;
}

// ---- redo rounds: each incomplete query alone over the rows whose key it has not found; every round adds a key
static int collapse_redo(const CollapseCall& c, std::vector<int64_t>& todo, int64_t* searches) {
  if (todo.empty()) return MRAG_OK;
  BfIndex* ix = c.ix;
  CollapseState& w = ix->collapse;
  const int64_t n = ix->n;
  ListScratch one;
  MRAG_TRY(one.bind(w.redo, (size_t)c.scan));
  MRAG_TRY(w.mask.ensure((size_t)collapse_mask_words(n) * 4));
  while (!todo.empty()) {
    for (const int64_t q : todo) {
      MRAG_TRY(launch_collapse_mask(c.key_of, n, c.out.third + (size_t)q * c.k, c.words + 2 * q, c.k, (uint32_t*)w.mask.p, c.stream));
      MRAG_TRY(search_allowed(ix, (const char*)c.queries + (size_t)q * ix->dim * c.esz, 1, c.q_dtype, c.normalize, c.queries_is_device,
                              c.scan, nullptr, w.mask.p, n, MRAG_ALLOW_BITS32, 1, MRAG_FILTER_AUTO, one.scores, one.ids, nullptr, 1,
                              c.stream));
      MRAG_TRY(launch_collapse_heads(one.scores, one.ids, 1, c.scan, c.key_of, n, ix->id_base, c.k, q, 1, c.words, c.out.scores, c.out.ids,
                                     c.out.third, c.stream));
      ++*searches;
    }
    MRAG_TRY(c.read_words());
    std::vector<int64_t> next;
    for (const int64_t q : todo)
      if (c.incomplete(q)) next.push_back(q);
    todo.swap(next);
  }
  return MRAG_OK;
}

}  // namespace mrag

using namespace mrag;

extern "C" {

int mrag_index_set_row_keys(mrag_handle h, const int32_t* keys, int64_t n, int keys_is_device) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  CollapseState& w = ix->collapse;
  if (n < 0) return fail(MRAG_ERR_INVALID, "n < 0");
  if (n == 0 && !keys) { w.n = -1; w.m = 0; w.distinct = 0; return MRAG_OK; }
  if (!keys) return fail(MRAG_ERR_INVALID, "keys is NULL");
  if (n != ix->n) return fail(MRAG_ERR_INVALID, "keys for %lld rows, the index holds %lld", (long long)n, (long long)ix->n);
  MRAG_TRY(use_device(ix->device));
  // the host copy: validated, then sorted to count the distinct keys and the longest run
  std::vector<int32_t> hk((size_t)n);
  if (n > 0) {
    if (keys_is_device) MRAG_HIP(hipMemcpy(hk.data(), keys, (size_t)n * 4, hipMemcpyDeviceToHost));
    else memcpy(hk.data(), keys, (size_t)n * 4);
  }
  for (int64_t r = 0; r < n; ++r)
    if (hk[(size_t)r] < 0) return fail(MRAG_ERR_INVALID, "row %lld has the negative key %d", (long long)r, (int)hk[(size_t)r]);
  // an earlier collapsed search with device outputs may still read the old keys on the caller's stream
  MRAG_HIP(hipDeviceSynchronize());
  MRAG_TRY(w.keys.ensure(std::max<size_t>((size_t)n, 1) * 4));
  if (n > 0) MRAG_HIP(hipMemcpy(w.keys.p, hk.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  std::sort(hk.begin(), hk.end());
  int64_t distinct = 0, longest = 0, run = 0;
  for (int64_t r = 0; r < n; ++r) {
    if (r == 0 || hk[(size_t)r] != hk[(size_t)r - 1]) { ++distinct; run = 0; }
    longest = std::max(longest, ++run);
  }
  w.n = n;
  w.m = longest;
  w.distinct = distinct;
  return MRAG_OK;
}

int mrag_index_search_collapsed(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device,
                                int k, int scan_k, float* out_scores, int64_t* out_ids, int32_t* out_keys, int out_is_device,
                                void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  MRAG_TRY(check_nq_k(nq, k));
  MRAG_TRY(collapse_check_args(ix, k, scan_k));
  if (nq == 0) return MRAG_OK;
  size_t esz = 0;
  MRAG_TRY(check_query_args(!queries || !out_scores || !out_ids, q_dtype, nq, "queries", &esz));
  MRAG_TRY(use_device(ix->device));
  CollapseState& w = ix->collapse;
  w.last.open();
  const int scan = scan_k ? scan_k : collapse_default_scan_k(k, w.m, ix->n);
  CollapseCall c{ix, queries, nq, q_dtype, normalize, queries_is_device, k, scan, esz, (hipStream_t)stream_};
  // the call's buffers: round 0's lists, the words with their host copy, the results (the found keys feed the redo masks, so
  // they are kept also when the caller does not ask for them)
  ListScratch in;
  MRAG_TRY(in.bind(w.in, (size_t)nq * scan));
  MRAG_TRY(w.words.ensure((size_t)nq * 8));
  MRAG_TRY(c.out.bind(w.out, (size_t)nq * k, out_scores, out_ids, out_keys, out_is_device, true));
  c.words = (int32_t*)w.words.p;
  c.key_of = (const int32_t*)w.keys.p;
  w.host.resize((size_t)nq * 2);
  c.hw = w.host.data();
  std::vector<int64_t> todo;
  MRAG_TRY(collapse_round0(c, in, todo));
  const int64_t redone = (int64_t)todo.size();
  int64_t searches = 0;
  MRAG_TRY(collapse_redo(c, todo, &searches));
  MRAG_TRY(c.out.copy_back(c.stream));
  w.last.close(scan, redone, searches);
  return MRAG_OK;
}

int mrag_index_last_collapsed(mrag_handle h, int* out_scan_k, int64_t* out_redone_queries, int64_t* out_redo_rounds,
                              int64_t* out_max_rows_per_key, int64_t* out_distinct_keys) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  int64_t scan = 0;
  MRAG_TRY(ix->collapse.last.read("collapsed search", &scan, out_redone_queries, out_redo_rounds));
  if (out_scan_k) *out_scan_k = (int)scan;
  if (out_max_rows_per_key) *out_max_rows_per_key = ix->collapse.m;
  if (out_distinct_keys) *out_distinct_keys = ix->collapse.distinct;
  return MRAG_OK;
}

}  // extern "C"
