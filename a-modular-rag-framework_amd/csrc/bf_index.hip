// The dense (brute-force) index: the BfIndex object, bf_launch -- which turns one search over prepared operands into K2 /
// K2s launches and their merges -- the DenseSearch call object and the C ABI of mrag_index_*.  The kernels live next door:
//   bf_batch.hip   K2, the fused similarity + top-k batch kernel      bf_stream.hip   K2s, the streaming kernel
//   bf_merge.hip   K4 / K4s / K4w, range count sum, wide verifier      bf_filter.hip   allow-set kernels + filtered search
//   bf_fp8.hip     fp8 quantisers + exact re-rank                      bf_kernels.h    what they share
#include "bf_kernels.h"

namespace mrag {

__global__ void fill_empty_kernel(float* sc, int64_t* ids, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { sc[i] = -INFINITY; ids[i] = -1; }
}

__global__ void unpack_rows_kernel(const uint16_t* __restrict__ src, int ld, int dim, int is_bf16, int64_t n,
                                   float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * dim) return;
  const int64_t r = i / dim;
  const int c = (int)(i % dim);
  const uint16_t b = src[r * ld + c];
  float f;
  if (is_bf16) f = __uint_as_float((uint32_t)b << 16);
  else { _Float16 h; __builtin_memcpy(&h, &b, 2); f = (float)h; }
  out[i] = f;
}

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

struct BfIndex : Object {
  int dim = 0, ld = 0, metric = 0, dtype = MRAG_F16;
  int64_t n = 0, cap_rows = 0, id_base = 0;
  uint16_t* rows = nullptr;
  DevBuf qbuf, lists, counts, stage_in, out_sc, out_id, clock;
  DevBuf rslots, out_cnt;                   // range search: per-(workgroup, query) count slots; counts for host outputs
  FilterWork fw;                            // filtered search: allow bitset, counts, compacted rows
  int last_fpath = -1;                      // path of the last filtered search (MRAG_FILTER_MASK / _COMPACT), -1 = none
  int64_t last_fallowed = -1;               // its allowed-row count; -1 = still on the device (fwork word 0, read on demand)
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool timed = false, want_clock = false;
  void* q_cleared_buf = nullptr;            // query buffer bookkeeping: rows [q_dirty_rows, q_cleared_rows) are known to be zero
  int64_t q_cleared_rows = 0, q_dirty_rows = 0;
  // fp8 scan copy (mrag_index_enable_fp8): rows8 [cap_rows][ld8], kept in step with `rows` by add / reserve
  bool fp8 = false;
  int ld8 = 0;
  uint8_t* rows8 = nullptr;
  DevBuf qbuf8, cand;                       // quantised queries [nq padded][ld8]; candidates (fp8 scores | local rows)
  DevBuf rr_q;                              // batched re-rank: its prepared queries [n_questions][ld] -- not qbuf, whose zero-padding
                                            // bookkeeping (q_cleared_*, q_dirty_rows) a 10 000-question re-rank must not disturb
  int last_refine = -1, last_regime = -1;   // of the last mrag_index_search_fp8
  // per-question allow-sets (mrag_index_search_sets): prepared queries + one zero row (not qbuf, as rr_q), the uploaded plan
  // (descriptors | question list | segment table), the scanned sets' rows, the score segments
  DevBuf sets_q, sets_plan, sets_rows, sets_S;
  int64_t last_sets[3] = {-1, -1, -1};      // of the last mrag_index_search_sets: scanned questions, routed questions, descriptors
  // grouped queries (mrag_index_search_groups): the search's [nq][k] lists (ids | scores), group_ptr on the device (uploaded
  // from grp_host, which outlives the call), the merged rows of a call with host outputs (ids | scores | which)
  DevBuf grp_in, grp_ptr, grp_out;
  std::vector<int64_t> grp_host;
  int64_t last_groups[3] = {-1, -1, -1};    // of the last mrag_index_search_groups: queries, questions, entries of the largest question
  // collapsed search (mrag_index_search_collapsed): the row keys on the device, the rows they were set for (-1 = none),
  // the largest number of rows that share a key and the distinct keys (counted on the host when the keys are set); round
  // 0's [nq][scan_k] lists and a redo round's one list (ids | scores each), the redo allow-set bitset, the per-query
  // {heads, valid} words with their host copy, the [nq][k] results (ids | scores | keys) when the caller's are on the host
  DevBuf col_keys, col_in, col_redo, col_mask, col_words, col_out;
  int64_t col_n = -1, col_m = 0, col_distinct = 0;
  std::vector<int32_t> col_host;
  int64_t last_collapsed[3] = {-1, -1, -1}; // of the last mrag_index_search_collapsed: scan_k, redone queries, redo searches
  ~BfIndex() override {
    col_keys.release(); col_in.release(); col_redo.release(); col_mask.release(); col_words.release(); col_out.release();
    grp_in.release(); grp_ptr.release(); grp_out.release();
    sets_q.release(); sets_plan.release(); sets_rows.release(); sets_S.release();
    if (rows) (void)hipFree(rows);
    if (rows8) (void)hipFree(rows8);
    qbuf8.release(); cand.release(); rr_q.release();
    qbuf.release(); lists.release(); counts.release(); stage_in.release(); out_sc.release(); out_id.release(); clock.release();
    rslots.release(); out_cnt.release();
    fw.release();   // (the destroy path synchronised the device)
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
  }
};

static size_t dtype_size(int dt) {
  switch (dt) { case MRAG_F32: return 4; case MRAG_F16: case MRAG_BF16: return 2; case MRAG_F64: return 8; default: return 0; }
}

static int grow_rows(BfIndex* ix, int64_t need_rows, hipStream_t stream) {
  if (need_rows <= ix->cap_rows) return MRAG_OK;
  int64_t cap = std::max<int64_t>(need_rows, ix->cap_rows + ix->cap_rows / 2);
  cap = round_up(std::max<int64_t>(cap, TM), TM);
  uint16_t* nr = nullptr;
  const size_t bytes = (size_t)cap * ix->ld * 2;
  hipError_t e = hipMalloc((void**)&nr, bytes);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(MRAG_ERR_OOM, "hipMalloc(%zu) for corpus rows failed: %s", bytes, hipGetErrorString(e)); }
  MRAG_HIP(hipMemsetAsync(nr, 0, bytes, stream));
  if (ix->rows && ix->n > 0) MRAG_HIP(hipMemcpyAsync(nr, ix->rows, (size_t)ix->n * ix->ld * 2, hipMemcpyDeviceToDevice, stream));
  uint8_t* nr8 = nullptr;
  if (ix->fp8) {   // the fp8 copy grows with the rows
    const size_t bytes8 = (size_t)cap * ix->ld8;
    e = hipMalloc((void**)&nr8, bytes8);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      (void)hipStreamSynchronize(stream);
      (void)hipFree(nr);
      return fail(MRAG_ERR_OOM, "hipMalloc(%zu) for the fp8 rows failed: %s", bytes8, hipGetErrorString(e));
    }
    MRAG_HIP(hipMemsetAsync(nr8, 0, bytes8, stream));
    if (ix->rows8 && ix->n > 0) MRAG_HIP(hipMemcpyAsync(nr8, ix->rows8, (size_t)ix->n * ix->ld8, hipMemcpyDeviceToDevice, stream));
  }
  if (ix->rows) { MRAG_HIP(hipStreamSynchronize(stream)); (void)hipFree(ix->rows); }
  if (ix->rows8) (void)hipFree(ix->rows8);   // (synchronised above: rows8 exists only next to rows)
  ix->rows = nr;
  ix->rows8 = nr8;
  ix->cap_rows = cap;
  return MRAG_OK;
}

// stored rows [r0, r0 + n) -> their fp8 copy
static int quant_rows_fp8(BfIndex* ix, int64_t r0, int64_t n, hipStream_t stream) {
  return launch_quant_rows_fp8(ix->rows + (size_t)r0 * ix->ld, ix->ld, ix->dtype == MRAG_BF16 ? 1 : 0, n, ix->rows8 + (size_t)r0 * ix->ld8,
                               ix->ld8, stream);
}

// CUs of the current device, read once per process
static int device_cus() {
  static int n_cu = 0;
  if (!n_cu) {
    hipDeviceProp_t pr; int dev = 0;
    n_cu = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0)
               ? pr.multiProcessorCount : 256;
  }
  return n_cu;
}

// choose the corpus split count for T query tiles
static void choose_split(int T, int n_ctiles, int* S_out, int* xcd_out) {
  // ONE wave of workgroups: S = floor(CUs / T) corpus splits per query tile (T <= 64 per launch).  Every
  // workgroup pays a first-tile bootstrap, loose thresholds in its early tiles and an end-of-split
  // compaction (~4.4 tiles' worth, measured), so few long splits beat the 2.5-5 waves of shorter ones a
  // CU-multiple grid needs -- even with T*S a little short of the CU count: 10 k queries (T = 40, S = 6,
  // 240 of 256 CUs) against S = 32: 2.43 -> 2.02 ms at 125 k rows, 4.22 -> 3.79 at 250 k, 7.60 -> 7.27 at
  // 500 k, 14.41 -> 14.32 at 1M.
  const int S = std::max(1, std::min(n_ctiles, device_cus() / std::max(1, T)));
  *S_out = S;
  // the XCD-aware block map needs a grid that splits evenly over the 8 XCDs, and pays when an XCD then holds
  // >= 2 whole query tiles (their workgroups share the corpus streams); with fewer it measured 3-6 % slower
  *xcd_out = ((T * S) % 8 == 0 && (T * S) / 8 >= 2 * S && n_ctiles >= 64) ? 1 : 0;
}


static int64_t g_wide_redone = 0;   // queries the last wide-batch search redid through the streaming kernel (tests / tools)
int64_t bf_last_wide_redone() { return g_wide_redone; }
int bf_max_k() { return KMAX; }            // fused batch kernel / IVF list scan
int bf_max_k_wide() { return KMAX_WIDE; }  // streaming kernel, 8 queries per launch
int64_t bf_round_rows(int64_t n) { return round_up(n, TM); }
// + 16 zero rows: the streaming kernel's last 8-query group reads a 16-row block
int64_t bf_query_rows(int64_t nq) { return round_up(nq, TQ) + SQ; }

// Query batches are cut so that one launch keeps its candidate lists (4.6 KB per workgroup and
// query) within a few GB: at most 64 query tiles (16 384 queries) per launch.
constexpr int MAX_QTILES_PER_LAUNCH = 64;

// the maximum dynamic LDS of a kernel, set once per process (the attribute is process-wide)
int set_max_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::vector<const void*> done;
  std::lock_guard<std::mutex> lock(mu);
  if (std::find(done.begin(), done.end(), fn) != done.end()) return MRAG_OK;
  MRAG_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  done.push_back(fn);
  return MRAG_OK;
}

// ---- bf_launch: one dense search over prepared operands = K2 or K2s launches, each followed by its merge ----
// the fields every K2 launch of `a` shares
static BfParams k2_params(const BfLaunch& a) {
  BfParams p = {};
  p.corpus = a.corpus;
  p.ld = a.ld;
  p.ksteps = a.ld / BK;
  p.k = a.k;
  p.clock = a.clock;
  p.allow = a.wg_desc ? nullptr : a.allow;
  p.floor = a.floor;
  return p;
}

// the merge's view of one K2 / K2s launch: its lists and counts over T query tiles x S splits (descriptor mode: the
// probes of a.pair_loc), the nq queries it served and where their results go
static MergeParams merge_params(const BfLaunch& a, const void* list, const void* counts, int T, int S, int64_t nq,
                                float* out_scores, int64_t* out_ids) {
  const bool desc = a.wg_desc != nullptr;
  MergeParams mp = {};
  mp.list = (const uint2*)list; mp.counts = (const int*)counts;
  mp.T = T; mp.S = S; mp.k = a.k; mp.nq = nq; mp.id_base = a.id_base;
  mp.pair_loc = desc ? (const int2*)a.pair_loc : nullptr; mp.nprobe = desc ? a.nprobe : 0; mp.row_ids = desc ? a.row_ids : nullptr;
  mp.out_scores = out_scores; mp.out_ids = out_ids;
  return mp;
}

// ---- descriptor mode (IVF list scan): one launch, one merge ----
static int launch_desc(const BfLaunch& a) {
  const size_t grid = (size_t)a.n_wg;
  MRAG_TRY(a.lists->ensure(grid * TQ * QCAP * 8));
  MRAG_TRY(a.counts->ensure(grid * TQ * sizeof(int)));
  BfParams p = k2_params(a);
  p.queries = a.queries;
  p.n_rows = 0; p.n_ctiles = 0; p.nq = 0; p.T = (int)grid; p.S = 1; p.xcd_map = 0;
  p.wg_desc = a.wg_desc;
  p.list = (uint2*)a.lists->p;
  p.counts = (int*)a.counts->p;
  MRAG_TRY(launch_k2(a.dtype, true, false, false, grid, a.stream, p));
  if (a.ev_k2_end) MRAG_HIP(hipEventRecord(a.ev_k2_end, a.stream));
  if (a.nq) MRAG_TRY(launch_merge(merge_params(a, p.list, p.counts, 0, 0, a.nq, a.out_scores, a.out_ids), nullptr, nullptr, a.stream));
  return MRAG_OK;
}

// ---- online regime: HBM-bound streaming kernel (K2s), one workgroup per CU-sized corpus split ----
// k <= 32: up to 16 queries per launch; 32 < k <= 256: 8 per launch with 512-entry lists; any number of queries as
// consecutive launches (exact, one HBM pass each), each followed by its merge.
static int stream_regions(int n_ctiles) { return std::max(1, std::min(n_ctiles, 256)); }

struct StreamCall {
  const uint16_t* queries;   // prepared rows; the last group reads a whole 16-row block (zero rows behind the queries)
  int64_t nq;
  float* out_scores;         // [nq][k]
  int64_t* out_ids;
  bool size_workspaces;      // grow lists / counts / range slots here; false: the caller sized them and keeps data in them
                             // (ensure() drops contents)
  bool sum_counts;           // range search: sum each group's count slots into a.out_counts
  bool record_end;           // record a.ev_k2_end behind the last K2s launch
};

static int launch_stream(const BfLaunch& a, const StreamCall& c) {
  const bool wi = a.k > 32;
  const int grp = wi ? 8 : SQ;
  const int n_ctiles = (int)((a.n_rows + TM - 1) / TM);
  const int S = stream_regions(n_ctiles);
  if (c.size_workspaces) {
    MRAG_TRY(a.lists->ensure((size_t)S * TQ * QCAP * 8));
    MRAG_TRY(a.counts->ensure(((size_t)S * TQ + 16) * sizeof(int)));   // + the K4s fallback flags of one query group
    if (a.range) MRAG_TRY(a.rslots->ensure((size_t)S * TQ * sizeof(int)));
  }
  // wide lists or more than one batch of regions: K4s + K4w, flags in the 16 ints behind the per-region counts
  int* flags = (wi || S > 64) ? (int*)a.counts->p + (size_t)S * TQ : nullptr;
  for (int64_t g0 = 0; g0 < c.nq; g0 += grp) {
    const int64_t gq = std::min<int64_t>(grp, c.nq - g0);
    StreamParams sp;
    sp.corpus = a.corpus; sp.queries = c.queries + (size_t)g0 * a.ld; sp.ld = a.ld; sp.ksteps = a.ld / BK;
    sp.n_rows = (int)a.n_rows; sp.n_ctiles = n_ctiles; sp.nq = (int)gq; sp.S = S; sp.k = a.k;
    sp.list = (uint2*)a.lists->p; sp.counts = (int*)a.counts->p;
    sp.allow = a.allow;
    sp.floor = a.floor;
    sp.rcounts = a.range ? (int*)a.rslots->p : nullptr;
    MRAG_TRY(launch_k2s(a.dtype, a.allow != nullptr, a.range, wi, a.stream, sp));
    if (a.range && c.sum_counts)
      MRAG_TRY(launch_range_sum((const int*)a.rslots->p, S, gq, a.out_counts ? a.out_counts + g0 : nullptr, a.stream));
    if (c.record_end && g0 + grp >= c.nq && a.ev_k2_end) MRAG_HIP(hipEventRecord(a.ev_k2_end, a.stream));
    MRAG_TRY(launch_merge(merge_params(a, sp.list, sp.counts, 1, S, gq, c.out_scores + (size_t)g0 * a.k, c.out_ids + (size_t)g0 * a.k),
                          flags, nullptr, a.stream));
  }
  return MRAG_OK;
}

// ---- batch regimes: the batch kernel over (query tile, corpus split) grids of at most T_max query tiles, each launch
// followed by its merge.
// Wide batch (k > 64): the batch kernel at k' = 64 over S >= 4k/64 splits + merge to k + verification
// (bf_wide_verify_kernel), the flagged queries redone by the streaming kernel.  10 000 queries at the reference's pool of
// 200 were 1 250 streaming launches (one HBM pass each, ~0.5 s over 1M rows); now ceil(T / 16..19) batch-kernel launches.

// The wide-batch regime's workspaces, sized once for every launch of the search (ensure() drops contents).  a.counts holds,
// behind the per-region counts (+ the 16 K4s flags of a streaming group of the redo), four more regions:
struct WideWork {
  size_t grid_max = 0;   // workgroups of the largest launch: T * S <= CUs for the batch kernel, the stream regime's regions for the redo
  size_t flags = 0;      // int index: the K4s flags of one batch launch [T_max * 256]
  size_t need = 0;       // int index: 1 where a query must be redone [nq]
  size_t stage = 0;      // byte offset: 16 staged query rows (8 redone queries + zero rows)
  size_t results = 0;    // byte offset: the redo's 8 x k scores, then its 8 x k ids
  size_t bytes = 0;      // all of it
  WideWork() {}
  WideWork(const BfLaunch& a, int n_ctiles, int T_max) {
    grid_max = (size_t)std::max(device_cus(), stream_regions(n_ctiles));
    flags = grid_max * TQ + 16;
    need = flags + (size_t)T_max * TQ;
    stage = (size_t)round_up((int64_t)((need + (size_t)a.nq) * sizeof(int)), 256);
    results = stage + (size_t)16 * a.ld * 2;
    bytes = results + (size_t)8 * a.k * 12 + 256;
  }
  int* flags_in(const DevBuf* b) const { return (int*)b->p + flags; }
  int* need_in(const DevBuf* b) const { return (int*)b->p + need; }
  uint16_t* stage_in(const DevBuf* b) const { return (uint16_t*)((char*)b->p + stage); }
  float* scores_in(const DevBuf* b) const { return (float*)((char*)b->p + results); }
  int64_t* ids_in(const DevBuf* b, int k) const { return (int64_t*)((char*)b->p + results + (size_t)8 * k * 4); }
};

// the queries the verifier flagged, exactly, eight per streaming launch (their rows staged contiguously)
static int redo_flagged(const BfLaunch& a, const WideWork& ww) {
  hipStream_t stream = a.stream;
  std::vector<int> h_need((size_t)a.nq);
  MRAG_HIP(hipMemcpyAsync(h_need.data(), ww.need_in(a.counts), (size_t)a.nq * sizeof(int), hipMemcpyDeviceToHost, stream));
  MRAG_HIP(hipStreamSynchronize(stream));
  std::vector<int64_t> redo;
  for (int64_t q = 0; q < a.nq; ++q) if (h_need[(size_t)q]) redo.push_back(q);
  g_wide_redone = (int64_t)redo.size();
  uint16_t* stage = ww.stage_in(a.counts);
  float* r_sc = ww.scores_in(a.counts);
  int64_t* r_id = ww.ids_in(a.counts, a.k);
  for (size_t g0 = 0; g0 < redo.size(); g0 += 8) {
    const size_t m = std::min<size_t>(8, redo.size() - g0);
    MRAG_HIP(hipMemsetAsync(stage, 0, (size_t)16 * a.ld * 2, stream));
    for (size_t i = 0; i < m; ++i)
      MRAG_HIP(hipMemcpyAsync(stage + i * a.ld, a.queries + (size_t)redo[g0 + i] * a.ld, (size_t)a.ld * 2, hipMemcpyDeviceToDevice, stream));
    // (the redo only fixes lists: its queries were counted by the batch pass, and the workspaces hold this search's data)
    MRAG_TRY(launch_stream(a, StreamCall{stage, (int64_t)m, r_sc, r_id, false, false, false}));
    for (size_t i = 0; i < m; ++i) {
      MRAG_HIP(hipMemcpyAsync(a.out_scores + (size_t)redo[g0 + i] * a.k, r_sc + i * a.k, (size_t)a.k * 4, hipMemcpyDeviceToDevice, stream));
      MRAG_HIP(hipMemcpyAsync(a.out_ids + (size_t)redo[g0 + i] * a.k, r_id + i * a.k, (size_t)a.k * 8, hipMemcpyDeviceToDevice, stream));
    }
  }
  return MRAG_OK;
}

static int launch_batch(const BfLaunch& a, bool wide) {
  const int n_ctiles = (int)((a.n_rows + TM - 1) / TM);
  const int T_all = (int)((a.nq + TQ - 1) / TQ);
  int T_max = MAX_QTILES_PER_LAUNCH;
  WideWork ww;
  if (wide) {
    const int S_min = std::max(4, (4 * a.k + KMAX - 1) / KMAX);
    T_max = std::max(1, std::min(MAX_QTILES_PER_LAUNCH, device_cus() / S_min));
    ww = WideWork(a, n_ctiles, T_max);
    MRAG_TRY(a.lists->ensure(ww.grid_max * TQ * QCAP * 8));
    MRAG_TRY(a.counts->ensure(ww.bytes));
    if (a.range) MRAG_TRY(a.rslots->ensure(ww.grid_max * TQ * sizeof(int)));
  }
  BfParams p = k2_params(a);
  p.n_rows = (int)a.n_rows; p.n_ctiles = n_ctiles;
  p.k = wide ? KMAX : a.k;
  for (int t0 = 0; t0 < T_all; t0 += T_max) {
    const int T = std::min(T_max, T_all - t0);
    const int64_t q0 = (int64_t)t0 * TQ;
    const int64_t nq = std::min<int64_t>(a.nq - q0, (int64_t)T * TQ);
    int S, xcd;
    choose_split(T, n_ctiles, &S, &xcd);
    const size_t grid = (size_t)T * S;
    if (!wide) {
      MRAG_TRY(a.lists->ensure(grid * TQ * QCAP * 8));
      MRAG_TRY(a.counts->ensure(grid * TQ * sizeof(int)));
      if (a.range) MRAG_TRY(a.rslots->ensure(grid * TQ * sizeof(int)));
    }
    p.queries = a.queries + (size_t)q0 * a.ld;
    p.nq = (int)nq;
    p.T = T; p.S = S; p.xcd_map = xcd;
    p.list = (uint2*)a.lists->p;
    p.counts = (int*)a.counts->p;
    p.rcounts = a.range ? (int*)a.rslots->p : nullptr;
    MRAG_TRY(launch_k2(a.dtype, false, a.allow != nullptr, a.range, grid, a.stream, p));
    if (t0 + T_max >= T_all && a.ev_k2_end) MRAG_HIP(hipEventRecord(a.ev_k2_end, a.stream));
    if (a.range) MRAG_TRY(launch_range_sum((const int*)a.rslots->p, S, nq, a.out_counts ? a.out_counts + q0 : nullptr, a.stream));
    const MergeParams mp = merge_params(a, p.list, p.counts, T, S, nq, a.out_scores + (size_t)q0 * a.k, a.out_ids + (size_t)q0 * a.k);
    if (wide) MRAG_TRY(launch_merge(mp, ww.flags_in(a.counts), ww.need_in(a.counts) + q0, a.stream));
    else MRAG_TRY(launch_merge(mp, nullptr, nullptr, a.stream));
  }
  return wide ? redo_flagged(a, ww) : MRAG_OK;
}

int bf_launch(const BfLaunch& a) {
  if (a.k <= 0 || a.k > (a.wg_desc ? KMAX : KMAX_WIDE)) return fail(MRAG_ERR_UNSUPPORTED, "k = %d outside 1..%d", a.k, a.wg_desc ? KMAX : KMAX_WIDE);
  if (a.range && (a.wg_desc || !a.rslots)) return fail(MRAG_ERR_UNSUPPORTED, "range search serves the dense mode only");
  if (a.ev_k2_begin) MRAG_HIP(hipEventRecord(a.ev_k2_begin, a.stream));
  if (a.wg_desc) return launch_desc(a);
  const BfRegime regime = bf_regime(a.nq, a.k, a.n_rows, a.force_stream);
  g_wide_redone = 0;
  if (regime == BF_STREAM) return launch_stream(a, StreamCall{a.queries, a.nq, a.out_scores, a.out_ids, true, true, true});
  return launch_batch(a, regime == BF_WIDE_BATCH);
}

// every slot of sc / ids (n each) -> (-inf, -1)
int launch_fill_empty(float* sc, int64_t* ids, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(fill_empty_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sc, ids, n);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

// nq and k of the exact dense searches
static int check_nq_k(int64_t nq, int k) {
  if (nq < 0) return fail(MRAG_ERR_INVALID, "nq < 0");
  if (k <= 0) return fail(MRAG_ERR_INVALID, "k must be positive");
  if (k > KMAX_WIDE) return fail(MRAG_ERR_UNSUPPORTED, "k = %d exceeds the top-k limit %d (see mrag_index_max_k)", k, KMAX_WIDE);
  return MRAG_OK;
}

// One call of a dense search entry point: the plumbing mrag_index_search, _filtered and _fp8 share around their own work.
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
    if (!queries || !out_scores || !out_ids) return fail(MRAG_ERR_INVALID, "NULL buffer");
    if (allow_null) return fail(MRAG_ERR_INVALID, "allow is NULL");
    esz = dtype_size(q_dtype);
    if (!esz) return fail(MRAG_ERR_INVALID, "unknown query dtype %d", q_dtype);
    if (nq > (1ll << 26)) return fail(MRAG_ERR_UNSUPPORTED, "nq too large for one call; batch the queries");
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

// mrag_index_search_filtered (floor NULL) and mrag_index_search_range (floor = &min_score).  The filtered search needs an
// allow-set over a non-empty index; the range search takes NULL for "every row" and then runs the plain search, and
// records its filter path only when it had an allow-set.
static int search_allowed(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device,
                          int k, const float* floor, const void* allow, int64_t allow_rows, int allow_format, int allow_is_device,
                          int path, float* out_scores, int64_t* out_ids, int64_t* out_counts, int out_is_device, void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  MRAG_TRY(check_nq_k(nq, k));
  if (floor && !std::isfinite(*floor)) return fail(MRAG_ERR_INVALID, "min_score must be finite, got %g", (double)*floor);
  const bool filtered = allow || !floor;
  if (filtered) MRAG_TRY(check_allow_args(allow_rows, ix->n, allow_format, path, "filter"));
  if (nq == 0) return MRAG_OK;
  if (floor && !out_counts) return fail(MRAG_ERR_INVALID, "NULL buffer");
  DenseSearch s{ix, nq, k, out_scores, out_ids, out_is_device, (hipStream_t)stream_, out_counts};
  MRAG_TRY(s.begin(queries, q_dtype, !allow && !floor && ix->n > 0, filtered ? &ix->last_fpath : nullptr));
  const int64_t n = ix->n;
  int64_t m = n;                      // rows searched (allow-set: allowed rows when known on the host, else -1)
  int chosen = -1;
  if (filtered) {
    // the whole-search figure (ev[0] .. ev[3]) covers the device work: with a host allow-set it starts after the
    // host-side packing and count, at the bitset's upload
    MRAG_TRY(filter_upload(ix->fw, allow, n, allow_format, allow_is_device, path != MRAG_FILTER_MASK, &m, ix->ev[0], s.stream));
    chosen = path != MRAG_FILTER_AUTO ? path : filter_choose_path(nq, k, n, m, ix->ld);
  } else {
    MRAG_HIP(hipEventRecord(ix->ev[0], s.stream));
  }
  if (n == 0 || m == 0) {
    MRAG_TRY(s.fill_empty());         // nothing to search: every slot (-inf, -1), every count 0
  } else {
    MRAG_TRY(s.prep_queries(queries, q_dtype, normalize, queries_is_device));
    BfLaunch a;
    MRAG_TRY(s.exact_launch(&a));
    if (floor) {
      a.range = true;
      a.floor = *floor;
      a.out_counts = s.d_cnt;
      a.rslots = &ix->rslots;
    }
    if (filtered) MRAG_TRY(filter_search(ix->fw, a, chosen, m, s.stream));
    else MRAG_TRY(bf_launch(a));
  }
  MRAG_TRY(s.end());
  if (filtered) {
    ix->last_fpath = chosen;
    ix->last_fallowed = m;
  }
  return s.copy_back();
}

// ---- mrag_index_search_sets: the host plan of the scan route ----
// Score scratch of one scan + select pair.  A call whose segments need more is cut into chunks of whole questions.
// Nobody has measured this limit: 1 GiB holds 32 768 segments of the largest scanned set and keeps the scratch a small
// part of the device's memory; a smaller scratch that stays in L2 between the scan and the select may well be faster.
constexpr int64_t SETS_SCRATCH_FLOATS = (int64_t)1 << 28;

struct SetsChunk {
  int64_t q0, nq;          // sorted scan questions [q0, q0 + nq)
  int64_t d0, nd;          // its descriptors
};
struct SetsPlan {
  std::vector<int> qlist;               // scan questions, sorted by set (stable): original question index
  std::vector<int> desc;                // SETS_DESC_WORDS ints per descriptor, chunk after chunk
  std::vector<int> pinfo;               // int4 per sorted scan question: segment offset (low, high), rows, first position
  std::vector<SetsChunk> chunks;
  std::vector<int64_t> rows;            // the scanned sets' rows when some set is routed (else the caller's set_rows serve)
  std::vector<int64_t> routed;          // sets above SETS_SCAN_MAX_ROWS that some question uses
  std::vector<int64_t> order, qstart;   // all questions sorted by set (stable); set s owns order[qstart[s] .. qstart[s+1])
  int64_t n_rows = 0, max_floats = 0;   // positions the scan may read; floats of the largest chunk
};

// (arguments validated by the caller)
static int sets_plan(int64_t nq, int64_t n_sets, const int64_t* set_ptr, const int64_t* set_rows, const int32_t* set_of, SetsPlan& p) {
  p.qstart.assign((size_t)n_sets + 1, 0);
  for (int64_t q = 0; q < nq; ++q) ++p.qstart[(size_t)set_of[q] + 1];
  for (int64_t s = 0; s < n_sets; ++s) p.qstart[(size_t)s + 1] += p.qstart[(size_t)s];
  p.order.resize((size_t)nq);
  {
    std::vector<int64_t> at(p.qstart.begin(), p.qstart.end() - 1);
    for (int64_t q = 0; q < nq; ++q) p.order[(size_t)at[(size_t)set_of[q]]++] = q;
  }
  for (int64_t s = 0; s < n_sets; ++s)
    if (p.qstart[(size_t)s + 1] > p.qstart[(size_t)s] && set_ptr[s + 1] - set_ptr[s] > SETS_SCAN_MAX_ROWS) p.routed.push_back(s);
  const bool compact = !p.routed.empty();
  int64_t floats = 0;                     // of the open chunk
  SetsChunk c{0, 0, 0, 0};
  const auto close = [&]() {
    if (c.nq) { p.chunks.push_back(c); p.max_floats = std::max(p.max_floats, floats); }
    c = SetsChunk{c.q0 + c.nq, 0, c.d0 + c.nd, 0};
    floats = 0;
  };
  for (int64_t s = 0; s < n_sets; ++s) {
    const int64_t m = set_ptr[s + 1] - set_ptr[s];
    int64_t g0 = p.qstart[(size_t)s];
    const int64_t g1 = p.qstart[(size_t)s + 1];
    if (g1 == g0 || m > SETS_SCAN_MAX_ROWS) continue;
    int64_t pos = set_ptr[s];
    if (compact) {
      pos = (int64_t)p.rows.size();
      p.rows.insert(p.rows.end(), set_rows + set_ptr[s], set_rows + set_ptr[s + 1]);
    }
    if (pos + m > 0x7FFFFFFFll) return fail(MRAG_ERR_UNSUPPORTED, "set %lld ends at position %lld of set_rows: one call scans at most 2^31 - 1 positions", (long long)s, (long long)(pos + m));
    p.n_rows = std::max(p.n_rows, pos + m);
    const int64_t pitch = ivfs_pitch(m);
    while (g0 < g1) {
      // the questions of the set that still fit the open chunk (an empty set's questions take no scratch)
      int64_t fit = pitch ? (SETS_SCRATCH_FLOATS - floats) / pitch : g1 - g0;
      if (fit <= 0) { close(); continue; }
      fit = std::min(fit, g1 - g0);
      for (int64_t r0 = 0; r0 < m; r0 += SETS_CHUNK)
        for (int64_t q0 = 0; q0 < fit; q0 += SETS_CHUNK) {
          const int64_t soff = floats + q0 * pitch;
          const int d[SETS_DESC_WORDS] = {(int)(c.q0 + c.nq + q0), (int)std::min<int64_t>(SETS_CHUNK, fit - q0), (int)(pos + r0),
                                          (int)std::min<int64_t>(SETS_CHUNK, m - r0), (int)r0, (int)(uint32_t)(soff & 0xFFFFFFFFll),
                                          (int)(soff >> 32), (int)pitch};
          p.desc.insert(p.desc.end(), d, d + SETS_DESC_WORDS);
          ++c.nd;
        }
      for (int64_t g = 0; g < fit; ++g) {
        const int64_t soff = floats + g * pitch;
        const int pi[4] = {(int)(uint32_t)(soff & 0xFFFFFFFFll), (int)(soff >> 32), (int)m, (int)pos};
        p.pinfo.insert(p.pinfo.end(), pi, pi + 4);
        p.qlist.push_back((int)p.order[(size_t)(g0 + g)]);
      }
      floats += fit * pitch;
      c.nq += fit;
      g0 += fit;
    }
  }
  close();
  return MRAG_OK;
}

}  // namespace mrag

using namespace mrag;

extern "C" {

int mrag_index_create(int dim, int metric, int storage_dtype, int device, mrag_handle* out) {
  if (!out) return fail(MRAG_ERR_INVALID, "out is NULL");
  if (dim <= 0 || dim > 8192) return fail(MRAG_ERR_INVALID, "dim %d out of range (1..8192)", dim);
  if (metric != MRAG_METRIC_COSINE && metric != MRAG_METRIC_IP) return fail(MRAG_ERR_INVALID, "unknown metric %d", metric);
  if (storage_dtype != MRAG_F16 && storage_dtype != MRAG_BF16) return fail(MRAG_ERR_INVALID, "storage dtype must be fp16 or bf16");
  MRAG_TRY(use_device(device));
  BfIndex* ix = new BfIndex();
  ix->kind = KIND_BF_INDEX;
  ix->device = device;
  ix->dim = dim;
  ix->ld = (int)round_up(dim, BK);
  ix->ld8 = (int)round_up(dim, FP8_K);
  ix->metric = metric;
  ix->dtype = storage_dtype;
  for (auto& e : ix->ev) {
    if (hipEventCreate(&e) != hipSuccess) { delete ix; return fail(MRAG_ERR_HIP, "hipEventCreate failed"); }
  }
  *out = register_object(ix);
  return MRAG_OK;
}

int mrag_index_destroy(mrag_handle h) {
  Object* o = take(h, KIND_BF_INDEX);
  if (!o) return MRAG_ERR_INVALID;
  (void)hipSetDevice(o->device);
  (void)hipDeviceSynchronize();
  delete o;
  return MRAG_OK;
}

int mrag_index_reserve(mrag_handle h, int64_t n_rows) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (n_rows < 0 || n_rows > 0x7FFFFF00ll) return fail(MRAG_ERR_INVALID, "n_rows out of range");
  MRAG_TRY(use_device(ix->device));
  MRAG_TRY(grow_rows(ix, n_rows, nullptr));
  // the zero fill / copy above ran on the null stream; callers add and search on their own (non-blocking)
  // streams, which are not ordered behind it: finish it here (reserve is a one-off)
  MRAG_HIP(hipStreamSynchronize(nullptr));
  return MRAG_OK;
}

int mrag_index_add(mrag_handle h, const void* rows, int64_t n, int src_dtype, int normalize, int rows_is_device,
                   void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (n < 0) return fail(MRAG_ERR_INVALID, "n < 0");
  if (n == 0) return MRAG_OK;
  if (!rows) return fail(MRAG_ERR_INVALID, "rows is NULL");
  const size_t esz = dtype_size(src_dtype);
  if (!esz) return fail(MRAG_ERR_INVALID, "unknown source dtype %d", src_dtype);
  if (ix->n + n > 0x7FFFFF00ll) return fail(MRAG_ERR_UNSUPPORTED, "more than 2^31 rows per index; shard the corpus");
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  MRAG_TRY(grow_rows(ix, ix->n + n, stream));
  const void* src = rows;
  if (!rows_is_device) {
    const size_t bytes = (size_t)n * ix->dim * esz;
    MRAG_TRY(ix->stage_in.ensure(bytes));
    MRAG_HIP(hipMemcpyAsync(ix->stage_in.p, rows, bytes, hipMemcpyHostToDevice, stream));
    src = ix->stage_in.p;
  }
  MRAG_TRY(launch_prep_rows(src, src_dtype, n, ix->dim, ix->rows + (size_t)ix->n * ix->ld, ix->ld, ix->dtype,
                            normalize, stream));
  if (ix->fp8) MRAG_TRY(quant_rows_fp8(ix, ix->n, n, stream));
  if (!rows_is_device) MRAG_HIP(hipStreamSynchronize(stream));
  ix->n += n;
  return MRAG_OK;
}

int mrag_index_size(mrag_handle h, int64_t* out_rows) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (!out_rows) return fail(MRAG_ERR_INVALID, "out_rows is NULL");
  *out_rows = ix->n;
  return MRAG_OK;
}

int mrag_index_dim(mrag_handle h, int* out_dim) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (!out_dim) return fail(MRAG_ERR_INVALID, "out_dim is NULL");
  *out_dim = ix->dim;
  return MRAG_OK;
}

int mrag_index_set_id_base(mrag_handle h, int64_t id_base) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  ix->id_base = id_base;
  return MRAG_OK;
}

int mrag_index_max_k(int64_t nq, int* out_k) {
  if (!out_k) return fail(MRAG_ERR_INVALID, "out_k is NULL");
  (void)nq;   // every batch size is served up to the wide limit (k > 64: streaming kernel, or the wide-batch path of bf_launch)
  *out_k = KMAX_WIDE;
  return MRAG_OK;
}

int mrag_index_last_wide_redone(int64_t* out_queries) {
  if (!out_queries) return fail(MRAG_ERR_INVALID, "out_queries is NULL");
  *out_queries = bf_last_wide_redone();
  return MRAG_OK;
}

int mrag_index_get_rows(mrag_handle h, int64_t row0, int64_t n, float* out, int out_is_device, void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (row0 < 0 || n < 0 || row0 + n > ix->n) return fail(MRAG_ERR_INVALID, "row range [%lld,%lld) outside [0,%lld)", (long long)row0, (long long)(row0 + n), (long long)ix->n);
  if (n == 0) return MRAG_OK;
  if (!out) return fail(MRAG_ERR_INVALID, "out is NULL");
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  float* dst = out;
  const size_t bytes = (size_t)n * ix->dim * 4;
  if (!out_is_device) { MRAG_TRY(ix->stage_in.ensure(bytes)); dst = (float*)ix->stage_in.p; }
  const int64_t tot = n * ix->dim;
  hipLaunchKernelGGL(unpack_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream,
                     ix->rows + (size_t)row0 * ix->ld, ix->ld, ix->dim, ix->dtype == MRAG_BF16 ? 1 : 0, n, dst);
  MRAG_HIP(hipGetLastError());
  if (!out_is_device) {
    MRAG_HIP(hipMemcpyAsync(out, dst, bytes, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipStreamSynchronize(stream));
  }
  return MRAG_OK;
}

int mrag_index_search(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize,
                      int queries_is_device, int k, float* out_scores, int64_t* out_ids, int out_is_device,
                      void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  MRAG_TRY(check_nq_k(nq, k));
  if (nq == 0) return MRAG_OK;
  DenseSearch s{ix, nq, k, out_scores, out_ids, out_is_device, (hipStream_t)stream_};
  MRAG_TRY(s.begin(queries, q_dtype));
  MRAG_HIP(hipEventRecord(ix->ev[0], s.stream));
  if (ix->n == 0) {
    MRAG_TRY(s.fill_empty());
  } else {
    MRAG_TRY(s.prep_queries(queries, q_dtype, normalize, queries_is_device));
    BfLaunch a;
    MRAG_TRY(s.exact_launch(&a));
    MRAG_TRY(bf_launch(a));
  }
  MRAG_TRY(s.end());
  return s.copy_back();
}

int mrag_index_search_filtered(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize,
                               int queries_is_device, int k, const void* allow, int64_t allow_rows, int allow_format,
                               int allow_is_device, int path, float* out_scores, int64_t* out_ids, int out_is_device,
                               void* stream_) {
  return search_allowed(h, queries, nq, q_dtype, normalize, queries_is_device, k, nullptr, allow, allow_rows, allow_format,
                        allow_is_device, path, out_scores, out_ids, nullptr, out_is_device, stream_);
}

int mrag_index_search_range(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device,
                            int k, float min_score, const void* allow, int64_t allow_rows, int allow_format, int allow_is_device,
                            int filter_path, float* out_scores, int64_t* out_ids, int64_t* out_counts, int out_is_device,
                            void* stream_) {
  return search_allowed(h, queries, nq, q_dtype, normalize, queries_is_device, k, &min_score, allow, allow_rows, allow_format,
                        allow_is_device, filter_path, out_scores, out_ids, out_counts, out_is_device, stream_);
}

int mrag_index_last_filter(mrag_handle h, int* out_path, int64_t* out_allowed) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (ix->last_fpath < 0) return fail(MRAG_ERR_INVALID, "no completed filtered search on this index");
  if (ix->last_fallowed < 0) {        // device allow-set, path M: the count is still on the device
    MRAG_TRY(use_device(ix->device));
    MRAG_HIP(hipEventSynchronize(ix->ev[3]));
    int hm = 0;
    MRAG_HIP(hipMemcpy(&hm, ix->fw.fwork.p, sizeof(int), hipMemcpyDeviceToHost));
    ix->last_fallowed = hm;
  }
  if (out_path) *out_path = ix->last_fpath;
  if (out_allowed) *out_allowed = ix->last_fallowed;
  return MRAG_OK;
}

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
  MRAG_HIP(hipMemcpyAsync(st, query, (size_t)ix->dim * esz, hipMemcpyHostToDevice, stream));
  MRAG_HIP(hipMemcpyAsync(st + qb, row_ids, (size_t)n * 8, hipMemcpyHostToDevice, stream));
  MRAG_TRY(launch_prep_rows(st, q_dtype, 1, ix->dim, ix->qbuf.p, ix->ld, ix->dtype,
                            normalize && ix->metric == MRAG_METRIC_COSINE, stream));
  if (ix->qbuf.p == ix->q_cleared_buf) ix->q_dirty_rows = std::max<int64_t>(ix->q_dirty_rows, 1);   // row 0 of the query buffer was written
  hipLaunchKernelGGL(score_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, ix->rows, (const uint16_t*)ix->qbuf.p,
                     ix->ld, ix->dtype == MRAG_BF16 ? 1 : 0, (const int64_t*)(st + qb), n, ix->n, (float*)(st + qb + ib));
  MRAG_HIP(hipGetLastError());
  MRAG_HIP(hipMemcpyAsync(out_scores, st + qb + ib, ob, hipMemcpyDeviceToHost, stream));
  MRAG_HIP(hipStreamSynchronize(stream));
  return MRAG_OK;
}

int mrag_index_score_rows_batch(mrag_handle h, const void* queries, int q_dtype, int normalize, int64_t n_questions,
                                const int64_t* row_ptr, const int64_t* row_ids, float* out_scores, void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (n_questions < 0) return fail(MRAG_ERR_INVALID, "n_questions < 0");
  if (n_questions == 0) return MRAG_OK;
  if (!row_ptr) return fail(MRAG_ERR_INVALID, "row_ptr is NULL");
  if (row_ptr[0] != 0) return fail(MRAG_ERR_INVALID, "row_ptr[0] = %lld, not 0 (question 0)", (long long)row_ptr[0]);
  for (int64_t g = 0; g < n_questions; ++g)
    if (row_ptr[g + 1] < row_ptr[g])
      return fail(MRAG_ERR_INVALID, "row_ptr decreases at question %lld (%lld -> %lld)", (long long)g, (long long)row_ptr[g],
                  (long long)row_ptr[g + 1]);
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
  // the uploads read `desc` and the caller's buffers asynchronously: whatever fails below, the stream is synchronised
  // before they go out of scope
  const auto enqueue = [&]() -> int {
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
  };
  const int status = enqueue();
  if (status != MRAG_OK) {
    (void)hipStreamSynchronize(stream);
    return status;
  }
  MRAG_HIP(hipStreamSynchronize(stream));
  return MRAG_OK;
}

int mrag_index_search_sets(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int k, int64_t n_sets,
                           const int64_t* set_ptr, const int64_t* set_rows, const int32_t* set_of, float* out_scores,
                           int64_t* out_ids, void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  MRAG_TRY(check_nq_k(nq, k));
  if (n_sets < 0) return fail(MRAG_ERR_INVALID, "n_sets < 0");
  if (nq == 0) return MRAG_OK;
  if (!queries || !set_ptr || !set_of || !out_scores || !out_ids) return fail(MRAG_ERR_INVALID, "NULL buffer");
  const size_t esz = dtype_size(q_dtype);
  if (!esz) return fail(MRAG_ERR_INVALID, "unknown query dtype %d", q_dtype);
  if (nq > (1ll << 26)) return fail(MRAG_ERR_UNSUPPORTED, "nq too large for one call; batch the questions");
  if (n_sets > 0 && set_ptr[0] != 0) return fail(MRAG_ERR_INVALID, "set_ptr[0] = %lld, not 0 (set 0)", (long long)set_ptr[0]);
  for (int64_t s = 0; s < n_sets; ++s)
    if (set_ptr[s + 1] < set_ptr[s])
      return fail(MRAG_ERR_INVALID, "set_ptr decreases at set %lld (%lld -> %lld)", (long long)s, (long long)set_ptr[s], (long long)set_ptr[s + 1]);
  if (n_sets > 0 && set_ptr[n_sets] > 0 && !set_rows) return fail(MRAG_ERR_INVALID, "NULL buffer (set_rows)");
  for (int64_t s = 0; s < n_sets; ++s)
    for (int64_t i = set_ptr[s]; i < set_ptr[s + 1]; ++i) {
      const int64_t r = set_rows[i];
      if (r < 0 || r >= ix->n)
        return fail(MRAG_ERR_INVALID, "set %lld: row %lld outside [0, %lld)", (long long)s, (long long)r, (long long)ix->n);
      if (i > set_ptr[s] && r <= set_rows[i - 1])
        return fail(MRAG_ERR_INVALID, "set %lld: rows are not strictly ascending (%lld after %lld)", (long long)s, (long long)r,
                    (long long)set_rows[i - 1]);
    }
  for (int64_t q = 0; q < nq; ++q)
    if (set_of[q] < 0 || set_of[q] >= n_sets)
      return fail(MRAG_ERR_INVALID, "question %lld: set %d outside [0, %lld)", (long long)q, (int)set_of[q], (long long)n_sets);
  SetsPlan p;
  MRAG_TRY(sets_plan(nq, n_sets, set_ptr, set_rows, set_of, p));
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  ix->last_sets[0] = -1;
  const int ld = ix->ld;
  const size_t row_bytes = (size_t)ix->dim * esz;

  // ---- scan route: every question of a set of <= SETS_SCAN_MAX_ROWS rows
  const int64_t n_scan = (int64_t)p.qlist.size();
  if (n_scan) {
    ix->timed = false;                                       // (the events of the last plain search bracket none of this)
    const int64_t* rows_src = p.routed.empty() ? set_rows : p.rows.data();
    // plan: [descriptors | question list | segment table], one upload
    const size_t db = (size_t)round_up((int64_t)(p.desc.size() * 4), 256), lb = (size_t)round_up(n_scan * 4, 256), pb = (size_t)n_scan * 16;
    std::vector<char> plan(db + lb + pb);
    if (!p.desc.empty()) memcpy(plan.data(), p.desc.data(), p.desc.size() * 4);
    memcpy(plan.data() + db, p.qlist.data(), (size_t)n_scan * 4);
    memcpy(plan.data() + db + lb, p.pinfo.data(), pb);
    std::vector<float> h_sc((size_t)n_scan * k);
    std::vector<int64_t> h_id((size_t)n_scan * k);
    MRAG_TRY(ix->stage_in.ensure((size_t)nq * row_bytes));
    MRAG_TRY(ix->sets_q.ensure((size_t)(nq + 1) * ld * 2));
    MRAG_TRY(ix->sets_plan.ensure(plan.size()));
    MRAG_TRY(ix->sets_rows.ensure((size_t)std::max<int64_t>(p.n_rows, 1) * 8));
    MRAG_TRY(ix->sets_S.ensure((size_t)std::max<int64_t>(p.max_floats, 32) * 4));
    MRAG_TRY(ix->out_sc.ensure((size_t)n_scan * k * 4));
    MRAG_TRY(ix->out_id.ensure((size_t)n_scan * k * 8));
    uint16_t* d_q = (uint16_t*)ix->sets_q.p;
    const uint16_t* d_zero = d_q + (size_t)nq * ld;
    const char* d_plan = (const char*)ix->sets_plan.p;
    float* d_sc = (float*)ix->out_sc.p;
    int64_t* d_id = (int64_t*)ix->out_id.p;
    // the uploads read `plan`, `p` and the caller's buffers asynchronously: whatever fails below, the stream is synchronised
    // before they go out of scope
    const auto enqueue = [&]() -> int {
      MRAG_HIP(hipMemcpyAsync(ix->stage_in.p, queries, (size_t)nq * row_bytes, hipMemcpyHostToDevice, stream));
      MRAG_HIP(hipMemcpyAsync(ix->sets_plan.p, plan.data(), plan.size(), hipMemcpyHostToDevice, stream));
      if (p.n_rows) MRAG_HIP(hipMemcpyAsync(ix->sets_rows.p, rows_src, (size_t)p.n_rows * 8, hipMemcpyHostToDevice, stream));
      MRAG_HIP(hipMemsetAsync((void*)d_zero, 0, (size_t)ld * 2, stream));
      MRAG_TRY(launch_prep_rows(ix->stage_in.p, q_dtype, nq, ix->dim, d_q, ld, ix->dtype, normalize && ix->metric == MRAG_METRIC_COSINE, stream));
      for (const SetsChunk& c : p.chunks) {
        MRAG_TRY(launch_sets_scan(ix->rows, d_q, d_zero, ld, ix->dtype, (const int*)d_plan + (size_t)c.d0 * SETS_DESC_WORDS, (int)c.nd,
                                  (const int64_t*)ix->sets_rows.p, (const int*)(d_plan + db), (float*)ix->sets_S.p, stream));
        MRAG_TRY(ivfs_select_lists((const float*)ix->sets_S.p, d_plan + db + lb + (size_t)c.q0 * 16, 1, c.nq, k, (const int64_t*)ix->sets_rows.p,
                                   ix->id_base, d_sc + (size_t)c.q0 * k, d_id + (size_t)c.q0 * k, stream));
      }
      MRAG_HIP(hipMemcpyAsync(h_sc.data(), d_sc, h_sc.size() * 4, hipMemcpyDeviceToHost, stream));
      MRAG_HIP(hipMemcpyAsync(h_id.data(), d_id, h_id.size() * 8, hipMemcpyDeviceToHost, stream));
      return MRAG_OK;
    };
    const int status = enqueue();
    if (status != MRAG_OK) {
      (void)hipStreamSynchronize(stream);
      return status;
    }
    MRAG_HIP(hipStreamSynchronize(stream));
    for (int64_t g = 0; g < n_scan; ++g) {
      const size_t q = (size_t)p.qlist[(size_t)g];
      memcpy(out_scores + q * k, h_sc.data() + (size_t)g * k, (size_t)k * 4);
      memcpy(out_ids + q * k, h_id.data() + (size_t)g * k, (size_t)k * 8);
    }
  }

  // ---- routed: a larger set is ONE filtered search over all of its questions (in groups where the batch limits k)
  int64_t n_routed = 0;
  for (const int64_t s : p.routed) {
    const int64_t g0 = p.qstart[(size_t)s], n_q = p.qstart[(size_t)s + 1] - g0;
    std::vector<uint32_t> bits((size_t)((ix->n + 31) / 32), 0u);
    for (int64_t i = set_ptr[s]; i < set_ptr[s + 1]; ++i) bits[(size_t)(set_rows[i] >> 5)] |= 1u << (set_rows[i] & 31);
    int64_t group = n_q;
    for (;;) {
      int kmax = 0;
      MRAG_TRY(mrag_index_max_k(group, &kmax));
      if (kmax >= k || group == 1) break;
      group = (group + 1) / 2;
    }
    std::vector<char> hq((size_t)group * row_bytes);
    std::vector<float> h_sc((size_t)group * k);
    std::vector<int64_t> h_id((size_t)group * k);
    for (int64_t j0 = 0; j0 < n_q; j0 += group) {
      const int64_t n_g = std::min(group, n_q - j0);
      for (int64_t j = 0; j < n_g; ++j)
        memcpy(hq.data() + (size_t)j * row_bytes, (const char*)queries + (size_t)p.order[(size_t)(g0 + j0 + j)] * row_bytes, row_bytes);
      MRAG_TRY(search_allowed(h, hq.data(), n_g, q_dtype, normalize, 0, k, nullptr, bits.data(), ix->n, MRAG_ALLOW_BITS32, 0,
                              MRAG_FILTER_AUTO, h_sc.data(), h_id.data(), nullptr, 0, stream_));
      for (int64_t j = 0; j < n_g; ++j) {
        const size_t q = (size_t)p.order[(size_t)(g0 + j0 + j)];
        memcpy(out_scores + q * k, h_sc.data() + (size_t)j * k, (size_t)k * 4);
        memcpy(out_ids + q * k, h_id.data() + (size_t)j * k, (size_t)k * 8);
      }
    }
    n_routed += n_q;
  }
  ix->last_sets[0] = n_scan;
  ix->last_sets[1] = n_routed;
  ix->last_sets[2] = (int64_t)(p.desc.size() / SETS_DESC_WORDS);
  return MRAG_OK;
}

int mrag_index_last_sets(mrag_handle h, int64_t* out_scanned_questions, int64_t* out_routed_questions, int64_t* out_descriptors) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (ix->last_sets[0] < 0) return fail(MRAG_ERR_INVALID, "no completed search over per-question sets on this index");
  if (out_scanned_questions) *out_scanned_questions = ix->last_sets[0];
  if (out_routed_questions) *out_routed_questions = ix->last_sets[1];
  if (out_descriptors) *out_descriptors = ix->last_sets[2];
  return MRAG_OK;
}

int mrag_index_search_groups(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device,
                             int k, int64_t n_groups, const int64_t* group_ptr, const void* allow, int64_t allow_rows,
                             int allow_format, float* out_scores, int64_t* out_ids, int32_t* out_which, int out_is_device,
                             void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  MRAG_TRY(check_nq_k(nq, k));
  if (n_groups < 0) return fail(MRAG_ERR_INVALID, "n_groups < 0");
  if (n_groups == 0 && nq == 0) return MRAG_OK;
  if (!group_ptr || !out_scores || !out_ids || (nq > 0 && !queries)) return fail(MRAG_ERR_INVALID, "NULL buffer");
  if (!dtype_size(q_dtype)) return fail(MRAG_ERR_INVALID, "unknown query dtype %d", q_dtype);
  if (group_ptr[0] != 0) return fail(MRAG_ERR_INVALID, "group_ptr[0] = %lld, not 0 (question 0)", (long long)group_ptr[0]);
  for (int64_t g = 0; g < n_groups; ++g)
    if (group_ptr[g + 1] < group_ptr[g])
      return fail(MRAG_ERR_INVALID, "group_ptr decreases at question %lld (%lld -> %lld)", (long long)g, (long long)group_ptr[g],
                  (long long)group_ptr[g + 1]);
  if (group_ptr[n_groups] != nq)
    return fail(MRAG_ERR_INVALID, "group_ptr ends at %lld behind question %lld, not at nq = %lld", (long long)group_ptr[n_groups],
                (long long)n_groups - 1, (long long)nq);
  int64_t q_max = 0;
  for (int64_t g = 0; g < n_groups; ++g) {
    const int64_t q = group_ptr[g + 1] - group_ptr[g];
    if (q * k > GROUPS_MAX_ENTRIES)
      return fail(MRAG_ERR_UNSUPPORTED, "question %lld has %lld queries x k = %d = %lld entries, more than %d", (long long)g, (long long)q,
                  k, (long long)(q * k), GROUPS_MAX_ENTRIES);
    q_max = std::max(q_max, q);
  }
  if (allow) MRAG_TRY(check_allow_args(allow_rows, ix->n, allow_format, MRAG_FILTER_AUTO, "filter"));
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  ix->last_groups[0] = -1;

  // ---- one search of all nq queries into index-owned scratch (mrag_index_max_k is 256 for every nq: never cut)
  const size_t n_in = (size_t)nq * k, n_out = (size_t)n_groups * k;
  MRAG_TRY(ix->grp_in.ensure(std::max<size_t>(n_in, 1) * 12));
  int64_t* s_id = (int64_t*)ix->grp_in.p;
  float* s_sc = (float*)(s_id + n_in);
  if (nq > 0) {
    if (allow)
      MRAG_TRY(search_allowed(h, queries, nq, q_dtype, normalize, queries_is_device, k, nullptr, allow, allow_rows, allow_format, 0,
                              MRAG_FILTER_AUTO, s_sc, s_id, nullptr, 1, stream_));
    else
      MRAG_TRY(mrag_index_search(h, queries, nq, q_dtype, normalize, queries_is_device, k, s_sc, s_id, 1, stream_));
  }

  // ---- one merge launch, straight into device outputs
  ix->grp_host.assign(group_ptr, group_ptr + n_groups + 1);
  MRAG_TRY(ix->grp_ptr.ensure((size_t)(n_groups + 1) * 8));
  float* d_sc = out_scores;
  int64_t* d_id = out_ids;
  int32_t* d_wh = out_which;
  if (!out_is_device) {
    MRAG_TRY(ix->grp_out.ensure(n_out * 16));
    d_id = (int64_t*)ix->grp_out.p;
    d_sc = (float*)(d_id + n_out);
    d_wh = out_which ? (int32_t*)(d_sc + n_out) : nullptr;
  }
  MRAG_HIP(hipMemcpyAsync(ix->grp_ptr.p, ix->grp_host.data(), (size_t)(n_groups + 1) * 8, hipMemcpyHostToDevice, stream));
  MRAG_TRY(launch_groups_merge(s_sc, s_id, (const int64_t*)ix->grp_ptr.p, n_groups, k, (int)(q_max * k), d_sc, d_id, d_wh, stream));
  if (!out_is_device) {
    MRAG_HIP(hipMemcpyAsync(out_scores, d_sc, n_out * 4, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipMemcpyAsync(out_ids, d_id, n_out * 8, hipMemcpyDeviceToHost, stream));
    if (out_which) MRAG_HIP(hipMemcpyAsync(out_which, d_wh, n_out * 4, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipStreamSynchronize(stream));
  }
  ix->last_groups[0] = nq;
  ix->last_groups[1] = n_groups;
  ix->last_groups[2] = q_max * k;
  return MRAG_OK;
}

int mrag_index_last_groups(mrag_handle h, int64_t* out_queries, int64_t* out_groups, int64_t* out_max_entries) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (ix->last_groups[0] < 0) return fail(MRAG_ERR_INVALID, "no completed search over grouped queries on this index");
  if (out_queries) *out_queries = ix->last_groups[0];
  if (out_groups) *out_groups = ix->last_groups[1];
  if (out_max_entries) *out_max_entries = ix->last_groups[2];
  return MRAG_OK;
}

int mrag_index_set_row_keys(mrag_handle h, const int32_t* keys, int64_t n, int keys_is_device) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (n < 0) return fail(MRAG_ERR_INVALID, "n < 0");
  if (n == 0 && !keys) { ix->col_n = -1; ix->col_m = 0; ix->col_distinct = 0; return MRAG_OK; }
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
  MRAG_TRY(ix->col_keys.ensure(std::max<size_t>((size_t)n, 1) * 4));
  if (n > 0) MRAG_HIP(hipMemcpy(ix->col_keys.p, hk.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  std::sort(hk.begin(), hk.end());
  int64_t distinct = 0, longest = 0, run = 0;
  for (int64_t r = 0; r < n; ++r) {
    if (r == 0 || hk[(size_t)r] != hk[(size_t)r - 1]) { ++distinct; run = 0; }
    longest = std::max(longest, ++run);
  }
  ix->col_n = n;
  ix->col_m = longest;
  ix->col_distinct = distinct;
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

int mrag_index_search_collapsed(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device,
                                int k, int scan_k, float* out_scores, int64_t* out_ids, int32_t* out_keys, int out_is_device,
                                void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  MRAG_TRY(check_nq_k(nq, k));
  if (scan_k != 0 && (scan_k < k || scan_k > KMAX_WIDE))
    return fail(MRAG_ERR_INVALID, "scan_k = %d lies outside [k, %d] = [%d, %d] (0 picks the default)", scan_k, KMAX_WIDE, k, KMAX_WIDE);
  const int64_t n = ix->n;
  if (ix->col_n < 0 && n > 0) return fail(MRAG_ERR_INVALID, "no row keys set on this index (mrag_index_set_row_keys)");
  if (ix->col_n >= 0 && ix->col_n != n)
    return fail(MRAG_ERR_INVALID, "row keys were set for %lld rows, the index holds %lld: set them again", (long long)ix->col_n, (long long)n);
  if (nq == 0) return MRAG_OK;
  if (!queries || !out_scores || !out_ids) return fail(MRAG_ERR_INVALID, "NULL buffer");
  const size_t esz = dtype_size(q_dtype);
  if (!esz) return fail(MRAG_ERR_INVALID, "unknown query dtype %d", q_dtype);
  if (nq > (1ll << 26)) return fail(MRAG_ERR_UNSUPPORTED, "nq too large for one call; batch the queries");
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  ix->last_collapsed[0] = -1;
  const int scan = scan_k ? scan_k : collapse_default_scan_k(k, ix->col_m, n);

  const size_t n_in = (size_t)nq * scan, n_out = (size_t)nq * k;
  MRAG_TRY(ix->col_in.ensure(n_in * 12));
  MRAG_TRY(ix->col_words.ensure((size_t)nq * 8));
  MRAG_TRY(ix->col_out.ensure(n_out * 16));
  int64_t* s_id = (int64_t*)ix->col_in.p;
  float* s_sc = (float*)(s_id + n_in);
  int32_t* words = (int32_t*)ix->col_words.p;
  const int32_t* key_of = (const int32_t*)ix->col_keys.p;       // (NULL only over an empty index: no list entry is valid)
  // the found keys feed the redo masks, so they are kept also when the caller does not ask for them
  int64_t* d_id = out_is_device ? out_ids : (int64_t*)ix->col_out.p;
  float* d_sc = out_is_device ? out_scores : (float*)((int64_t*)ix->col_out.p + n_out);
  int32_t* d_key = out_is_device && out_keys ? out_keys : (int32_t*)((char*)ix->col_out.p + n_out * 12);

  // ---- round 0: one search of all queries at depth `scan`, one collapse launch, the words read back
  MRAG_TRY(mrag_index_search(h, queries, nq, q_dtype, normalize, queries_is_device, scan, s_sc, s_id, 1, stream_));
  MRAG_TRY(launch_collapse_heads(s_sc, s_id, nq, scan, key_of, n, ix->id_base, k, 0, 0, words, d_sc, d_id, d_key, stream));
  ix->col_host.resize((size_t)nq * 2);
  int32_t* hw = ix->col_host.data();
  MRAG_HIP(hipMemcpyAsync(hw, words, (size_t)nq * 8, hipMemcpyDeviceToHost, stream));
  MRAG_HIP(hipStreamSynchronize(stream));
  // incomplete: fewer than k keys, and the list was full (rows may stand behind it)
  std::vector<int64_t> todo;
  for (int64_t q = 0; q < nq; ++q)
    if (hw[2 * q] < k && hw[2 * q + 1] >= scan) todo.push_back(q);
  const int64_t redone = (int64_t)todo.size();
  int64_t searches = 0;

  // ---- redo rounds: each incomplete query alone over the rows whose key it has not found; every round adds a key
  if (redone) {
    MRAG_TRY(ix->col_redo.ensure((size_t)scan * 12));
    MRAG_TRY(ix->col_mask.ensure((size_t)collapse_mask_words(n) * 4));
  }
  int64_t* r_id = (int64_t*)ix->col_redo.p;
  float* r_sc = (float*)(r_id + scan);
  while (!todo.empty()) {
    for (const int64_t q : todo) {
      MRAG_TRY(launch_collapse_mask(key_of, n, d_key + (size_t)q * k, words + 2 * q, k, (uint32_t*)ix->col_mask.p, stream));
      MRAG_TRY(search_allowed(h, (const char*)queries + (size_t)q * ix->dim * esz, 1, q_dtype, normalize, queries_is_device, scan,
                              nullptr, ix->col_mask.p, n, MRAG_ALLOW_BITS32, 1, MRAG_FILTER_AUTO, r_sc, r_id, nullptr, 1, stream_));
      MRAG_TRY(launch_collapse_heads(r_sc, r_id, 1, scan, key_of, n, ix->id_base, k, q, 1, words, d_sc, d_id, d_key, stream));
      ++searches;
    }
    MRAG_HIP(hipMemcpyAsync(hw, words, (size_t)nq * 8, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipStreamSynchronize(stream));
    std::vector<int64_t> next;
    for (const int64_t q : todo)
      if (hw[2 * q] < k && hw[2 * q + 1] >= scan) next.push_back(q);
    todo.swap(next);
  }

  if (!out_is_device) {
    MRAG_HIP(hipMemcpyAsync(out_scores, d_sc, n_out * 4, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipMemcpyAsync(out_ids, d_id, n_out * 8, hipMemcpyDeviceToHost, stream));
    if (out_keys) MRAG_HIP(hipMemcpyAsync(out_keys, d_key, n_out * 4, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipStreamSynchronize(stream));
  }
  ix->last_collapsed[0] = scan;
  ix->last_collapsed[1] = redone;
  ix->last_collapsed[2] = searches;
  return MRAG_OK;
}

int mrag_index_last_collapsed(mrag_handle h, int* out_scan_k, int64_t* out_redone_queries, int64_t* out_redo_rounds,
                              int64_t* out_max_rows_per_key, int64_t* out_distinct_keys) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (ix->last_collapsed[0] < 0) return fail(MRAG_ERR_INVALID, "no completed collapsed search on this index");
  if (out_scan_k) *out_scan_k = (int)ix->last_collapsed[0];
  if (out_redone_queries) *out_redone_queries = ix->last_collapsed[1];
  if (out_redo_rounds) *out_redo_rounds = ix->last_collapsed[2];
  if (out_max_rows_per_key) *out_max_rows_per_key = ix->col_m;
  if (out_distinct_keys) *out_distinct_keys = ix->col_distinct;
  return MRAG_OK;
}

int mrag_index_measure_clock(mrag_handle h, int enable) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  ix->want_clock = enable != 0;
  return MRAG_OK;
}

int mrag_index_last_clock(mrag_handle h, float* out_ghz) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (!out_ghz) return fail(MRAG_ERR_INVALID, "out_ghz is NULL");
  if (!ix->timed || !ix->want_clock || !ix->clock.p) return fail(MRAG_ERR_INVALID, "no search with the clock reading enabled");
  MRAG_TRY(use_device(ix->device));
  MRAG_HIP(hipEventSynchronize(ix->ev[3]));
  long long w[4] = {0, 0, 0, 0};
  MRAG_HIP(hipMemcpy(w, ix->clock.p, sizeof(w), hipMemcpyDeviceToHost));
  const double dc = (double)(w[2] - w[0]), dr = (double)(w[3] - w[1]);
  if (dr <= 0 || dc <= 0) return fail(MRAG_ERR_UNSUPPORTED, "the last search did not run the batch kernel (no clock stamps)");
  *out_ghz = (float)(dc / dr * 0.1);   // s_memrealtime ticks at 100 MHz
  return MRAG_OK;
}

int mrag_index_enable_fp8(mrag_handle h) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (ix->metric != MRAG_METRIC_COSINE) return fail(MRAG_ERR_INVALID, "the fp8 scan copy serves cosine indexes only");
  if (ix->fp8) return MRAG_OK;
  MRAG_TRY(use_device(ix->device));
  if (ix->cap_rows > 0) {
    // rows already stored (adds on any stream): settle them, build the copy on the null stream, finish it here (a one-off)
    MRAG_HIP(hipDeviceSynchronize());
    const size_t bytes8 = (size_t)ix->cap_rows * ix->ld8;
    hipError_t e = hipMalloc((void**)&ix->rows8, bytes8);
    if (e != hipSuccess) { (void)hipGetLastError(); ix->rows8 = nullptr; return fail(MRAG_ERR_OOM, "hipMalloc(%zu) for the fp8 rows failed: %s", bytes8, hipGetErrorString(e)); }
    MRAG_HIP(hipMemsetAsync(ix->rows8, 0, bytes8, nullptr));
    MRAG_TRY(quant_rows_fp8(ix, 0, ix->n, nullptr));
    MRAG_HIP(hipStreamSynchronize(nullptr));
  }
  ix->fp8 = true;
  return MRAG_OK;
}

int mrag_index_get_rows_fp8(mrag_handle h, int64_t row0, int64_t n, uint8_t* out, int out_is_device, void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (!ix->fp8) return fail(MRAG_ERR_INVALID, "no fp8 scan copy (mrag_index_enable_fp8)");
  if (row0 < 0 || n < 0 || row0 + n > ix->n) return fail(MRAG_ERR_INVALID, "row range [%lld,%lld) outside [0,%lld)", (long long)row0, (long long)(row0 + n), (long long)ix->n);
  if (n == 0) return MRAG_OK;
  if (!out) return fail(MRAG_ERR_INVALID, "out is NULL");
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  MRAG_HIP(hipMemcpy2DAsync(out, (size_t)ix->dim, ix->rows8 + (size_t)row0 * ix->ld8, (size_t)ix->ld8, (size_t)ix->dim, (size_t)n,
                            out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
  if (!out_is_device) MRAG_HIP(hipStreamSynchronize(stream));
  return MRAG_OK;
}

int mrag_index_fp8_default_refine(int k, int* out) {
  if (!out) return fail(MRAG_ERR_INVALID, "out is NULL");
  if (k < 1 || k > FP8_MAX_REFINE) return fail(MRAG_ERR_INVALID, "fp8 search serves 1 <= k <= %d, got %d", FP8_MAX_REFINE, k);
  *out = std::min(FP8_MAX_REFINE, std::max(40, 4 * k));
  return MRAG_OK;
}

int mrag_index_search_fp8(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device,
                          int k, int refine, float* out_scores, int64_t* out_ids, int out_is_device, void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (!ix->fp8) return fail(MRAG_ERR_INVALID, "no fp8 scan copy on this index (mrag_index_enable_fp8)");
  if (nq < 0) return fail(MRAG_ERR_INVALID, "nq < 0");
  if (k < 1 || k > FP8_MAX_REFINE) return fail(MRAG_ERR_INVALID, "fp8 search serves 1 <= k <= %d, got %d", FP8_MAX_REFINE, k);
  if (refine == 0) MRAG_TRY(mrag_index_fp8_default_refine(k, &refine));
  if (refine < k || refine > FP8_MAX_REFINE) return fail(MRAG_ERR_INVALID, "refine = %d outside k..%d (k = %d)", refine, FP8_MAX_REFINE, k);
  if (nq == 0) return MRAG_OK;
  DenseSearch s{ix, nq, k, out_scores, out_ids, out_is_device, (hipStream_t)stream_};
  MRAG_TRY(s.begin(queries, q_dtype, false, &ix->last_refine));
  const bool stream_regime = nq <= SQ;   // as the plain search: up to 16 queries take the streaming kernel
  MRAG_HIP(hipEventRecord(ix->ev[0], s.stream));
  if (ix->n == 0) {
    MRAG_TRY(s.fill_empty());
  } else {
    MRAG_TRY(s.prep_queries(queries, q_dtype, normalize, queries_is_device));
    const int64_t nq_pad = bf_query_rows(nq);   // prep_queries keeps qbuf rows [nq, nq_pad) zero: so are their fp8 rows
    MRAG_TRY(ix->qbuf8.ensure((size_t)nq_pad * ix->ld8));
    MRAG_TRY(launch_quant_queries_fp8((const uint16_t*)ix->qbuf.p, ix->ld, ix->dtype == MRAG_BF16 ? 1 : 0, nq_pad, (uint8_t*)ix->qbuf8.p,
                                      ix->ld8, s.stream));
    MRAG_TRY(ix->cand.ensure((size_t)nq * refine * 12));
    int64_t* c_id = (int64_t*)ix->cand.p;
    float* c_sc = (float*)(c_id + (size_t)nq * refine);
    BfLaunch a = s.launch(refine, c_sc, c_id);
    a.corpus = (const uint16_t*)ix->rows8;
    a.queries = (const uint16_t*)ix->qbuf8.p;
    a.ld = ix->ld8 / 2;              // in 16-bit units: the kernels address rows of ld8 bytes
    a.dtype = MRAG_DT_FP8;
    a.id_base = 0;                   // local rows for the re-rank
    a.force_stream = stream_regime;
    MRAG_TRY(bf_launch(a));
    MRAG_TRY(launch_fp8_rerank((const uint16_t*)ix->rows, (const uint16_t*)ix->qbuf.p, ix->ld, ix->dtype == MRAG_BF16 ? 1 : 0,
                               (const int64_t*)c_id, nq, refine, k, ix->id_base, s.d_sc, s.d_id, s.stream));
  }
  MRAG_TRY(s.end());
  ix->last_refine = refine;
  ix->last_regime = stream_regime ? MRAG_FP8_STREAM : MRAG_FP8_BATCH;
  return s.copy_back();
}

int mrag_index_last_fp8(mrag_handle h, int* out_refine, int* out_regime) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (ix->last_refine < 0) return fail(MRAG_ERR_INVALID, "no completed fp8 search on this index");
  if (out_refine) *out_refine = ix->last_refine;
  if (out_regime) *out_regime = ix->last_regime;
  return MRAG_OK;
}

int mrag_index_last_timing(mrag_handle h, float* out_gemm_ms, float* out_total_ms) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (!ix->timed) return fail(MRAG_ERR_INVALID, "no completed search to time");
  MRAG_TRY(use_device(ix->device));
  MRAG_HIP(hipEventSynchronize(ix->ev[3]));
  float g = 0.f, t = 0.f;
  MRAG_HIP(hipEventElapsedTime(&g, ix->ev[1], ix->ev[2]));
  MRAG_HIP(hipEventElapsedTime(&t, ix->ev[0], ix->ev[3]));
  if (out_gemm_ms) *out_gemm_ms = g;
  if (out_total_ms) *out_total_ms = t;
  return MRAG_OK;
}

}  // extern "C"
