// The dense (brute-force) index: bf_launch -- which turns one search over prepared operands into K2 / K2s launches and their
// merges -- row growth, and the C ABI of mrag_index_* for create / destroy / add / get, the plain, filtered, range and fp8
// searches and the timing calls.  The BfIndex object and the DenseSearch call object are in bf_index.h.  Next door:
//   bf_batch.hip   K2, the fused similarity + top-k batch kernel      bf_stream.hip   K2s, the streaming kernel
//   bf_merge.hip   K4 / K4s / K4w, range count sum, wide verifier      bf_filter.hip   allow-set kernels + filtered search
//   bf_fp8.hip     fp8 quantisers + exact re-rank                      bf_kernels.h    what the kernels share
// and the composite searches, each with its kernels and its entry points:
//   bf_rerank_batch.hip   mrag_index_score_rows, _score_rows_batch     bf_filter_batch.hip   mrag_index_search_sets
//   bf_groups.hip         mrag_index_search_groups                     bf_collapse.hip       mrag_index_search_collapsed
#include "bf_index.h"

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

static int grow_rows(BfIndex* ix, int64_t need_rows, hipStream_t stream) {
  if (need_rows <= ix->cap_rows) return MRAG_OK;
  int64_t cap = std::max<int64_t>(need_rows, ix->cap_rows + ix->cap_rows / 2);
  cap = round_up(std::max<int64_t>(cap, TM), TM);
  // the new owners, filled and settled, then moved into place: a failure part-way leaves the index as it was
  DevArray<uint16_t> nr;
  DevArray<uint8_t> nr8;
  const size_t bytes = (size_t)cap * ix->ld * 2;
  MRAG_TRY(nr.alloc(bytes, "corpus rows"));
  MRAG_HIP(hipMemsetAsync(nr, 0, bytes, stream));
  if (ix->rows && ix->n > 0) MRAG_HIP(hipMemcpyAsync(nr, ix->rows, (size_t)ix->n * ix->ld * 2, hipMemcpyDeviceToDevice, stream));
  if (ix->fp8) {   // the fp8 copy grows with the rows
    const size_t bytes8 = (size_t)cap * ix->ld8;
    MRAG_TRY(nr8.alloc(bytes8, "the fp8 rows"));
    MRAG_HIP(hipMemsetAsync(nr8, 0, bytes8, stream));
    if (ix->rows8 && ix->n > 0) MRAG_HIP(hipMemcpyAsync(nr8, ix->rows8, (size_t)ix->n * ix->ld8, hipMemcpyDeviceToDevice, stream));
  }
  if (ix->rows) MRAG_HIP(hipStreamSynchronize(stream));   // (the old rows are freed behind the copies out of them)
  ix->rows.swap(nr);
  ix->rows8.swap(nr8);
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

// the plain search (declared in bf_index.h)
int bf_search(BfIndex* ix, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device, int k,
              float* out_scores, int64_t* out_ids, int out_is_device, hipStream_t stream) {
  MRAG_TRY(check_nq_k(nq, k));
  if (nq == 0) return MRAG_OK;
  DenseSearch s{ix, nq, k, out_scores, out_ids, out_is_device, stream};
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

// the filtered and the range search (declared in bf_index.h)
int search_allowed(BfIndex* ix, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device, int k,
                   const float* floor, const void* allow, int64_t allow_rows, int allow_format, int allow_is_device, int path,
                   float* out_scores, int64_t* out_ids, int64_t* out_counts, int out_is_device, hipStream_t stream) {
  MRAG_TRY(check_nq_k(nq, k));
  if (floor && !std::isfinite(*floor)) return fail(MRAG_ERR_INVALID, "min_score must be finite, got %g", (double)*floor);
  const bool filtered = allow || !floor;
  if (filtered) MRAG_TRY(check_allow_args(allow_rows, ix->n, allow_format, path, "filter"));
  if (nq == 0) return MRAG_OK;
  if (floor && !out_counts) return fail(MRAG_ERR_INVALID, "NULL buffer");
  DenseSearch s{ix, nq, k, out_scores, out_ids, out_is_device, stream, out_counts};
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
  int st = MRAG_OK;
  for (auto& e : ix->ev)
    if (st == MRAG_OK) st = e.create(true);
  if (st != MRAG_OK) { delete ix; return st; }
  *out = register_object(ix);
  return MRAG_OK;
}

int mrag_index_destroy(mrag_handle h) { return destroy_object(h, KIND_BF_INDEX); }

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
  return bf_search(ix, queries, nq, q_dtype, normalize, queries_is_device, k, out_scores, out_ids, out_is_device, (hipStream_t)stream_);
}

int mrag_index_search_filtered(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize,
                               int queries_is_device, int k, const void* allow, int64_t allow_rows, int allow_format,
                               int allow_is_device, int path, float* out_scores, int64_t* out_ids, int out_is_device,
                               void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  return search_allowed(ix, queries, nq, q_dtype, normalize, queries_is_device, k, nullptr, allow, allow_rows, allow_format,
                        allow_is_device, path, out_scores, out_ids, nullptr, out_is_device, (hipStream_t)stream_);
}

int mrag_index_search_range(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device,
                            int k, float min_score, const void* allow, int64_t allow_rows, int allow_format, int allow_is_device,
                            int filter_path, float* out_scores, int64_t* out_ids, int64_t* out_counts, int out_is_device,
                            void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  return search_allowed(ix, queries, nq, q_dtype, normalize, queries_is_device, k, &min_score, allow, allow_rows, allow_format,
                        allow_is_device, filter_path, out_scores, out_ids, out_counts, out_is_device, (hipStream_t)stream_);
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
    MRAG_TRY(ix->rows8.alloc(bytes8, "the fp8 rows"));
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
    a.corpus = (const uint16_t*)ix->rows8.p;
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
