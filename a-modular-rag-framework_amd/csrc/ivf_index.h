// The host side of the IVF-flat index, for the ivf_*.hip sources that hold an mrag_ivf_* entry point: the IvfIndex object with
// one state struct per feature, the IvfSearch call object and its IvfChunk pipeline, and the few functions that cross files.
//   ivf_build.hip    create / destroy / centroids / train / add, row growth, the regroup; k-means and gather kernels
//   ivf_search.hip   the search pipeline (IvfSearch, IvfChunk) and its regrouping kernels; mrag_ivf_search, _last_timing
//   ivf_filter.hip   filtered search: allow-image and live-list kernels, AUTO's rule, paths E and P
//   ivf_range.hip    range search and self-join: inverse-position and exclusion kernels
//   ivf_fp8.hip      the fp8 scan copy and its search
//   ivf_scan.hip     the "score segments + select" kernels (declared in common.h)
// Host only.
#pragma once
#include "common.h"

#include <algorithm>
#include <cmath>

namespace mrag {

// filtered search (ivf_filter.hip): the allow-set over the original rows (fw.fbits), its image over the stored positions,
// the per-list allowed counts and the live-list bitset
struct IvfFilterState {
  FilterWork fw;
  DevBuf fstored;                 // uint32 bitset over the n_sorted stored positions
  DevBuf flist;                   // int counts [nlist] | int live-list count (+ 3 pad) | uint32 live bits [round256(nlist) / 32] | int caller counts [nlist]
  DevBuf flast;                   // int allowed rows, int live lists of the last path-P search (copied at its end, read on demand)
  PinnedBuf h_lallow;             // pinned staging of a host list_allowed
  Event ev_lallow;                // recorded after the last copy out of h_lallow
  int last_fpath = -1;            // MRAG_IVF_FILTER_PROBE / _EXACT of the last filtered search, -1 = none
  int64_t last_fallowed = -1;     // its allowed rows (-1: still on the device, flast word 0)
  int last_flive = -1;            // its live lists (-1: on the device, flast word 1; -2: not computed, path E)
  // the parts of flist, for an index of nlist lists
  int* counts() const { return (int*)flist.p; }
  int* nlive(int nlist) const { return (int*)flist.p + nlist; }
  uint32_t* live(int nlist) const { return (uint32_t*)flist.p + nlist + 4; }
  int* caller(int nlist) const { return (int*)flist.p + nlist + 4 + bf_round_rows(nlist) / 32; }
};

// range search and self-join (ivf_range.hip)
struct IvfRangeState {
  DevBuf inv_pos;                 // int64 [n]: original row -> stored position (built on the first use after a regroup)
  bool inv_valid = false;
  DevBuf excl;                    // int64 [nq] excluded rows of a host caller | int64 [nq] their stored positions
  DevBuf out_cnt;                 // int64 [nq] counts of a chunk with host outputs
};

// fp8 scan copy (ivf_fp8.hip): sorted8 [n_sorted][ld8] next to `sorted`, rebuilt with it by ivf_finalize
struct IvfFp8State {
  bool on = false;                // mrag_ivf_enable_fp8
  int ld8 = 0;
  DevArray<uint8_t> sorted8;
  DevBuf qbuf8, cand;             // quantised queries [nq padded][ld8]; candidates of a chunk: int64 [nq][refine] local rows
  int last_refine = -1;           // of the last mrag_ivf_search_fp8
};

struct IvfIndex : Object {
  int dim = 0, ld = 0, nlist = 0, metric = 0, dtype = MRAG_F16;
  bool has_centroids = false;
  int64_t n = 0, cap = 0, id_base = 0;
  DevArray<uint16_t> cen;         // [round256(nlist)][ld]
  DevArray<uint16_t> raw;         // [cap][ld] rows in arrival order
  DevArray<int32_t> assign;       // [cap]
  // regrouped storage (rebuilt lazily)
  bool dirty = true;
  DevArray<uint16_t> sorted;      // [n_sorted][ld]
  DevArray<int64_t> row_ids;      // [n_sorted] original row or -1
  int64_t n_sorted = 0;
  std::vector<int> list_tile_lo, list_count;
  int max_list_rows = 0;
  DevBuf qbuf, qg, lists, counts, stage_in, tmp_sc, tmp_id, out_sc, out_id, desc, ploc, gq, sums, cnts;
  DevBuf d_list_count, d_list_tile_lo, plan;   // device copies of the list layout; plan = lcount | wg_first | cursor | n_wg
  DevBuf scores, sdesc;                        // "score segments + select" regime (ivf_scan.hip): fp32 segments, dense descriptors
  Event ev_begin, ev_end;         // the device work of the last search; ev_end also closes every other call that uses the scratch buffers
  Event ev_count_begin;           // start of mrag_ivf_allowed_per_list's upload
  std::vector<Event> cev;         // per chunk of the last search: list scan begin, list scan end
  int n_chunks = 0;               // chunks of the last search (mrag_ivf_last_timing sums their scan brackets)
  DevBuf stats;                   // device accumulators of the last search: int64 rows streamed by the list scans, int64 workgroups
  bool timed = false, end_recorded = false;
  IvfFilterState filter;
  IvfRangeState range;
  IvfFp8State f8;
};

// ---- what crosses the files ----
// The dense launch (bf_launch) of nq prepared `queries` over n_rows prepared rows of `corpus`, in the index's layout and with its
// workspace.  The caller adds k and the outputs, and what only it needs: id_base, an allow-set, events, the descriptor mode's fields.
BfLaunch ivf_launch(IvfIndex* ix, const uint16_t* corpus, int64_t n_rows, const void* queries, int64_t nq, hipStream_t stream);
// a caller's rows: n rows of ix->dim elements of any supported dtype, in host or device memory
struct IvfRows { const void* p; int64_t n; int dtype, normalize, is_device; };
// rows -> prepared storage rows at dst (device), padded buffer rows zeroed by caller
int ivf_prepare(IvfIndex* ix, const IvfRows& r, uint16_t* dst, hipStream_t stream);
// regroup rows by list: stable by original row, each list padded to a multiple of 256 rows (a no-op unless rows were added)
int ivf_finalize(IvfIndex* ix, hipStream_t stream);
// dst row r = src row idx[r], one wave per row; idx < 0: a zero row (zero_fill) or left alone
int ivf_gather_rows(const uint16_t* src, const int64_t* idx, int64_t n, int ld, uint16_t* dst, int zero_fill, hipStream_t stream);
// the fp8 copy of the regrouped rows, built into `dst` (ivf_fp8.hip)
int ivf_build_sorted8(IvfIndex* ix, const uint16_t* sorted, int64_t n_sorted, DevArray<uint8_t>& dst, hipStream_t stream);
// An asynchronous call (device inputs + results) returns with the handle's scratch buffers still in use on ITS stream; a call
// on another stream first waits for that one's end event (a no-op on the same stream or after a synchronous call).
int ivf_wait_previous(IvfIndex* ix, hipStream_t stream);
// ... and the end event of this call: the handle's buffers are in use on `stream` until here
int ivf_record_end(IvfIndex* ix, hipStream_t stream);
// range.inv_pos = original row -> stored position of the current regroup (built once after every regroup; ivf_range.hip)
int ivf_ensure_inv_pos(IvfIndex* ix, hipStream_t stream);
// The score buffer of the "score segments + select" regime: MRAG_IVF_SCORES_MB, default 16 GiB, 0 = always the fused kernel.
int64_t ivf_scores_cap();
// the per-chunk events of a search in n_chunks chunks: list scan begin, list scan end
int ivf_grow_cev(IvfIndex* ix, int n_chunks);

// nq, k and nprobe of the plain, filtered and fp8 searches' kind
static inline int ivf_check_nq_k(int64_t nq, int k, int nprobe) {
  if (nq < 0 || k <= 0 || nprobe <= 0) return fail(MRAG_ERR_INVALID, "bad nq / k / nprobe");
  if (k > bf_max_k()) return fail(MRAG_ERR_UNSUPPORTED, "k = %d exceeds the fused top-k limit %d", k, bf_max_k());
  return MRAG_OK;
}

// What a search does beyond "the k best rows of the probed lists".  A mode's fields of IvfSearch are read under that mode
// alone, so these four are all the combinations there are: no filter with a floor, no fp8 scan with either.
enum IvfMode {
  IVF_PLAIN,      // the only mode with a fused form: exhaustive probing of > 256 lists, MRAG_IVF_SCORES_MB = 0, oversized segments
  IVF_FILTERED,   // path P of the filtered search: probes live lists, selects allowed stored positions; score segments without a host round trip only
  IVF_RANGE,      // lists and counts the rows scoring >= floor; score segments only
  IVF_FP8,        // scans the fp8 copies, re-scores the `refine` best local rows per query against the 16-bit rows; score segments only
};

// One call of an IVF search entry point: the plumbing mrag_ivf_search, _search_range, _self_join, _search_filtered and
// _search_fp8 share around their own argument checks and their mode's own work (bodies in ivf_search.hip).
struct IvfSearch {
  IvfIndex* ix; hipStream_t stream;
  int64_t nq; int k, nprobe;                        // (nprobe: clamped to nlist by begin)
  const void* queries; int q_dtype, normalize, queries_is_device;
  float* out_scores; int64_t* out_ids; int out_is_device;
  IvfMode mode = IVF_PLAIN;
  const uint32_t *live_bits = nullptr, *stored_bits = nullptr;   // IVF_FILTERED: bitsets over the lists / the stored positions
  float floor = 0.f;                       // IVF_RANGE
  const int64_t* excl_pos = nullptr;       //   per query the stored position of its excluded row (device, or NULL: none)
  int64_t* out_counts = nullptr;           //   [nq], in the memory space of the other outputs
  bool stored_rows = false;                //   `queries` are rows of ix->raw (storage dtype, ld apart: the self-join), copied as they are
  int refine = 0;                          // IVF_FP8
  int64_t chunk = 0;                       // queries per chunk (begin)
  const char* what() const { return mode == IVF_FP8 ? "fp8" : "range"; }   // (the modes without a fused form, as the refusals name them)

  // After the entry point's own argument checks: nprobe clamped and checked (nq == 0 stops there: the caller returns),
  // the buffers, the device, the index finalized, the batch cut into chunks of `chunk` queries, no search timed, `stream`
  // ordered behind the previous call on this handle.
  int begin();
  // (range, fp8) the refusals known before any chunk runs; a refused call has recorded nothing
  int refuse_fused() const;
  // The search's device work starts here: ev_begin, and its device accumulators (rows streamed, workgroups) start at zero.
  // record_begin = false: the filtered search, whose ev_begin filter_upload records behind the host-side packing of a host allow-set.
  int start(bool record_begin = true);
  // the chunks, one after another; ix->n_chunks is theirs once all have run
  int run_chunks();
  // (range; ivf_range.hip) start, then the excluded rows as stored positions in range.excl's second half (sized by the caller)
  // -- rows: device int64 [nq], or NULL with self_row0 >= 0 for "query i excludes row self_row0 + i", or neither: no
  // exclusion --, then the chunks
  int run_range(const int64_t* d_excl_rows, int64_t self_row0);
  // The search's device work is done: ev_end, the search is timed.  Host buffers (pageable memory) must not be touched by the
  // caller before the copies are done: the call then returns when they have landed; otherwise it is asynchronous on `stream`.
  int finish(bool host_buffer_involved);
};

// One chunk of a search (<= 2^20 queries): seven stages, run in this order on the search's stream.  The list scan (and the
// probe selection before it) runs as "score segments + select" (ivf_scan.hip) whenever the fp32 segments of the chunk fit
// the score buffer; otherwise (exhaustive probing of a big index) as the fused GEMM + top-k kernel in descriptor mode.
// DevBuf::ensure does not keep contents: every stage sizes a buffer before the chunk's first write into it.
struct IvfChunk {
  const IvfSearch& s; IvfIndex* const ix; const hipStream_t stream;
  const int64_t off, nq;                  // the chunk's queries: [off, off + nq) of the search's
  const hipEvent_t ev_scan0, ev_scan1;    // bracket the list scan (mrag_ivf_last_timing sums the chunks')
  const bool rg, f8;                      // the search's mode is IVF_RANGE / IVF_FP8
  float* d_sc = nullptr; int64_t* d_id = nullptr; int64_t* d_cnt = nullptr;   // stage_outputs: the chunk's results on the device
  // select_probes: views of ix->plan -- queries per list | first group of the list | cursor | first descriptor |
  // descriptor count, score floats (low, high) | float offset of the list's score blocks
  int *d_lcount = nullptr, *d_wg_first = nullptr, *d_cursor = nullptr, *d_dfirst = nullptr, *d_nwg = nullptr;
  long long* d_foff = nullptr;
  bool lcount_filled = false;             // select_probes: the probe selection counted the queries per list itself
  size_t npairs = 0; int64_t wg_bound = 0, desc_bound = 0;   // plan: (query, probe) pairs, bounds of the workgroup and descriptor counts
  bool use_scores = false, no_sync = false;   // plan: score-segment regime (else fused) / ... without a host round trip: the descriptor count stays on the device
  bool planned_scores = false; int n_desc = 0;   // plan: a score plan ran (and counted the chunk in ix->stats), whichever regime follows; scan descriptors of a synced one

  IvfChunk(const IvfSearch& s_, int c)
      : s(s_), ix(s_.ix), stream(s_.stream), off((int64_t)c * s_.chunk), nq(std::min(s_.chunk, s_.nq - off)),
        ev_scan0(ix->cev[2 * c]), ev_scan1(ix->cev[2 * c + 1]), rg(s_.mode == IVF_RANGE), f8(s_.mode == IVF_FP8) {}
  unsigned pgrid() const { return (unsigned)((npairs + 255) / 256); }
  // Needs nothing.  Leaves d_sc / d_id (range: d_cnt) = where the chunk's nq x k results (nq counts) are written: the
  // caller's buffers, or out_sc / out_id (range.out_cnt) for host outputs, which copy_back returns.
  int stage_outputs();
  // Needs nothing.  Leaves ix->qbuf = the chunk's queries in the storage dtype, zero padded to bf_query_rows(nq) rows; fp8:
  // their quantised image in f8.qbuf8 (zero pad rows too, the scan's pad row nq among them), f8.cand sized for the candidates.
  int prepare_queries();
  // Needs qbuf.  Leaves the probed lists of every query in ix->tmp_id ([nq][nprobe] list ids, -1: none; filtered: live lists
  // only), the plan views over ix->plan, d_lcount zeroed -- or, with lcount_filled, already holding the queries per list.
  int select_probes();
  // Needs the probes and d_lcount (counted here unless lcount_filled).  The one place that decides the regime: leaves
  // use_scores / no_sync, or the mode's refusal.  With use_scores the score plan has run and ix->scores is sized for the
  // segments; only a plan whose bound does not fit comes back to the host (12 bytes: n_desc and the size of the segments).
  int plan();
  // Needs plan() with use_scores.  Scatters the pairs into their groups, scores every (query, probed list) pair into
  // ix->scores, selects per query; leaves the results at d_sc / d_id (/ d_cnt) -- fp8: via the candidates' exact re-rank.
  int scan_scores();
  // Needs plan() without use_scores (plain search only).  Plans 256-query workgroups, scatters, reads the workgroup count
  // back (4 bytes), gathers the queries per workgroup and runs the fused kernel in descriptor mode; results at d_sc / d_id.
  int scan_fused();
  // Needs the results at d_sc / d_id (/ d_cnt).  Host outputs: their copies are queued (the search synchronises at its end).
  int copy_back() const;
  int run();
};

}  // namespace mrag
