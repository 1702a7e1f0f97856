// IVF-flat over the same fused similarity + top-k kernels (BASELINE.json config 5; the reference
// has no IVF index -- PARITY UNPINNED by the reference, checked against this library's own brute
// force and the oracle's ivf_search on identical centroids / assignments).
//
//   train    spherical k-means on the device: assignment = the dense kernel with the CENTROIDS as
//            corpus and the rows as queries (k = 1, ties to the lowest list id), update = float
//            atomics into [nlist][dim] sums, re-normalised and rounded to the storage dtype.
//   add      rows are normalised/rounded once, kept in arrival order, assigned as above.
//   search   1) probe lists: dense kernel over the centroids, k = nprobe
//            2) rows regrouped by list (stable by original row, each list padded to 256 rows);
//               every list becomes workgroups of <= 256 of the queries that probe it: the list's
//               rows are streamed from HBM ONCE for all of them (HBM-bound: bytes = list rows x
//               ld x 2 per workgroup), scored on MFMA and filtered by the same in-kernel top-k
//            3) per query the nprobe candidate sets are merged by (score desc, original row asc)
//   The (list -> queries) regrouping of step 2 runs on the device (count / plan / scatter kernels below);
//   only the workgroup count comes back to the host.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace mrag {

struct IvfIndex : Object {
  int dim = 0, ld = 0, nlist = 0, metric = 0, dtype = MRAG_F16;
  bool has_centroids = false;
  int64_t n = 0, cap = 0, id_base = 0;
  uint16_t* cen = nullptr;        // [round256(nlist)][ld]
  uint16_t* raw = nullptr;        // [cap][ld] rows in arrival order
  int32_t* assign = nullptr;      // [cap]
  // regrouped storage (rebuilt lazily)
  bool dirty = true;
  uint16_t* sorted = nullptr;     // [n_sorted][ld]
  int64_t* row_ids = nullptr;     // [n_sorted] original row or -1
  int64_t n_sorted = 0;
  std::vector<int> list_tile_lo, list_count;
  int max_list_rows = 0;
  DevBuf qbuf, qg, lists, counts, stage_in, tmp_sc, tmp_id, out_sc, out_id, desc, ploc, gq, sums, cnts;
  DevBuf d_list_count, d_list_tile_lo, plan;   // device copies of the list layout; plan = lcount | wg_first | cursor | n_wg
  DevBuf scores, sdesc;                        // "score segments + select" regime (ivf_scan.hip): fp32 segments, dense descriptors
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // search start | start of mrag_ivf_allowed_per_list's upload | (unused) | search end
  std::vector<hipEvent_t> cev;    // per chunk of the last search: list scan begin, list scan end
  int n_chunks = 0;               // chunks of the last search (mrag_ivf_last_timing sums their scan brackets)
  DevBuf stats;                   // device accumulators of the last search: int64 rows streamed by the list scans, int64 workgroups
  bool timed = false, end_recorded = false;
  // filtered search (mrag_ivf_search_filtered): the allow-set over the original rows (fw.fbits), its image over the stored
  // positions, the per-list allowed counts and the live-list bitset
  FilterWork fw;
  DevBuf fstored;                 // uint32 bitset over the n_sorted stored positions
  DevBuf flist;                   // int counts [nlist] | int live-list count | uint32 live bits [round256(nlist) / 32] | int caller counts [nlist]
  DevBuf flast;                   // int allowed rows, int live lists of the last path-P search (copied at its end, read on demand)
  int32_t* h_lallow = nullptr;    // pinned staging of a host list_allowed
  hipEvent_t ev_lallow = nullptr; // recorded after the last copy out of h_lallow
  int last_fpath = -1;            // MRAG_IVF_FILTER_PROBE / _EXACT of the last filtered search, -1 = none
  int64_t last_fallowed = -1;     // its allowed rows (-1: still on the device, flast word 0)
  int last_flive = -1;            // its live lists (-1: on the device, flast word 1; -2: not computed, path E)
  // range search (mrag_ivf_search_range, mrag_ivf_self_join)
  DevBuf inv_pos;                 // int64 [n]: original row -> stored position (built on the first exclusion after a regroup)
  bool inv_valid = false;
  DevBuf excl;                    // int64 [nq] excluded rows of a host caller | int64 [nq] their stored positions
  DevBuf out_cnt;                 // int64 [nq] counts of a chunk with host outputs
  // fp8 scan copy (mrag_ivf_enable_fp8): sorted8 [n_sorted][ld8] next to `sorted`, rebuilt with it by ivf_finalize
  bool fp8 = false;
  int ld8 = 0;
  uint8_t* sorted8 = nullptr;
  DevBuf qbuf8, cand;             // quantised queries [nq padded][ld8]; candidates of a chunk: int64 [nq][refine] local rows
  int last_refine = -1;           // of the last mrag_ivf_search_fp8
  ~IvfIndex() override {
    if (sorted8) (void)hipFree(sorted8);
    qbuf8.release(); cand.release();
    inv_pos.release(); excl.release(); out_cnt.release();
    fw.release(); fstored.release(); flist.release(); flast.release();
    if (ev_lallow) (void)hipEventDestroy(ev_lallow);
    if (h_lallow) (void)hipHostFree(h_lallow);
    for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : cev) if (e) (void)hipEventDestroy(e);
    for (void* p : {(void*)cen, (void*)raw, (void*)assign, (void*)sorted, (void*)row_ids}) if (p) (void)hipFree(p);
    for (DevBuf* b : {&qbuf, &qg, &lists, &counts, &stage_in, &tmp_sc, &tmp_id, &out_sc, &out_id, &desc, &ploc, &gq, &sums, &cnts, &d_list_count, &d_list_tile_lo, &plan, &scores, &sdesc, &stats}) b->release();
  }
};

static size_t esize(int dt) { return dt == MRAG_F32 ? 4 : dt == MRAG_F64 ? 8 : (dt == MRAG_F16 || dt == MRAG_BF16) ? 2 : 0; }

__global__ void gather_rows_kernel(const uint16_t* __restrict__ src, const int64_t* __restrict__ idx, int64_t n, int ld,
                                   uint16_t* __restrict__ dst, int zero_fill) {
  // one wave per destination row; idx < 0 -> zero row
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const int64_t s = idx[r];
  if (s < 0 && !zero_fill) return;   // search-time query slabs: rows past a group's queries are never read
  const uint4* sp = (const uint4*)(src + (size_t)(s < 0 ? 0 : s) * ld);
  uint4* dp = (uint4*)(dst + (size_t)r * ld);
  for (int i = lane; i < ld / 8; i += 64) dp[i] = s < 0 ? make_uint4(0, 0, 0, 0) : sp[i];
}

// fp8 bytes of the original rows [row0, row0 + n) (mrag_ivf_get_rows_fp8): out [n][dim] from the regrouped copy through inv
__global__ void gather_rows8_kernel(const uint8_t* __restrict__ sorted8, int ld8, const int64_t* __restrict__ inv, int64_t row0,
                                    int64_t n, int dim, uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * dim) return;
  const int64_t r = i / dim;
  out[i] = sorted8[(size_t)inv[row0 + r] * ld8 + (i - r * dim)];
}

// ---- search-time regrouping on the device: list -> the (query, probe) pairs that hit it -------------
// probes [npairs] = list id per (query, probe slot) (< 0: none).  Pass 1 counts the pairs per list;
// pass 2 (one block) turns the counts into "first workgroup of the list" (256 queries per workgroup)
// and writes the workgroup descriptors; pass 3 hands every pair its (workgroup, slot) with an atomic
// cursor per list.  The slot order inside a list depends on the atomics' order, the results do not:
// every (query, row) score is computed the same way whichever slot the query sits in.
__global__ void ivf_count_kernel(const int64_t* __restrict__ probes, int64_t npairs, const int* __restrict__ list_count,
                                 int* __restrict__ lcount) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npairs) return;
  const int64_t l = probes[i];
  if (l >= 0 && list_count[l] > 0) atomicAdd(&lcount[l], 1);
}

__global__ __launch_bounds__(1024) void ivf_plan_kernel(const int* __restrict__ lcount, const int* __restrict__ list_count,
                                                        const int* __restrict__ list_tile_lo, int nlist,
                                                        int* __restrict__ wg_first, int* __restrict__ cursor,
                                                        int* __restrict__ desc, int desc_cap, int* __restrict__ n_wg_out,
                                                        unsigned long long* __restrict__ stats) {
  __shared__ int part[1024];
  __shared__ int carry;
  __shared__ unsigned long long rows_acc;
  const int tid = threadIdx.x;
  if (tid == 0) { carry = 0; rows_acc = 0ull; }
  __syncthreads();
  for (int base = 0; base < nlist; base += 1024) {
    const int l = base + tid;
    const int cnt = l < nlist ? lcount[l] : 0;
    const int nt = (cnt + 255) >> 8;
    if (nt && l < nlist) atomicAdd(&rows_acc, (unsigned long long)nt * (unsigned long long)list_count[l]);
    part[tid] = nt;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {           // inclusive scan (Hillis-Steele)
      const int v = tid >= off ? part[tid - off] : 0;
      __syncthreads();
      part[tid] += v;
      __syncthreads();
    }
    const int first = carry + part[tid] - nt;
    if (l < nlist) {
      wg_first[l] = first;
      cursor[l] = 0;
      const int tlo = list_tile_lo[l], lc = list_count[l];
      for (int c = 0; c < nt; ++c) {
        const int wgi = first + c;
        if (wgi < desc_cap) {
          int* d = desc + (size_t)wgi * 8;
          d[0] = wgi * 256;
          d[1] = min(256, cnt - c * 256);
          d[2] = tlo;
          d[3] = tlo + ((lc + 255) >> 8);
          d[4] = tlo * 256 + lc;
          d[5] = 0; d[6] = 0; d[7] = 0;
        }
      }
    }
    __syncthreads();
    if (tid == 1023) carry += part[1023];
    __syncthreads();
  }
  if (tid == 0) {
    *n_wg_out = carry;
    if (stats) { atomicAdd(&stats[0], rows_acc); atomicAdd(&stats[1], (unsigned long long)carry); }
  }
}

// (score-segment regime, pinfo != nullptr: the thread that draws slot 0 of a query group also writes the group's scan
// descriptors -- one per IVFS_CHUNK_ROWS rows of the list --, so the single-workgroup plan kernel only runs the prefix sums)
__global__ void ivf_scatter_kernel(const int64_t* __restrict__ probes, int64_t npairs, int nprobe,
                                   const int* __restrict__ list_count, const int* __restrict__ wg_first,
                                   int* __restrict__ cursor, int64_t* __restrict__ gq, int2* __restrict__ ploc, int qshift,
                                   const long long* __restrict__ foff, const int* __restrict__ list_tile_lo, int4* __restrict__ pinfo,
                                   const int* __restrict__ lcount, const int* __restrict__ dfirst, int* __restrict__ desc, int desc_cap) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npairs) return;
  const int64_t l = probes[i];
  if (l < 0 || list_count[l] == 0) {
    if (pinfo) pinfo[i] = make_int4(0, 0, 0, 0); else ploc[i] = make_int2(-1, 0);
    return;
  }
  const int pos = atomicAdd(&cursor[l], 1);
  const int wgi = wg_first[l] + (pos >> qshift), slot = pos & ((1 << qshift) - 1);   // 2^qshift queries per workgroup
  gq[((size_t)wgi << qshift) + slot] = i / nprobe;
  if (pinfo) {
    // score-segment regime: everything the per-query selection needs about this pair, in one 16-byte record -- its score
    // segment (its group's block + slot x pitch), the rows and the first stored row of the whole LIST (the list's rows may be
    // cut over several scan descriptors; every one of them writes its rows of this segment)
    const int lc = list_count[l], grp = pos >> qshift, tlo = list_tile_lo[l];
    const long long pitch = (lc + IVFS_PITCH_ALIGN - 1) / IVFS_PITCH_ALIGN * IVFS_PITCH_ALIGN;
    const long long gso = foff[l] + (long long)grp * IVFS_QUERIES * pitch;      // the group's score block
    const long long so = gso + (long long)slot * pitch;
    pinfo[i] = make_int4((int)(unsigned)(so & 0xFFFFFFFFll), (int)(so >> 32), lc, tlo * 256);
    if (slot == 0) {
      const int cnt = lcount[l], nch = (lc + IVFS_CHUNK_ROWS - 1) / IVFS_CHUNK_ROWS;
      for (int r = 0; r < nch; ++r) {
        const int di = dfirst[l] + grp * nch + r;
        if (di < desc_cap) {
          int4* d = (int4*)(desc + (size_t)di * IVFS_DESC_WORDS);
          d[0] = make_int4(wgi * IVFS_QUERIES, min(IVFS_QUERIES, cnt - grp * IVFS_QUERIES), tlo * 256 + r * IVFS_CHUNK_ROWS,
                           min(IVFS_CHUNK_ROWS, lc - r * IVFS_CHUNK_ROWS));
          d[1] = make_int4(r * IVFS_CHUNK_ROWS, (int)(unsigned)(gso & 0xFFFFFFFFll), (int)(gso >> 32), (int)pitch);
        }
      }
    }
  } else {
    ploc[i] = make_int2(wgi, slot);
  }
}

// Plan of the "score segments + select" regime (ivf_scan.hip).  A list probed by cnt queries becomes ceil(cnt / 128) query
// GROUPS (one block of scores S[query slot of the group][pitch = list rows rounded to 32] each, one block of 128 query-row
// ids in gq each) x ceil(rows / IVFS_CHUNK_ROWS) row CHUNKS = that many scan descriptors: a long list (skewed data: thousands
// of rows where the median list has a hundred) is scanned by several workgroups instead of being one workgroup's tail.
// Measured (round 3, one box, whole search): chunk = whole list / 1024 / 512 / 256 / 128 rows -- C5 share (152-row lists) 0.743 /
// - / 0.743 / 0.713 / 0.700 ms; 5 M rows (1 220-row lists) 4.02 / 3.81 / 3.64 / 3.51 / 3.56 ms; Zipf-sized lists (0 ... 5 330 rows),
// nprobe 1 / 32: 0.98 / 1.38 -> 0.62 / 1.13 -> 0.61 / 1.05 -> 0.52 / 0.94 -> 0.50 / 0.94 ms.
// out[0] = descriptors, out[1..2] = score floats; per list: wg_first = first group, dfirst = first descriptor, foff = float offset of its score blocks.
__global__ __launch_bounds__(1024) void ivf_plan_scores_kernel(const int* __restrict__ lcount, const int* __restrict__ list_count,
                                                               int nlist, int* __restrict__ wg_first, int* __restrict__ cursor,
                                                               int* __restrict__ dfirst, long long* __restrict__ foff,
                                                               int* __restrict__ out, unsigned long long* __restrict__ stats) {
  // three exclusive prefix sums over the lists (query groups, scan descriptors, score floats): wave scans by shuffles, the 16
  // wave totals through LDS -- two barriers per 1024 lists (the Hillis-Steele form took 20 per sum and wrote every descriptor
  // from this one workgroup: 37 us at the C5 share, 86 us over 5 M rows; the descriptors are now written by ivf_scatter_kernel)
  __shared__ int wt_g[16], wt_d[16];
  __shared__ long long wt_f[16];
  __shared__ unsigned long long rows_acc;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int carry = 0, dcarry = 0;
  long long fcarry = 0;
  if (tid == 0) rows_acc = 0ull;
  __syncthreads();
  for (int base = 0; base < nlist; base += 1024) {
    const int l = base + tid;
    const int cnt = l < nlist ? lcount[l] : 0;
    const int lc = l < nlist ? list_count[l] : 0;
    const int nt = (cnt + IVFS_QUERIES - 1) / IVFS_QUERIES;
    const int nch = (lc + IVFS_CHUNK_ROWS - 1) / IVFS_CHUNK_ROWS;
    if (nt && lc) atomicAdd(&rows_acc, (unsigned long long)nt * (unsigned long long)lc);   // rows this list's workgroups stream
    const int pitch = (lc + IVFS_PITCH_ALIGN - 1) / IVFS_PITCH_ALIGN * IVFS_PITCH_ALIGN;
    const long long fl = (long long)cnt * pitch;
    int ig = nt, id = nt * nch;
    long long iff = fl;
    for (int off = 1; off < 64; off <<= 1) {
      const int vg = __shfl_up(ig, off), vd = __shfl_up(id, off);
      const long long vf = __shfl_up(iff, off);
      if (lane >= off) { ig += vg; id += vd; iff += vf; }
    }
    if (lane == 63) { wt_g[w] = ig; wt_d[w] = id; wt_f[w] = iff; }
    __syncthreads();
    int bg = 0, bd = 0, tg = 0, td = 0;
    long long bf = 0, tf = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int g_ = wt_g[i], d_ = wt_d[i];
      const long long f_ = wt_f[i];
      if (i < w) { bg += g_; bd += d_; bf += f_; }
      tg += g_; td += d_; tf += f_;
    }
    if (l < nlist) {
      wg_first[l] = carry + bg + ig - nt;
      dfirst[l] = dcarry + bd + id - nt * nch;
      foff[l] = fcarry + bf + iff - fl;
      cursor[l] = 0;
    }
    carry += tg; dcarry += td; fcarry += tf;     // (every thread keeps the same running totals)
    __syncthreads();                             // the wave totals are rewritten by the next 1024 lists
  }
  if (tid == 0) {
    out[0] = dcarry;
    out[1] = (int)(unsigned)(fcarry & 0xFFFFFFFFll);
    out[2] = (int)(fcarry >> 32);
    if (stats) { atomicAdd(&stats[0], rows_acc); atomicAdd(&stats[1], (unsigned long long)dcarry); }
  }
}

// nprobe == nlist: every query probes every list (the exhaustive limit, == brute force)
__global__ void ivf_all_lists_kernel(int64_t* __restrict__ probes, int64_t npairs, int nlist) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < npairs) probes[i] = i % nlist;
}

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

__global__ void ids_to_i32_kernel(const int64_t* __restrict__ ids, int64_t n, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (int32_t)ids[i];
}

template <int BF16>
__global__ void kmeans_accum_kernel(const uint16_t* __restrict__ x, const int64_t* __restrict__ a, int64_t n, int ld, int dim,
                                    float* __restrict__ sums, int* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const int64_t c = a[r];
  if (c < 0) return;
  const uint16_t* row = x + (size_t)r * ld;
  for (int i = lane; i < dim; i += 64) {
    float v;
    if (BF16) v = __uint_as_float((uint32_t)row[i] << 16);
    else { _Float16 h; __builtin_memcpy(&h, &row[i], 2); v = (float)h; }
    atomicAdd(&sums[(size_t)c * dim + i], v);
  }
  if (lane == 0) atomicAdd(&cnt[c], 1);
}

// after the accumulation, one thread per (list, dim) element of sums: an empty list takes its centroid back (it keeps
// it); MEAN (inner product) turns the sum of a non-empty list into the mean, (float)((double)sum / count), one rounding
// to fp32 like K1's own.  Cosine leaves the sum: the normalisation that follows makes the division redundant.
template <int BF16, int MEAN>
__global__ void kmeans_keep_empty_kernel(const uint16_t* __restrict__ cen, int ld, int dim, int nlist, const int* __restrict__ cnt,
                                         float* __restrict__ sums) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)nlist * dim) return;
  const int c = (int)(i / dim), d = (int)(i % dim);
  const int m = cnt[c];
  if (m > 0) {
    if (MEAN) sums[i] = (float)((double)sums[i] / (double)m);
    return;
  }
  const uint16_t b = cen[(size_t)c * ld + d];
  float v;
  if (BF16) v = __uint_as_float((uint32_t)b << 16);
  else { _Float16 h; __builtin_memcpy(&h, &b, 2); v = (float)h; }
  sums[i] = v;   // an empty list keeps its centroid
}

static int ivf_grow(IvfIndex* ix, int64_t need, hipStream_t stream) {
  if (need <= ix->cap) return MRAG_OK;
  int64_t cap = bf_round_rows(std::max<int64_t>(need, ix->cap + ix->cap / 2));
  uint16_t* nr = nullptr;
  int32_t* na = nullptr;
  MRAG_HIP(hipMalloc((void**)&nr, (size_t)cap * ix->ld * 2));
  MRAG_HIP(hipMalloc((void**)&na, (size_t)cap * 4));
  MRAG_HIP(hipMemsetAsync(nr, 0, (size_t)cap * ix->ld * 2, stream));
  if (ix->n) {
    MRAG_HIP(hipMemcpyAsync(nr, ix->raw, (size_t)ix->n * ix->ld * 2, hipMemcpyDeviceToDevice, stream));
    MRAG_HIP(hipMemcpyAsync(na, ix->assign, (size_t)ix->n * 4, hipMemcpyDeviceToDevice, stream));
  }
  MRAG_HIP(hipStreamSynchronize(stream));
  if (ix->raw) (void)hipFree(ix->raw);
  if (ix->assign) (void)hipFree(ix->assign);
  ix->raw = nr; ix->assign = na; ix->cap = cap;
  return MRAG_OK;
}

// The dense launch (bf_launch) of nq prepared `queries` over n_rows prepared rows of `corpus`, in the index's layout and with its
// workspace.  The caller adds k and the outputs, and what only it needs: id_base, an allow-set, events, the descriptor mode's fields.
static BfLaunch ivf_launch(IvfIndex* ix, const uint16_t* corpus, int64_t n_rows, const void* queries, int64_t nq, hipStream_t stream) {
  BfLaunch a;
  a.corpus = corpus; a.n_rows = n_rows; a.queries = (const uint16_t*)queries; a.nq = nq;
  a.ld = ix->ld; a.dtype = ix->dtype;
  a.lists = &ix->lists; a.counts = &ix->counts; a.stream = stream;
  return a;
}

// nearest centroid (k = 1) of prepared rows x [n][ld] (n need not be a multiple of 256: the
// buffer behind it must be readable up to the next multiple) -> out_ids int64 [n]
static int ivf_assign_rows(IvfIndex* ix, const uint16_t* x, int64_t n, int64_t* out_ids, float* out_sc, hipStream_t stream) {
  BfLaunch a = ivf_launch(ix, ix->cen, ix->nlist, x, n, stream);
  a.k = 1; a.out_scores = out_sc; a.out_ids = out_ids;
  return bf_launch(a);
}

// a caller's rows: n rows of ix->dim elements of any supported dtype, in host or device memory
struct IvfRows { const void* p; int64_t n; int dtype, normalize, is_device; };

// rows -> prepared storage rows at dst (device), padded buffer rows zeroed by caller
static int ivf_prepare(IvfIndex* ix, const IvfRows& r, uint16_t* dst, hipStream_t stream) {
  const void* src = r.p;
  if (!r.is_device) {
    const size_t bytes = (size_t)r.n * ix->dim * esize(r.dtype);
    MRAG_TRY(ix->stage_in.ensure(bytes));
    MRAG_HIP(hipMemcpyAsync(ix->stage_in.p, r.p, bytes, hipMemcpyHostToDevice, stream));
    src = ix->stage_in.p;
  }
  return launch_prep_rows(src, r.dtype, r.n, ix->dim, dst, ix->ld, ix->dtype, r.normalize && ix->metric == MRAG_METRIC_COSINE, stream);
}

static uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the fp8 copy of the regrouped rows: every byte of sorted8 [n_sorted][ld8] is written (pad rows of `sorted` are zero,
// pad columns are zeroed by the kernel)
static int ivf_build_sorted8(IvfIndex* ix, hipStream_t stream) {
  if (ix->sorted8) (void)hipFree(ix->sorted8);
  ix->sorted8 = nullptr;
  const size_t bytes8 = (size_t)ix->n_sorted * ix->ld8;
  hipError_t e = hipMalloc((void**)&ix->sorted8, bytes8);
  if (e != hipSuccess) { (void)hipGetLastError(); ix->sorted8 = nullptr; return fail(MRAG_ERR_OOM, "hipMalloc(%zu) for the fp8 rows failed: %s", bytes8, hipGetErrorString(e)); }
  return launch_quant_rows_fp8(ix->sorted, ix->ld, ix->dtype == MRAG_BF16 ? 1 : 0, ix->n_sorted, ix->sorted8, ix->ld8, stream);
}

// regroup rows by list: stable by original row, each list padded to a multiple of 256 rows
static int ivf_finalize(IvfIndex* ix, hipStream_t stream) {
  if (!ix->dirty) return MRAG_OK;
  const int64_t n = ix->n;
  std::vector<int32_t> a((size_t)n);
  if (n) MRAG_HIP(hipMemcpyAsync(a.data(), ix->assign, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
  MRAG_HIP(hipStreamSynchronize(stream));
  ix->list_count.assign(ix->nlist, 0);
  for (int64_t i = 0; i < n; ++i) ix->list_count[a[i]]++;
  ix->list_tile_lo.assign(ix->nlist, 0);
  int64_t tiles = 0;
  for (int l = 0; l < ix->nlist; ++l) { ix->list_tile_lo[l] = (int)tiles; tiles += (ix->list_count[l] + 255) / 256; }
  const int64_t ns = std::max<int64_t>(tiles, 1) * 256;
  std::vector<int64_t> perm((size_t)ns, -1);
  std::vector<int64_t> cur(ix->nlist);
  for (int l = 0; l < ix->nlist; ++l) cur[l] = (int64_t)ix->list_tile_lo[l] * 256;
  for (int64_t i = 0; i < n; ++i) perm[cur[a[i]]++] = i;
  if (ix->sorted) (void)hipFree(ix->sorted);
  if (ix->row_ids) (void)hipFree(ix->row_ids);
  if (ix->sorted8) (void)hipFree(ix->sorted8);
  ix->sorted = nullptr; ix->row_ids = nullptr; ix->sorted8 = nullptr;
  MRAG_HIP(hipMalloc((void**)&ix->sorted, (size_t)ns * ix->ld * 2));
  MRAG_HIP(hipMalloc((void**)&ix->row_ids, (size_t)ns * 8));
  MRAG_HIP(hipMemcpyAsync(ix->row_ids, perm.data(), (size_t)ns * 8, hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((ns + 3) / 4)), dim3(256), 0, stream, ix->raw ? ix->raw : ix->sorted, ix->row_ids, ns, ix->ld, ix->sorted, 1);
  MRAG_HIP(hipGetLastError());
  ix->n_sorted = ns;
  if (ix->fp8) MRAG_TRY(ivf_build_sorted8(ix, stream));
  MRAG_TRY(ix->d_list_count.ensure((size_t)ix->nlist * 4));
  MRAG_TRY(ix->d_list_tile_lo.ensure((size_t)ix->nlist * 4));
  MRAG_HIP(hipMemcpyAsync(ix->d_list_count.p, ix->list_count.data(), (size_t)ix->nlist * 4, hipMemcpyHostToDevice, stream));
  MRAG_HIP(hipMemcpyAsync(ix->d_list_tile_lo.p, ix->list_tile_lo.data(), (size_t)ix->nlist * 4, hipMemcpyHostToDevice, stream));
  MRAG_HIP(hipStreamSynchronize(stream));
  ix->max_list_rows = ix->list_count.empty() ? 0 : *std::max_element(ix->list_count.begin(), ix->list_count.end());
  ix->inv_valid = false;
  ix->dirty = false;
  return MRAG_OK;
}

}  // namespace mrag

using namespace mrag;

extern "C" {

int mrag_ivf_create(int dim, int nlist, int metric, int storage_dtype, int device, mrag_handle* out) {
  if (!out) return fail(MRAG_ERR_INVALID, "out is NULL");
  if (dim <= 0 || dim > 8192) return fail(MRAG_ERR_INVALID, "dim %d out of range", dim);
  if (nlist <= 0 || nlist > (1 << 20)) return fail(MRAG_ERR_INVALID, "nlist %d out of range", nlist);
  if (storage_dtype != MRAG_F16 && storage_dtype != MRAG_BF16) return fail(MRAG_ERR_INVALID, "storage dtype must be fp16 or bf16");
  MRAG_TRY(use_device(device));
  IvfIndex* ix = new IvfIndex();
  ix->kind = KIND_IVF; ix->device = device; ix->dim = dim; ix->ld = (int)round_up(dim, 64);
  ix->ld8 = (int)round_up(dim, FP8_K);
  ix->nlist = nlist; ix->metric = metric; ix->dtype = storage_dtype;
  const size_t cb = (size_t)bf_round_rows(nlist) * ix->ld * 2;
  if (hipMalloc((void**)&ix->cen, cb) != hipSuccess) { delete ix; return fail(MRAG_ERR_OOM, "centroid allocation failed"); }
  (void)hipMemset(ix->cen, 0, cb);
  for (auto& e : ix->ev)
    if (hipEventCreate(&e) != hipSuccess) { delete ix; return fail(MRAG_ERR_HIP, "hipEventCreate failed"); }
  *out = register_object(ix);
  return MRAG_OK;
}

int mrag_ivf_destroy(mrag_handle h) {
  Object* o = take(h, KIND_IVF);
  if (!o) return MRAG_ERR_INVALID;
  (void)hipSetDevice(o->device);
  (void)hipDeviceSynchronize();
  delete o;
  return MRAG_OK;
}

int mrag_ivf_set_centroids(mrag_handle h, const void* centroids, int src_dtype, int normalize, int is_device, void* stream_) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (!centroids || !esize(src_dtype)) return fail(MRAG_ERR_INVALID, "bad centroid buffer / dtype");
  if (ix->n) return fail(MRAG_ERR_INVALID, "centroids cannot change after rows were added");
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  MRAG_TRY(ivf_prepare(ix, {centroids, ix->nlist, src_dtype, normalize, is_device}, ix->cen, stream));
  MRAG_HIP(hipStreamSynchronize(stream));
  ix->has_centroids = true;
  return MRAG_OK;
}

int mrag_ivf_get_centroids(mrag_handle h, float* out, int out_is_device, void* stream_) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (!out) return fail(MRAG_ERR_INVALID, "out is NULL");
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  std::vector<uint16_t> hc((size_t)ix->nlist * ix->ld);
  MRAG_HIP(hipMemcpyAsync(hc.data(), ix->cen, hc.size() * 2, hipMemcpyDeviceToHost, stream));
  MRAG_HIP(hipStreamSynchronize(stream));
  std::vector<float> f((size_t)ix->nlist * ix->dim);
  for (int r = 0; r < ix->nlist; ++r)
    for (int c = 0; c < ix->dim; ++c) {
      const uint16_t b = hc[(size_t)r * ix->ld + c];
      float v;
      if (ix->dtype == MRAG_BF16) { uint32_t u = (uint32_t)b << 16; memcpy(&v, &u, 4); }
      else { _Float16 hh; memcpy(&hh, &b, 2); v = (float)hh; }
      f[(size_t)r * ix->dim + c] = v;
    }
  if (out_is_device) MRAG_HIP(hipMemcpy(out, f.data(), f.size() * 4, hipMemcpyHostToDevice));
  else memcpy(out, f.data(), f.size() * 4);
  return MRAG_OK;
}

int mrag_ivf_train(mrag_handle h, const void* rows, int64_t n, int src_dtype, int normalize, int rows_is_device, int iters,
                   uint64_t seed, void* stream_) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (!rows || !esize(src_dtype)) return fail(MRAG_ERR_INVALID, "bad rows buffer / dtype");
  if (n < ix->nlist) return fail(MRAG_ERR_INVALID, "need at least nlist = %d training rows, got %lld", ix->nlist, (long long)n);
  if (ix->n) return fail(MRAG_ERR_INVALID, "train before adding rows");
  if (iters < 0) return fail(MRAG_ERR_INVALID, "iters < 0");
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t npad = bf_round_rows(n);
  DevBuf x;
  MRAG_TRY(x.ensure((size_t)npad * ix->ld * 2));
  MRAG_HIP(hipMemsetAsync(x.p, 0, (size_t)npad * ix->ld * 2, stream));
  int st = ivf_prepare(ix, {rows, n, src_dtype, normalize, rows_is_device}, (uint16_t*)x.p, stream);
  if (st != MRAG_OK) { x.release(); return st; }
  // init: nlist distinct rows (Floyd's sampling from splitmix64(seed)), in ascending row order
  std::vector<int64_t> pick;
  {
    std::vector<int64_t> chosen;
    uint64_t s = seed;
    for (int64_t j = n - ix->nlist; j < n; ++j) {
      int64_t t = (int64_t)(splitmix64(s) % (uint64_t)(j + 1));
      if (std::find(chosen.begin(), chosen.end(), t) != chosen.end()) t = j;
      chosen.push_back(t);
    }
    std::sort(chosen.begin(), chosen.end());
    pick = chosen;
  }
  DevBuf dpick, ids, sc;
  st = dpick.ensure((size_t)ix->nlist * 8);
  if (st == MRAG_OK) st = ids.ensure((size_t)n * 8);
  if (st == MRAG_OK) st = sc.ensure((size_t)n * 4);
  if (st == MRAG_OK) st = ix->sums.ensure((size_t)ix->nlist * ix->dim * 4);
  if (st == MRAG_OK) st = ix->cnts.ensure((size_t)ix->nlist * 4);
  auto cleanup = [&]() { x.release(); dpick.release(); ids.release(); sc.release(); };
  if (st != MRAG_OK) { cleanup(); return st; }
  hipError_t e = hipMemcpyAsync(dpick.p, pick.data(), (size_t)ix->nlist * 8, hipMemcpyHostToDevice, stream);
  if (e != hipSuccess) { cleanup(); return fail(MRAG_ERR_HIP, "H2D failed"); }
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((ix->nlist + 3) / 4)), dim3(256), 0, stream, (const uint16_t*)x.p,
                     (const int64_t*)dpick.p, (int64_t)ix->nlist, ix->ld, ix->cen, 1);
  (void)hipStreamSynchronize(stream);
  for (int it = 0; it < iters; ++it) {
    st = ivf_assign_rows(ix, (const uint16_t*)x.p, n, (int64_t*)ids.p, (float*)sc.p, stream);
    if (st != MRAG_OK) { cleanup(); return st; }
    (void)hipMemsetAsync(ix->sums.p, 0, (size_t)ix->nlist * ix->dim * 4, stream);
    (void)hipMemsetAsync(ix->cnts.p, 0, (size_t)ix->nlist * 4, stream);
    const dim3 g((unsigned)((n + 3) / 4)), b(256);
    const dim3 g2((unsigned)(((int64_t)ix->nlist * ix->dim + 255) / 256));
    const bool mean = ix->metric != MRAG_METRIC_COSINE;   // inner product: centroid = mean of its rows, not their sum
    const uint16_t* xr = (const uint16_t*)x.p;
    const int64_t* idp = (const int64_t*)ids.p;
    float* sums = (float*)ix->sums.p;
    int* cnts = (int*)ix->cnts.p;
    if (ix->dtype == MRAG_BF16) {
      hipLaunchKernelGGL((kmeans_accum_kernel<1>), g, b, 0, stream, xr, idp, n, ix->ld, ix->dim, sums, cnts);
      if (mean) hipLaunchKernelGGL((kmeans_keep_empty_kernel<1, 1>), g2, b, 0, stream, ix->cen, ix->ld, ix->dim, ix->nlist, (const int*)cnts, sums);
      else hipLaunchKernelGGL((kmeans_keep_empty_kernel<1, 0>), g2, b, 0, stream, ix->cen, ix->ld, ix->dim, ix->nlist, (const int*)cnts, sums);
    } else {
      hipLaunchKernelGGL((kmeans_accum_kernel<0>), g, b, 0, stream, xr, idp, n, ix->ld, ix->dim, sums, cnts);
      if (mean) hipLaunchKernelGGL((kmeans_keep_empty_kernel<0, 1>), g2, b, 0, stream, ix->cen, ix->ld, ix->dim, ix->nlist, (const int*)cnts, sums);
      else hipLaunchKernelGGL((kmeans_keep_empty_kernel<0, 0>), g2, b, 0, stream, ix->cen, ix->ld, ix->dim, ix->nlist, (const int*)cnts, sums);
    }
    st = launch_prep_rows(ix->sums.p, MRAG_F32, ix->nlist, ix->dim, ix->cen, ix->ld, ix->dtype, ix->metric == MRAG_METRIC_COSINE, stream);
    if (st != MRAG_OK) { cleanup(); return st; }
  }
  e = hipStreamSynchronize(stream);
  cleanup();
  if (e != hipSuccess) return fail(MRAG_ERR_HIP, "k-means failed: %s", hipGetErrorString(e));
  ix->has_centroids = true;
  return MRAG_OK;
}

int mrag_ivf_add(mrag_handle h, const void* rows, int64_t n, int src_dtype, int normalize, int rows_is_device, void* stream_) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (n < 0) return fail(MRAG_ERR_INVALID, "n < 0");
  if (n == 0) return MRAG_OK;
  if (!rows || !esize(src_dtype)) return fail(MRAG_ERR_INVALID, "bad rows buffer / dtype");
  if (!ix->has_centroids) return fail(MRAG_ERR_INVALID, "train or set centroids before adding rows");
  if (ix->n + n > 0x7FFFFF00ll) return fail(MRAG_ERR_UNSUPPORTED, "more than 2^31 rows per index; shard the corpus");
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  // the assignment below reads the new rows in place as a prepared query buffer: whole 256-row tiles + 16 rows from `dst` on,
  // wherever the stored rows end (not on a tile boundary after an add of any other size), so the capacity covers that read
  MRAG_TRY(ivf_grow(ix, ix->n + bf_query_rows(n), stream));
  uint16_t* dst = ix->raw + (size_t)ix->n * ix->ld;
  MRAG_TRY(ivf_prepare(ix, {rows, n, src_dtype, normalize, rows_is_device}, dst, stream));
  MRAG_TRY(ix->tmp_id.ensure((size_t)n * 8));
  MRAG_TRY(ix->tmp_sc.ensure((size_t)n * 4));
  // (the raw buffer is zero beyond the stored rows and holds bf_query_rows(n) rows from dst on: safe to read as padded queries)
  MRAG_TRY(ivf_assign_rows(ix, dst, n, (int64_t*)ix->tmp_id.p, (float*)ix->tmp_sc.p, stream));
  hipLaunchKernelGGL(ids_to_i32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const int64_t*)ix->tmp_id.p, n, ix->assign + ix->n);
  MRAG_HIP(hipGetLastError());
  MRAG_HIP(hipStreamSynchronize(stream));
  ix->n += n;
  ix->dirty = true;
  return MRAG_OK;
}

int mrag_ivf_size(mrag_handle h, int64_t* out_rows) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (!out_rows) return fail(MRAG_ERR_INVALID, "out_rows is NULL");
  *out_rows = ix->n;
  return MRAG_OK;
}

int mrag_ivf_set_id_base(mrag_handle h, int64_t id_base) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  ix->id_base = id_base;
  return MRAG_OK;
}

int mrag_ivf_get_assignments(mrag_handle h, int32_t* out, int out_is_device, void* stream_) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (!out && ix->n) return fail(MRAG_ERR_INVALID, "out is NULL");
  if (!ix->n) return MRAG_OK;
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  MRAG_HIP(hipMemcpyAsync(out, ix->assign, (size_t)ix->n * 4, out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
  MRAG_HIP(hipStreamSynchronize(stream));
  return MRAG_OK;
}

}  // extern "C"

namespace mrag {

// The score buffer of the "score segments + select" regime: MRAG_IVF_SCORES_MB, default 16 GiB, 0 = always the fused kernel.
static int64_t ivf_scores_cap() {
  static const int64_t cap = [] { const char* e = getenv("MRAG_IVF_SCORES_MB"); return (int64_t)(e ? atoll(e) : 16384) << 20; }();
  return cap;
}

// Large batches are cut so that a chunk's score segments fit the score buffer even if every pair probes the longest
// list (ivf_scan.hip's regime, without a host round trip); results are per query, so the chunks are independent.
// Every chunk streams the probed lists again, so the default buffer is generous (16 GiB of the 288: C5's 10 000 x 32
// pairs over 5 M rows need 1.6 GB, their no-round-trip bound ~5 GB); MRAG_IVF_SCORES_MB sets it, 0 = fused regime.
// -> queries per chunk (the last chunk may be shorter)
static int64_t ivf_chunk_queries(const IvfIndex* ix, int64_t nq, int nprobe) {
  const int64_t cap = ivf_scores_cap();
  const int64_t per_query = std::max<int64_t>((int64_t)std::min(nprobe, 256) * ivfs_pitch(ix->max_list_rows), ivfs_pitch(ix->nlist)) * 4;
  int64_t chunk = std::max<int64_t>(1024, cap / std::max<int64_t>(per_query, 1) / IVFS_QUERIES * IVFS_QUERIES);
  if (!(cap > 0 && nprobe <= 256 && nq > chunk)) chunk = nq;
  else chunk = round_up((nq + (nq + chunk - 1) / chunk - 1) / ((nq + chunk - 1) / chunk), IVFS_QUERIES);   // equal chunks
  return chunk;
}

// range and fp8 searches have no fused form: what ("range" / "fp8") is refused, and why
static int ivf_segments_only(const char* what, const char* why) { return fail(MRAG_ERR_UNSUPPORTED, "IVF %s search runs in the score-segment regime only: %s", what, why); }

// the per-chunk events of a search in n_chunks chunks: list scan begin, list scan end
static int ivf_grow_cev(IvfIndex* ix, int n_chunks) {
  while ((int)ix->cev.size() < 2 * n_chunks) {
    hipEvent_t e = nullptr;
    MRAG_HIP(hipEventCreate(&e));
    ix->cev.push_back(e);
  }
  return MRAG_OK;
}

// An asynchronous call (device inputs + results) returns with the handle's scratch buffers still in use on ITS stream; a call
// on another stream first waits for that one's end event (a no-op on the same stream or after a synchronous call).
static int ivf_wait_previous(IvfIndex* ix, hipStream_t stream) {
  if (ix->end_recorded) MRAG_HIP(hipStreamWaitEvent(stream, ix->ev[3], 0));
  return MRAG_OK;
}
// ... and the end event of this call: the handle's buffers are in use on `stream` until here
static int ivf_record_end(IvfIndex* ix, hipStream_t stream) {
  MRAG_HIP(hipEventRecord(ix->ev[3], stream));
  ix->end_recorded = true;
  return MRAG_OK;
}

// inv_pos = original row -> stored position of the current regroup (built once after every regroup)
static int ivf_ensure_inv_pos(IvfIndex* ix, hipStream_t stream) {
  if (ix->inv_valid) return MRAG_OK;
  MRAG_TRY(ix->inv_pos.ensure((size_t)std::max<int64_t>(ix->n, 1) * 8));
  hipLaunchKernelGGL(ivf_inverse_pos_kernel, dim3((unsigned)((ix->n_sorted + 255) / 256)), dim3(256), 0, stream,
                     (const int64_t*)ix->row_ids, ix->n_sorted, ix->n, (int64_t*)ix->inv_pos.p);
  MRAG_HIP(hipGetLastError());
  ix->inv_valid = true;
  return MRAG_OK;
}

// nq, k and nprobe of the plain, filtered and fp8 searches' kind
static int ivf_check_nq_k(int64_t nq, int k, int nprobe) {
  if (nq < 0 || k <= 0 || nprobe <= 0) return fail(MRAG_ERR_INVALID, "bad nq / k / nprobe");
  if (k > bf_max_k()) return fail(MRAG_ERR_UNSUPPORTED, "k = %d exceeds the fused top-k limit %d", k, bf_max_k());
  return MRAG_OK;
}
static int ivf_check_range_args(int64_t nq, int k, int nprobe, float min_score, const void* out_counts) {
  if (nq < 0 || k <= 0 || nprobe <= 0) return fail(MRAG_ERR_INVALID, "bad nq / k / nprobe");
  if (k > 256) return fail(MRAG_ERR_INVALID, "range search: k = %d, supported are 1..256 (the per-query selection's limit)", k);
  if (!std::isfinite(min_score)) return fail(MRAG_ERR_INVALID, "min_score must be finite");
  if (nq > 0 && !out_counts) return fail(MRAG_ERR_INVALID, "out_counts is NULL");
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
// _search_fp8 share around their own argument checks and their mode's own work.
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
  int begin() {
    nprobe = std::min(nprobe, ix->nlist);
    // probe selection = top-nprobe over the centroids: the fused kernel up to 64, the streaming kernel up to 256
    // (8 queries per launch); nprobe == nlist needs no selection at all
    if (nprobe > bf_max_k_wide() && nprobe < ix->nlist)
      return fail(MRAG_ERR_UNSUPPORTED, "nprobe = %d: supported are 1..%d and nlist (= %d, exhaustive)", nprobe, bf_max_k_wide(), ix->nlist);
    if (nq == 0) return MRAG_OK;
    if (!queries || !out_scores || !out_ids || !esize(q_dtype)) return fail(MRAG_ERR_INVALID, "bad buffer / dtype");
    if (!ix->has_centroids) return fail(MRAG_ERR_INVALID, "index has no centroids");
    MRAG_TRY(use_device(ix->device));
    MRAG_TRY(ivf_finalize(ix, stream));
    chunk = ivf_chunk_queries(ix, nq, nprobe);
    if (chunk > (1 << 20)) return fail(MRAG_ERR_UNSUPPORTED, "nq too large for one IVF batch (2^20); cut the query batch");
    ix->timed = false;
    return ivf_wait_previous(ix, stream);
  }

  // (range, fp8) the refusals known before any chunk runs; a refused call has recorded nothing
  int refuse_fused() const {
    if (ivf_scores_cap() <= 0) return ivf_segments_only(what(), "the score buffer is disabled (MRAG_IVF_SCORES_MB = 0)");
    if (nprobe > 256) return ivf_segments_only(what(), "more than 256 probed lists per query (exhaustive probing with nlist > 256)");
    return MRAG_OK;
  }

  // The search's device work starts here: ev[0], and its device accumulators (rows streamed, workgroups) start at zero.
  // record_ev0 = false: the filtered search, whose ev[0] filter_upload records behind the host-side packing of a host allow-set.
  int start(bool record_ev0 = true) {
    if (record_ev0) MRAG_HIP(hipEventRecord(ix->ev[0], stream));
    MRAG_TRY(ix->stats.ensure(16));
    MRAG_HIP(hipMemsetAsync(ix->stats.p, 0, 16, stream));
    return MRAG_OK;
  }

  // the chunks, one after another; ix->n_chunks is theirs once all have run
  int run_chunks();

  // (range) start, then the excluded rows as stored positions in ix->excl's second half (sized by the caller) -- rows: device
  // int64 [nq], or NULL with self_row0 >= 0 for "query i excludes row self_row0 + i", or neither: no exclusion --, then the chunks
  int run_range(const int64_t* d_excl_rows, int64_t self_row0) {
    MRAG_TRY(refuse_fused());
    MRAG_TRY(start());
    if (d_excl_rows || self_row0 >= 0) {
      MRAG_TRY(ivf_ensure_inv_pos(ix, stream));
      int64_t* d_pos = (int64_t*)ix->excl.p + nq;
      hipLaunchKernelGGL(ivf_excl_pos_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, stream, d_excl_rows, self_row0, nq, ix->n,
                         (const int64_t*)ix->inv_pos.p, d_pos);
      MRAG_HIP(hipGetLastError());
      excl_pos = d_pos;
    }
    return run_chunks();
  }

  // The search's device work is done: ev[3], the search is timed.  Host buffers (pageable memory) must not be touched by the
  // caller before the copies are done: the call then returns when they have landed; otherwise it is asynchronous on `stream`.
  int finish(bool host_buffer_involved) {
    MRAG_TRY(ivf_record_end(ix, stream));
    ix->timed = true;
    if (host_buffer_involved) MRAG_HIP(hipStreamSynchronize(stream));
    return MRAG_OK;
  }
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
  // caller's buffers, or out_sc / out_id (out_cnt) for host outputs, which copy_back returns.
  int stage_outputs() {
    d_sc = s.out_scores + (size_t)off * s.k; d_id = s.out_ids + (size_t)off * s.k;
    if (rg) d_cnt = s.out_counts + off;
    if (s.out_is_device) return MRAG_OK;
    MRAG_TRY(ix->out_sc.ensure((size_t)nq * s.k * 4));
    MRAG_TRY(ix->out_id.ensure((size_t)nq * s.k * 8));
    d_sc = (float*)ix->out_sc.p; d_id = (int64_t*)ix->out_id.p;
    if (rg) { MRAG_TRY(ix->out_cnt.ensure((size_t)nq * 8)); d_cnt = (int64_t*)ix->out_cnt.p; }
    return MRAG_OK;
  }

  // Needs nothing.  Leaves ix->qbuf = the chunk's queries in the storage dtype, zero padded to bf_query_rows(nq) rows; fp8:
  // their quantised image in ix->qbuf8 (zero pad rows too, the scan's pad row nq among them), ix->cand sized for the candidates.
  int prepare_queries() {
    const int64_t nq_pad = bf_query_rows(nq);
    const size_t row = (size_t)ix->ld * 2;
    MRAG_TRY(ix->qbuf.ensure((size_t)nq_pad * row));
    MRAG_HIP(hipMemsetAsync((char*)ix->qbuf.p + (size_t)nq * row, 0, (size_t)(nq_pad - nq) * row, stream));
    if (rg && s.stored_rows)
      MRAG_HIP(hipMemcpyAsync(ix->qbuf.p, (const char*)s.queries + (size_t)off * row, (size_t)nq * row, hipMemcpyDeviceToDevice, stream));
    else
      MRAG_TRY(ivf_prepare(ix, {(const char*)s.queries + (size_t)off * ix->dim * esize(s.q_dtype), nq, s.q_dtype, s.normalize, s.queries_is_device},
                           (uint16_t*)ix->qbuf.p, stream));
    if (!f8) return MRAG_OK;
    MRAG_TRY(ix->qbuf8.ensure((size_t)nq_pad * ix->ld8));
    MRAG_TRY(launch_quant_queries_fp8((const uint16_t*)ix->qbuf.p, ix->ld, ix->dtype == MRAG_BF16 ? 1 : 0, nq_pad, (uint8_t*)ix->qbuf8.p,
                                      ix->ld8, stream));
    return ix->cand.ensure((size_t)nq * s.refine * 8);
  }

  // Needs qbuf.  Leaves the probed lists of every query in ix->tmp_id ([nq][nprobe] list ids, -1: none; filtered: live lists
  // only), the plan views over ix->plan, d_lcount zeroed -- or, with lcount_filled, already holding the queries per list.
  int select_probes() {
    MRAG_TRY(ix->tmp_id.ensure((size_t)nq * s.nprobe * 8));
    MRAG_TRY(ix->tmp_sc.ensure((size_t)nq * s.nprobe * 4));
    const int nl = ix->nlist;
    MRAG_TRY(ix->plan.ensure((size_t)(4 * nl + 4) * 4 + (size_t)nl * 8));
    d_lcount = (int*)ix->plan.p; d_wg_first = d_lcount + nl; d_cursor = d_wg_first + nl; d_dfirst = d_cursor + nl;
    d_nwg = d_dfirst + nl; d_foff = (long long*)(d_nwg + 4);
    MRAG_HIP(hipMemsetAsync(d_lcount, 0, (size_t)nl * 4, stream));
    if (s.nprobe == nl) {                  // exhaustive: no selection
      const int64_t np_ = nq * s.nprobe;
      hipLaunchKernelGGL(ivf_all_lists_kernel, dim3((unsigned)((np_ + 255) / 256)), dim3(256), 0, stream, (int64_t*)ix->tmp_id.p, np_, nl);
      MRAG_HIP(hipGetLastError());
    } else if (round_up(nq, IVFS_QUERIES) * ivfs_pitch(nl) * 4 <= ivf_scores_cap()) {   // dense score segments + top-k
      MRAG_TRY(ix->sdesc.ensure((size_t)ivfs_dense_n_desc(nq, nl) * IVFS_DESC_WORDS * 4));
      MRAG_TRY(ix->scores.ensure((size_t)(round_up(nq, IVFS_QUERIES) * ivfs_pitch(nl) * 4)));
      MRAG_TRY(ivfs_dense_topk(ix->cen, nl, (const uint16_t*)ix->qbuf.p, nq, ix->ld, ix->dtype, s.nprobe, (int*)ix->sdesc.p,
                               (float*)ix->scores.p, (float*)ix->tmp_sc.p, (int64_t*)ix->tmp_id.p, stream, d_lcount,
                               (const int*)ix->d_list_count.p, s.live_bits));
      lcount_filled = true;
    } else {                               // the centroid scores do not fit the score buffer: the fused kernel
      BfLaunch a = ivf_launch(ix, ix->cen, nl, ix->qbuf.p, nq, stream);
      a.k = s.nprobe; a.out_scores = (float*)ix->tmp_sc.p; a.out_ids = (int64_t*)ix->tmp_id.p;
      a.allow = s.live_bits;               // (filtered: dead lists are never probed; a pair without a list gets probe id -1)
      MRAG_TRY(bf_launch(a));
    }
    return MRAG_OK;
  }

  // Needs the probes and d_lcount (counted here unless lcount_filled).  The one place that decides the regime: leaves
  // use_scores / no_sync, or the mode's refusal.  With use_scores the score plan has run and ix->scores is sized for the
  // segments; only a plan whose bound does not fit comes back to the host (12 bytes: n_desc and the size of the segments).
  int plan() {
    const int64_t scores_cap = ivf_scores_cap();
    npairs = (size_t)nq * s.nprobe;
    wg_bound = (int64_t)std::min<size_t>((size_t)ix->nlist, npairs) + (int64_t)(npairs / IVFS_QUERIES) + 1;   // (covers the 256-query plan too)
    // score-segment regime: every group is cut into ceil(list rows / IVFS_CHUNK_ROWS) scan descriptors
    desc_bound = wg_bound * std::max<int64_t>(1, (ix->max_list_rows + IVFS_CHUNK_ROWS - 1) / IVFS_CHUNK_ROWS);
    MRAG_TRY(ix->desc.ensure((size_t)desc_bound * 8 * 4));
    MRAG_TRY(ix->gq.ensure((size_t)wg_bound * 256 * 8));
    MRAG_TRY(ix->ploc.ensure(npairs * 16));   // int2 (fused regime) or int4 (score segments) per pair
    if (!lcount_filled)
      hipLaunchKernelGGL(ivf_count_kernel, dim3(pgrid()), dim3(256), 0, stream, (const int64_t*)ix->tmp_id.p, (int64_t)npairs,
                         (const int*)ix->d_list_count.p, d_lcount);
    use_scores = scores_cap > 0 && s.nprobe <= 256;   // (the select kernel holds <= 256 segments per query; exhaustive probing takes the fused path)
    if ((rg || f8) && !use_scores) return ivf_segments_only(s.what(), scores_cap > 0 ? "more than 256 probed lists per query" : "the score buffer is disabled (MRAG_IVF_SCORES_MB = 0)");
    // Score floats of this chunk: known exactly only on the device (sum over the probed lists of queries x rows).  When
    // even the bound "every pair probes the longest list" fits the buffer, nothing comes back to the host at all: the
    // scan is launched over the BOUND of the descriptor count and reads the real one from device memory.
    const int64_t max_pitch = ivfs_pitch(ix->max_list_rows);
    no_sync = use_scores && (int64_t)npairs * max_pitch * 4 <= scores_cap;
    // (a filtered search only comes here when it fits: mrag_ivf_search_filtered runs path E otherwise)
    if (s.stored_bits && !no_sync) return fail(MRAG_ERR_INVALID, "filtered IVF chunk does not fit the score buffer");
    planned_scores = use_scores;
    if (!use_scores) return MRAG_OK;
    hipLaunchKernelGGL(ivf_plan_scores_kernel, dim3(1), dim3(1024), 0, stream, (const int*)d_lcount, (const int*)ix->d_list_count.p,
                       ix->nlist, d_wg_first, d_cursor, d_dfirst, d_foff, d_nwg, (unsigned long long*)ix->stats.p);
    MRAG_HIP(hipGetLastError());
    if (no_sync) return ix->scores.ensure((size_t)std::max<int64_t>((int64_t)npairs * max_pitch, 4) * 4);
    int plan_out[3] = {0, 0, 0};
    MRAG_HIP(hipMemcpyAsync(plan_out, d_nwg, 12, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipStreamSynchronize(stream));
    n_desc = plan_out[0];
    const int64_t floats = (int64_t)(uint32_t)plan_out[1] | ((int64_t)plan_out[2] << 32);
    if (n_desc < 0 || n_desc > desc_bound) return fail(MRAG_ERR_HIP, "IVF plan produced %d workgroups (bound %lld)", n_desc, (long long)desc_bound);
    if (floats * 4 > scores_cap && (rg || f8)) return ivf_segments_only(s.what(), "the score segments of one chunk exceed the score buffer (MRAG_IVF_SCORES_MB)");
    if (floats * 4 > scores_cap) { use_scores = false; return MRAG_OK; }   // (plain search: the fused regime takes the chunk)
    return ix->scores.ensure((size_t)std::max<int64_t>(floats, 4) * 4);
  }

  // Needs plan() with use_scores.  Scatters the pairs into their groups, scores every (query, probed list) pair into
  // ix->scores, selects per query; leaves the results at d_sc / d_id (/ d_cnt) -- fp8: via the candidates' exact re-rank.
  int scan_scores() {
    hipLaunchKernelGGL(ivf_scatter_kernel, dim3(pgrid()), dim3(256), 0, stream, (const int64_t*)ix->tmp_id.p, (int64_t)npairs, s.nprobe,
                       (const int*)ix->d_list_count.p, (const int*)d_wg_first, d_cursor, (int64_t*)ix->gq.p, nullptr, 7,
                       (const long long*)d_foff, (const int*)ix->d_list_tile_lo.p, (int4*)ix->ploc.p, (const int*)d_lcount,
                       (const int*)d_dfirst, (int*)ix->desc.p, (int)desc_bound);
    MRAG_HIP(hipGetLastError());
    MRAG_HIP(hipEventRecord(ev_scan0, stream));
    // (no_sync: the descriptor count stays on the device, the grid is its bound)
    MRAG_TRY(ivfs_scan(f8 ? (const uint16_t*)ix->sorted8 : ix->sorted, (const uint16_t*)(f8 ? ix->qbuf8.p : ix->qbuf.p),
                       f8 ? ix->ld8 / 2 : ix->ld, f8 ? MRAG_DT_FP8 : ix->dtype, nq, (const int*)ix->desc.p,
                       no_sync ? (int)desc_bound : n_desc, no_sync ? d_nwg : nullptr, (const int64_t*)ix->gq.p, (float*)ix->scores.p,
                       stream));
    IvfsRange sel_range{s.floor, s.excl_pos ? s.excl_pos + off : nullptr, d_cnt};
    if (f8)   // candidates: local rows in (fp8 score desc, row asc) order, -1 past the rows of the probed lists
      MRAG_TRY(ivfs_select_lists((const float*)ix->scores.p, ix->ploc.p, s.nprobe, nq, s.refine, ix->row_ids, 0, nullptr, (int64_t*)ix->cand.p, stream));
    else
      MRAG_TRY(ivfs_select_lists((const float*)ix->scores.p, ix->ploc.p, s.nprobe, nq, s.k, ix->row_ids, ix->id_base, d_sc, d_id, stream,
                                 s.stored_bits, rg ? &sel_range : nullptr));
    MRAG_HIP(hipEventRecord(ev_scan1, stream));
    if (f8)
      MRAG_TRY(launch_fp8_rerank(ix->raw, (const uint16_t*)ix->qbuf.p, ix->ld, ix->dtype == MRAG_BF16 ? 1 : 0, (const int64_t*)ix->cand.p, nq,
                                 s.refine, s.k, ix->id_base, d_sc, d_id, stream));
    return MRAG_OK;
  }

  // Needs plan() without use_scores (plain search only).  Plans 256-query workgroups, scatters, reads the workgroup count
  // back (4 bytes), gathers the queries per workgroup and runs the fused kernel in descriptor mode; results at d_sc / d_id.
  int scan_fused() {
    MRAG_HIP(hipMemsetAsync(ix->gq.p, 0xFF, (size_t)wg_bound * 256 * 8, stream));   // (the gather below reads whole 256-slot slabs)
    hipLaunchKernelGGL(ivf_plan_kernel, dim3(1), dim3(1024), 0, stream, (const int*)d_lcount, (const int*)ix->d_list_count.p,
                       (const int*)ix->d_list_tile_lo.p, ix->nlist, d_wg_first, d_cursor, (int*)ix->desc.p, (int)wg_bound, d_nwg,
                       planned_scores ? nullptr : (unsigned long long*)ix->stats.p);   // (a scores plan that turned out too big has already counted this chunk)
    hipLaunchKernelGGL(ivf_scatter_kernel, dim3(pgrid()), dim3(256), 0, stream, (const int64_t*)ix->tmp_id.p, (int64_t)npairs, s.nprobe,
                       (const int*)ix->d_list_count.p, (const int*)d_wg_first, d_cursor, (int64_t*)ix->gq.p, (int2*)ix->ploc.p, 8,
                       nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
    MRAG_HIP(hipGetLastError());
    int n_wg = -1;
    MRAG_HIP(hipMemcpyAsync(&n_wg, d_nwg, 4, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipStreamSynchronize(stream));
    if (n_wg < 0 || n_wg > wg_bound) return fail(MRAG_ERR_HIP, "IVF plan produced %d workgroups (bound %lld)", n_wg, (long long)wg_bound);
    if (n_wg) {
      MRAG_TRY(ix->qg.ensure((size_t)n_wg * 256 * ix->ld * 2));
      const int64_t ng = (int64_t)n_wg * 256;
      hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((ng + 3) / 4)), dim3(256), 0, stream, (const uint16_t*)ix->qbuf.p,
                         (const int64_t*)ix->gq.p, ng, ix->ld, (uint16_t*)ix->qg.p, 0);
      MRAG_HIP(hipGetLastError());
    }
    BfLaunch a = ivf_launch(ix, ix->sorted, 0, ix->qg.p, nq, stream);
    a.k = s.k; a.out_scores = d_sc; a.out_ids = d_id; a.id_base = ix->id_base;
    static const int dummy_desc = 0;
    a.wg_desc = n_wg ? (const int*)ix->desc.p : &dummy_desc; a.n_wg = n_wg;
    a.pair_loc = ix->ploc.p; a.nprobe = s.nprobe; a.row_ids = ix->row_ids;
    a.ev_k2_begin = ev_scan0; a.ev_k2_end = ev_scan1;
    return bf_launch(a);
  }

  // Needs the results at d_sc / d_id (/ d_cnt).  Host outputs: their copies are queued (the search synchronises at its end).
  int copy_back() const {
    if (s.out_is_device) return MRAG_OK;
    if (rg) MRAG_HIP(hipMemcpyAsync(s.out_counts + off, d_cnt, (size_t)nq * 8, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipMemcpyAsync(s.out_scores + (size_t)off * s.k, d_sc, (size_t)nq * s.k * 4, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipMemcpyAsync(s.out_ids + (size_t)off * s.k, d_id, (size_t)nq * s.k * 8, hipMemcpyDeviceToHost, stream));
    return MRAG_OK;
  }

  int run() {
    MRAG_TRY(stage_outputs());
    MRAG_TRY(prepare_queries());
    MRAG_TRY(select_probes());
    MRAG_TRY(plan());
    MRAG_TRY(use_scores ? scan_scores() : scan_fused());
    return copy_back();
  }
};

int IvfSearch::run_chunks() {
  const int n_chunks = (int)((nq + chunk - 1) / chunk);
  MRAG_TRY(ivf_grow_cev(ix, n_chunks));
  for (int c = 0; c < n_chunks; ++c) MRAG_TRY(IvfChunk(*this, c).run());
  ix->n_chunks = n_chunks;
  return MRAG_OK;
}

// ---- filtered search: AUTO's choice between path P (probe the live lists) and path E (filtered brute force) ------------
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

// flist layout (ints): counts [nlist] | live-list count (+ 3 pad) | live bits [round256(nlist) / 32] | caller counts [nlist]
static int* flist_counts(IvfIndex* ix) { return (int*)ix->flist.p; }
static int* flist_nlive(IvfIndex* ix) { return (int*)ix->flist.p + ix->nlist; }
static uint32_t* flist_live(IvfIndex* ix) { return (uint32_t*)ix->flist.p + ix->nlist + 4; }
static int* flist_caller(IvfIndex* ix) { return (int*)ix->flist.p + ix->nlist + 4 + bf_round_rows(ix->nlist) / 32; }

// (after filter_upload) the allow-set's image over the stored positions and the allowed rows per list
static int ivf_filter_stored(IvfIndex* ix, hipStream_t stream) {
  MRAG_TRY(ix->fstored.ensure((size_t)(ix->n_sorted / 32) * 4));
  MRAG_TRY(ix->flist.ensure(((size_t)2 * ix->nlist + 4 + (size_t)bf_round_rows(ix->nlist) / 32) * 4));
  hipLaunchKernelGGL(ivf_allow_stored_kernel, dim3((unsigned)ix->nlist), dim3(256), 0, stream, (const uint32_t*)ix->fw.fbits.p,
                     (const int64_t*)ix->row_ids, (const int*)ix->d_list_count.p, (const int*)ix->d_list_tile_lo.p,
                     (uint32_t*)ix->fstored.p, flist_counts(ix));
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

static int check_ivf_allow_args(IvfIndex* ix, const void* allow, int64_t allow_rows, int allow_format, int path) {
  MRAG_TRY(check_allow_args(allow_rows, ix->n, allow_format, path, "IVF filter"));
  if (!allow && ix->n > 0) return fail(MRAG_ERR_INVALID, "allow is NULL");
  return MRAG_OK;
}

}  // namespace mrag

extern "C" {

int mrag_ivf_search(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device, int nprobe,
                    int k, float* out_scores, int64_t* out_ids, int out_is_device, void* stream_) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  MRAG_TRY(ivf_check_nq_k(nq, k, nprobe));
  IvfSearch s{ix, (hipStream_t)stream_, nq, k, nprobe, queries, q_dtype, normalize, queries_is_device, out_scores, out_ids, out_is_device};
  MRAG_TRY(s.begin());
  if (nq == 0) return MRAG_OK;
  MRAG_TRY(s.start());
  MRAG_TRY(s.run_chunks());
  return s.finish(!out_is_device || !queries_is_device);
}

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
    MRAG_TRY(ix->excl.ensure((size_t)nq * 16));
    if (exclude_is_device) {
      d_excl = exclude_rows;
    } else {
      for (int64_t i = 0; i < nq; ++i)
        if (exclude_rows[i] < -1 || exclude_rows[i] >= ix->n)
          return fail(MRAG_ERR_INVALID, "exclude_rows[%lld] = %lld: a local row 0..%lld or -1", (long long)i, (long long)exclude_rows[i], (long long)ix->n - 1);
      MRAG_HIP(hipMemcpyAsync(ix->excl.p, exclude_rows, (size_t)nq * 8, hipMemcpyHostToDevice, s.stream));
      d_excl = (const int64_t*)ix->excl.p;
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
  MRAG_TRY(ix->excl.ensure((size_t)n * 16));
  MRAG_TRY(s.run_range(nullptr, row0));
  return s.finish(false);   // (everything on the device: never synchronises)
}

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
  MRAG_TRY(filter_upload(ix->fw, allow, ix->n, allow_format, allow_is_device, false, &m, ix->ev[1], stream));
  MRAG_TRY(ivf_filter_stored(ix, stream));
  MRAG_HIP(hipMemcpyAsync(out_counts, flist_counts(ix), (size_t)ix->nlist * 4, out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
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
  hipStream_t stream = s.stream;
  ix->last_fpath = -1;
  // path P runs the score-segment regime only, every chunk without a host round trip (IvfChunk::plan's no_sync case);
  // where that does not hold (nprobe == nlist, MRAG_IVF_SCORES_MB = 0, segments too big) the search runs path E
  const int64_t cap = ivf_scores_cap();
  const bool probe_fits = cap > 0 && s.nprobe < ix->nlist && s.chunk * s.nprobe * ivfs_pitch(ix->max_list_rows) * 4 <= cap;
  const int64_t n = ix->n;
  int64_t m = -1;
  // (ev[0], the search's start, is recorded in there: behind the host-side packing of a host allow-set)
  MRAG_TRY(filter_upload(ix->fw, allow, n, allow_format, allow_is_device, path != MRAG_IVF_FILTER_PROBE, &m, ix->ev[0], stream));
  int chosen = path != MRAG_IVF_FILTER_AUTO ? path : ivf_choose_filter_path(nq, s.nprobe, ix->nlist, n, m);
  if (!probe_fits) chosen = MRAG_IVF_FILTER_EXACT;
  if (chosen == MRAG_IVF_FILTER_EXACT && m < 0) {   // (forced P that cannot run as P, device allow-set: E needs the count)
    int hm = 0;
    MRAG_HIP(hipMemcpyAsync(&hm, ix->fw.fwork.p, sizeof(int), hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipStreamSynchronize(stream));
    m = hm;
  }
  MRAG_TRY(s.start(false));
  MRAG_TRY(ivf_grow_cev(ix, 1));
  int live = -2;
  if (chosen == MRAG_IVF_FILTER_EXACT || m == 0) {
    s.chunk = nq;                        // one chunk, whatever nq: its outputs, its queries, its scan events cev[0..1]
    IvfChunk e(s, 0);
    MRAG_TRY(e.stage_outputs());
    if (m == 0) {                      // nothing allowed: no search kernel
      MRAG_HIP(hipEventRecord(e.ev_scan0, stream));
      MRAG_TRY(launch_fill_empty(e.d_sc, e.d_id, nq * k, stream));
      MRAG_HIP(hipEventRecord(e.ev_scan1, stream));
    } else {
      // path E: the dense filtered search over the rows in arrival order (ix->raw: whole zeroed 256-row tiles), ids = row + id_base
      MRAG_TRY(e.prepare_queries());
      BfLaunch a = ivf_launch(ix, ix->raw, n, ix->qbuf.p, nq, stream);
      a.k = k; a.out_scores = e.d_sc; a.out_ids = e.d_id; a.id_base = ix->id_base;
      a.ev_k2_begin = e.ev_scan0; a.ev_k2_end = e.ev_scan1;
      MRAG_TRY(filter_search(ix->fw, a, filter_choose_path(nq, k, n, m, ix->ld), m, stream));
    }
    ix->n_chunks = 1;
    MRAG_TRY(e.copy_back());
    if (m == 0) live = 0;
  } else {
    // path P: allow-set -> stored positions + per-list counts; liveness from those counts or the caller's (sharded: global)
    MRAG_TRY(ivf_filter_stored(ix, stream));
    const int* cnt = flist_counts(ix);
    if (list_allowed && allow_is_device) {        // (list_allowed lives where the allow-set does)
      cnt = list_allowed;
    } else if (list_allowed) {
      if (!ix->ev_lallow) {
        MRAG_HIP(hipEventCreateWithFlags(&ix->ev_lallow, hipEventDisableTiming));
        MRAG_HIP(hipHostMalloc((void**)&ix->h_lallow, (size_t)ix->nlist * 4, hipHostMallocDefault));
      } else {
        MRAG_HIP(hipEventSynchronize(ix->ev_lallow));   // the previous copy out of the staging buffer is done
      }
      memcpy(ix->h_lallow, list_allowed, (size_t)ix->nlist * 4);
      MRAG_HIP(hipMemcpyAsync(flist_caller(ix), ix->h_lallow, (size_t)ix->nlist * 4, hipMemcpyHostToDevice, stream));
      MRAG_HIP(hipEventRecord(ix->ev_lallow, stream));
      cnt = flist_caller(ix);
    }
    MRAG_HIP(hipMemsetAsync(flist_nlive(ix), 0, 4, stream));
    hipLaunchKernelGGL(ivf_live_bits_kernel, dim3((unsigned)(bf_round_rows(ix->nlist) / 256)), dim3(256), 0, stream, cnt, ix->nlist,
                       flist_live(ix), flist_nlive(ix));
    MRAG_HIP(hipGetLastError());
    s.mode = IVF_FILTERED; s.live_bits = flist_live(ix); s.stored_bits = (const uint32_t*)ix->fstored.p;
    MRAG_TRY(s.run_chunks());
    // the figures last_filter reports, kept apart from the words the next call overwrites (no sync here)
    MRAG_TRY(ix->flast.ensure(8));
    MRAG_HIP(hipMemcpyAsync(ix->flast.p, ix->fw.fwork.p, 4, hipMemcpyDeviceToDevice, stream));
    MRAG_HIP(hipMemcpyAsync((int*)ix->flast.p + 1, flist_nlive(ix), 4, hipMemcpyDeviceToDevice, stream));
    live = -1;
  }
  MRAG_TRY(s.finish(!out_is_device || !queries_is_device));
  ix->last_fpath = chosen;
  ix->last_fallowed = m;
  ix->last_flive = live;
  return MRAG_OK;
}

int mrag_ivf_last_filter(mrag_handle h, int* out_path, int64_t* out_allowed, int* out_live_lists) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (ix->last_fpath < 0) return fail(MRAG_ERR_INVALID, "no completed filtered search on this index");
  MRAG_TRY(use_device(ix->device));
  if (ix->last_fallowed < 0 || ix->last_flive == -1) {   // path P: still on the device
    MRAG_HIP(hipEventSynchronize(ix->ev[3]));
    int h[2] = {0, 0};
    MRAG_HIP(hipMemcpy(h, ix->flast.p, 8, hipMemcpyDeviceToHost));
    if (ix->last_fallowed < 0) ix->last_fallowed = h[0];
    if (ix->last_flive == -1) ix->last_flive = h[1];
  }
  if (out_path) *out_path = ix->last_fpath;
  if (out_allowed) *out_allowed = ix->last_fallowed;
  if (out_live_lists) *out_live_lists = ix->last_flive;
  return MRAG_OK;
}

// ---- fp8 scan copy + exact re-rank (contract in include/mrag.h) ---------------------------------------------------
int mrag_ivf_enable_fp8(mrag_handle h) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (ix->metric != MRAG_METRIC_COSINE) return fail(MRAG_ERR_INVALID, "the fp8 scan copy serves cosine indexes only");
  if (ix->fp8) return MRAG_OK;
  MRAG_TRY(use_device(ix->device));
  ix->fp8 = true;
  if (ix->n > 0) {
    // rows already stored (adds and searches on any stream): settle them, build the copy on the null stream -- with the
    // regroup when that is due anyway --, finish it here (a one-off)
    int st = hipDeviceSynchronize() == hipSuccess ? MRAG_OK : fail(MRAG_ERR_HIP, "hipDeviceSynchronize failed");
    if (st == MRAG_OK) st = ix->dirty ? ivf_finalize(ix, nullptr) : ivf_build_sorted8(ix, nullptr);
    if (st == MRAG_OK && hipStreamSynchronize(nullptr) != hipSuccess) st = fail(MRAG_ERR_HIP, "building the fp8 rows failed");
    if (st != MRAG_OK) { ix->fp8 = false; return st; }
  }
  return MRAG_OK;
}

int mrag_ivf_get_rows_fp8(mrag_handle h, int64_t row0, int64_t n, uint8_t* out, int out_is_device, void* stream_) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (!ix->fp8) return fail(MRAG_ERR_INVALID, "no fp8 scan copy (mrag_ivf_enable_fp8)");
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
  hipLaunchKernelGGL(gather_rows8_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, (const uint8_t*)ix->sorted8, ix->ld8,
                     (const int64_t*)ix->inv_pos.p, row0, n, ix->dim, d_out);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && !out_is_device) e = hipMemcpyAsync(out, d_out, (size_t)tot, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess && !out_is_device) e = hipStreamSynchronize(stream);
  tmp.release();
  if (e != hipSuccess) return fail(MRAG_ERR_HIP, "reading the fp8 rows failed: %s", hipGetErrorString(e));
  ix->timed = false;
  return ivf_record_end(ix, stream);   // (inv_pos is in use on `stream` until here)
}

int mrag_ivf_search_fp8(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device, int nprobe,
                        int k, int refine, float* out_scores, int64_t* out_ids, int out_is_device, void* stream_) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (!ix->fp8) return fail(MRAG_ERR_INVALID, "no fp8 scan copy on this index (mrag_ivf_enable_fp8)");
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
  ix->last_refine = refine;
  return MRAG_OK;
}

int mrag_ivf_last_fp8(mrag_handle h, int* out_refine) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (ix->last_refine < 0) return fail(MRAG_ERR_INVALID, "no completed fp8 search on this index");
  if (out_refine) *out_refine = ix->last_refine;
  return MRAG_OK;
}

int mrag_ivf_last_timing(mrag_handle h, float* out_scan_ms, float* out_total_ms, int64_t* out_scanned_rows, int* out_n_wg) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (!ix->timed) return fail(MRAG_ERR_INVALID, "no completed search to time");
  MRAG_TRY(use_device(ix->device));
  MRAG_HIP(hipEventSynchronize(ix->ev[3]));
  // a search cut into chunks (score buffer cap) reports the SUM of its chunks' list-scan brackets, rows and workgroups
  float g = 0.f, t = 0.f;
  for (int c = 0; c < ix->n_chunks; ++c) {
    float gc = 0.f;
    MRAG_HIP(hipEventElapsedTime(&gc, ix->cev[2 * c], ix->cev[2 * c + 1]));
    g += gc;
  }
  MRAG_HIP(hipEventElapsedTime(&t, ix->ev[0], ix->ev[3]));
  if (out_scan_ms) *out_scan_ms = g;
  if (out_total_ms) *out_total_ms = t;
  unsigned long long st[2] = {0ull, 0ull};
  MRAG_HIP(hipMemcpy(st, ix->stats.p, 16, hipMemcpyDeviceToHost));   // (accumulated on the device by the plan kernels)
  if (out_n_wg) *out_n_wg = (int)st[1];
  if (out_scanned_rows) *out_scanned_rows = (int64_t)st[0];
  return MRAG_OK;
}

}  // extern "C"
