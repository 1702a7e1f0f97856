// The IVF search pipeline: the device-side regrouping of (query, probe) pairs by list, the IvfSearch call object and the
// seven stages of an IvfChunk (declared in ivf_index.h), mrag_ivf_search and mrag_ivf_last_timing.  IVF-flat runs over the
// dense index's fused similarity + top-k kernels (BASELINE.json config 5; the reference has no IVF index -- PARITY UNPINNED
// by the reference, checked against this library's own brute force and the oracle's ivf_search on identical centroids /
// assignments); the steps of a search are listed in ivf_build.hip.
#include "ivf_index.h"

namespace mrag {

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

int64_t ivf_scores_cap() {
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

int ivf_grow_cev(IvfIndex* ix, int n_chunks) {
  while ((int)ix->cev.size() < 2 * n_chunks) {
    Event e;
    MRAG_TRY(e.create(true));
    ix->cev.push_back(std::move(e));
  }
  return MRAG_OK;
}

int ivf_wait_previous(IvfIndex* ix, hipStream_t stream) {
  if (ix->end_recorded) MRAG_HIP(hipStreamWaitEvent(stream, ix->ev_end, 0));
  return MRAG_OK;
}
int ivf_record_end(IvfIndex* ix, hipStream_t stream) {
  MRAG_HIP(hipEventRecord(ix->ev_end, stream));
  ix->end_recorded = true;
  return MRAG_OK;
}

int IvfSearch::begin() {
  nprobe = std::min(nprobe, ix->nlist);
  // probe selection = top-nprobe over the centroids: the fused kernel up to 64, the streaming kernel up to 256
  // (8 queries per launch); nprobe == nlist needs no selection at all
  if (nprobe > bf_max_k_wide() && nprobe < ix->nlist)
    return fail(MRAG_ERR_UNSUPPORTED, "nprobe = %d: supported are 1..%d and nlist (= %d, exhaustive)", nprobe, bf_max_k_wide(), ix->nlist);
  if (nq == 0) return MRAG_OK;
  if (!queries || !out_scores || !out_ids || !dtype_size(q_dtype)) return fail(MRAG_ERR_INVALID, "bad buffer / dtype");
  if (!ix->has_centroids) return fail(MRAG_ERR_INVALID, "index has no centroids");
  MRAG_TRY(use_device(ix->device));
  MRAG_TRY(ivf_finalize(ix, stream));
  chunk = ivf_chunk_queries(ix, nq, nprobe);
  if (chunk > (1 << 20)) return fail(MRAG_ERR_UNSUPPORTED, "nq too large for one IVF batch (2^20); cut the query batch");
  ix->timed = false;
  return ivf_wait_previous(ix, stream);
}

int IvfSearch::refuse_fused() const {
  if (ivf_scores_cap() <= 0) return ivf_segments_only(what(), "the score buffer is disabled (MRAG_IVF_SCORES_MB = 0)");
  if (nprobe > 256) return ivf_segments_only(what(), "more than 256 probed lists per query (exhaustive probing with nlist > 256)");
  return MRAG_OK;
}

int IvfSearch::start(bool record_begin) {
  if (record_begin) MRAG_HIP(hipEventRecord(ix->ev_begin, stream));
  MRAG_TRY(ix->stats.ensure(16));
  MRAG_HIP(hipMemsetAsync(ix->stats.p, 0, 16, stream));
  return MRAG_OK;
}

int IvfSearch::finish(bool host_buffer_involved) {
  MRAG_TRY(ivf_record_end(ix, stream));
  ix->timed = true;
  if (host_buffer_involved) MRAG_HIP(hipStreamSynchronize(stream));
  return MRAG_OK;
}

int IvfSearch::run_chunks() {
  const int n_chunks = (int)((nq + chunk - 1) / chunk);
  MRAG_TRY(ivf_grow_cev(ix, n_chunks));
  for (int c = 0; c < n_chunks; ++c) MRAG_TRY(IvfChunk(*this, c).run());
  ix->n_chunks = n_chunks;
  return MRAG_OK;
}

int IvfChunk::stage_outputs() {
  d_sc = s.out_scores + (size_t)off * s.k; d_id = s.out_ids + (size_t)off * s.k;
  if (rg) d_cnt = s.out_counts + off;
  if (s.out_is_device) return MRAG_OK;
  MRAG_TRY(ix->out_sc.ensure((size_t)nq * s.k * 4));
  MRAG_TRY(ix->out_id.ensure((size_t)nq * s.k * 8));
  d_sc = (float*)ix->out_sc.p; d_id = (int64_t*)ix->out_id.p;
  if (rg) { MRAG_TRY(ix->range.out_cnt.ensure((size_t)nq * 8)); d_cnt = (int64_t*)ix->range.out_cnt.p; }
  return MRAG_OK;
}

int IvfChunk::prepare_queries() {
  const int64_t nq_pad = bf_query_rows(nq);
  const size_t row = (size_t)ix->ld * 2;
  MRAG_TRY(ix->qbuf.ensure((size_t)nq_pad * row));
  MRAG_HIP(hipMemsetAsync((char*)ix->qbuf.p + (size_t)nq * row, 0, (size_t)(nq_pad - nq) * row, stream));
  if (rg && s.stored_rows)
    MRAG_HIP(hipMemcpyAsync(ix->qbuf.p, (const char*)s.queries + (size_t)off * row, (size_t)nq * row, hipMemcpyDeviceToDevice, stream));
  else
    MRAG_TRY(ivf_prepare(ix, {(const char*)s.queries + (size_t)off * ix->dim * dtype_size(s.q_dtype), nq, s.q_dtype, s.normalize, s.queries_is_device},
                         (uint16_t*)ix->qbuf.p, stream));
  if (!f8) return MRAG_OK;
  MRAG_TRY(ix->f8.qbuf8.ensure((size_t)nq_pad * ix->f8.ld8));
  MRAG_TRY(launch_quant_queries_fp8((const uint16_t*)ix->qbuf.p, ix->ld, ix->dtype == MRAG_BF16 ? 1 : 0, nq_pad, (uint8_t*)ix->f8.qbuf8.p,
                                    ix->f8.ld8, stream));
  return ix->f8.cand.ensure((size_t)nq * s.refine * 8);
}

int IvfChunk::select_probes() {
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

int IvfChunk::plan() {
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

int IvfChunk::scan_scores() {
  hipLaunchKernelGGL(ivf_scatter_kernel, dim3(pgrid()), dim3(256), 0, stream, (const int64_t*)ix->tmp_id.p, (int64_t)npairs, s.nprobe,
                     (const int*)ix->d_list_count.p, (const int*)d_wg_first, d_cursor, (int64_t*)ix->gq.p, nullptr, 7,
                     (const long long*)d_foff, (const int*)ix->d_list_tile_lo.p, (int4*)ix->ploc.p, (const int*)d_lcount,
                     (const int*)d_dfirst, (int*)ix->desc.p, (int)desc_bound);
  MRAG_HIP(hipGetLastError());
  MRAG_HIP(hipEventRecord(ev_scan0, stream));
  // (no_sync: the descriptor count stays on the device, the grid is its bound)
  MRAG_TRY(ivfs_scan(f8 ? (const uint16_t*)ix->f8.sorted8.p : (const uint16_t*)ix->sorted, (const uint16_t*)(f8 ? ix->f8.qbuf8.p : ix->qbuf.p),
                     f8 ? ix->f8.ld8 / 2 : ix->ld, f8 ? MRAG_DT_FP8 : ix->dtype, nq, (const int*)ix->desc.p,
                     no_sync ? (int)desc_bound : n_desc, no_sync ? d_nwg : nullptr, (const int64_t*)ix->gq.p, (float*)ix->scores.p,
                     stream));
  IvfsRange sel_range{s.floor, s.excl_pos ? s.excl_pos + off : nullptr, d_cnt};
  if (f8)   // candidates: local rows in (fp8 score desc, row asc) order, -1 past the rows of the probed lists
    MRAG_TRY(ivfs_select_lists((const float*)ix->scores.p, ix->ploc.p, s.nprobe, nq, s.refine, ix->row_ids, 0, nullptr, (int64_t*)ix->f8.cand.p, stream));
  else
    MRAG_TRY(ivfs_select_lists((const float*)ix->scores.p, ix->ploc.p, s.nprobe, nq, s.k, ix->row_ids, ix->id_base, d_sc, d_id, stream,
                               s.stored_bits, rg ? &sel_range : nullptr));
  MRAG_HIP(hipEventRecord(ev_scan1, stream));
  if (f8)
    MRAG_TRY(launch_fp8_rerank(ix->raw, (const uint16_t*)ix->qbuf.p, ix->ld, ix->dtype == MRAG_BF16 ? 1 : 0, (const int64_t*)ix->f8.cand.p, nq,
                               s.refine, s.k, ix->id_base, d_sc, d_id, stream));
  return MRAG_OK;
}

int IvfChunk::scan_fused() {
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
    MRAG_TRY(ivf_gather_rows((const uint16_t*)ix->qbuf.p, (const int64_t*)ix->gq.p, (int64_t)n_wg * 256, ix->ld, (uint16_t*)ix->qg.p, 0, stream));
  }
  BfLaunch a = ivf_launch(ix, ix->sorted, 0, ix->qg.p, nq, stream);
  a.k = s.k; a.out_scores = d_sc; a.out_ids = d_id; a.id_base = ix->id_base;
  static const int dummy_desc = 0;
  a.wg_desc = n_wg ? (const int*)ix->desc.p : &dummy_desc; a.n_wg = n_wg;
  a.pair_loc = ix->ploc.p; a.nprobe = s.nprobe; a.row_ids = ix->row_ids;
  a.ev_k2_begin = ev_scan0; a.ev_k2_end = ev_scan1;
  return bf_launch(a);
}

int IvfChunk::copy_back() const {
  if (s.out_is_device) return MRAG_OK;
  if (rg) MRAG_HIP(hipMemcpyAsync(s.out_counts + off, d_cnt, (size_t)nq * 8, hipMemcpyDeviceToHost, stream));
  MRAG_HIP(hipMemcpyAsync(s.out_scores + (size_t)off * s.k, d_sc, (size_t)nq * s.k * 4, hipMemcpyDeviceToHost, stream));
  MRAG_HIP(hipMemcpyAsync(s.out_ids + (size_t)off * s.k, d_id, (size_t)nq * s.k * 8, hipMemcpyDeviceToHost, stream));
  return MRAG_OK;
}

int IvfChunk::run() {
  MRAG_TRY(stage_outputs());
  MRAG_TRY(prepare_queries());
  MRAG_TRY(select_probes());
  MRAG_TRY(plan());
  MRAG_TRY(use_scores ? scan_scores() : scan_fused());
  return copy_back();
}

}  // namespace mrag

using namespace mrag;

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

int mrag_ivf_last_timing(mrag_handle h, float* out_scan_ms, float* out_total_ms, int64_t* out_scanned_rows, int* out_n_wg) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (!ix->timed) return fail(MRAG_ERR_INVALID, "no completed search to time");
  MRAG_TRY(use_device(ix->device));
  MRAG_HIP(hipEventSynchronize(ix->ev_end));
  // a search cut into chunks (score buffer cap) reports the SUM of its chunks' list-scan brackets, rows and workgroups
  float g = 0.f, t = 0.f;
  for (int c = 0; c < ix->n_chunks; ++c) {
    float gc = 0.f;
    MRAG_HIP(hipEventElapsedTime(&gc, ix->cev[2 * c], ix->cev[2 * c + 1]));
    g += gc;
  }
  MRAG_HIP(hipEventElapsedTime(&t, ix->ev_begin, ix->ev_end));
  if (out_scan_ms) *out_scan_ms = g;
  if (out_total_ms) *out_total_ms = t;
  unsigned long long st[2] = {0ull, 0ull};
  MRAG_HIP(hipMemcpy(st, ix->stats.p, 16, hipMemcpyDeviceToHost));   // (accumulated on the device by the plan kernels)
  if (out_n_wg) *out_n_wg = (int)st[1];
  if (out_scanned_rows) *out_scanned_rows = (int64_t)st[0];
  return MRAG_OK;
}

}  // extern "C"
