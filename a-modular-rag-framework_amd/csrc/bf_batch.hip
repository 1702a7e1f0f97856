// Brute-force cosine / inner-product top-k over an HBM-resident fp16/bf16 corpus.
//
// Replaces, at corpus scale, the reference's "cosine every candidate, sort descending,
// truncate" (app/modules/retrieval/retrieval_backend.py:192-197,245,371-372).
//
//   K1  prep_rows_kernel (common.hip)  normalise + round queries/rows to storage type
//   K2  bf_gemm_topk_kernel            S = C . Q^T on MFMA 16x16x32 with the top-k filter
//                                      fused into the epilogue; the score matrix never
//                                      reaches HBM
//   K4  bf_merge_kernel                per query: select the k best of the candidates the
//                                      K2 workgroups kept, order (score desc, row asc)
//
// K2 geometry (MI355X: 256 CUs, 160 KiB LDS, 8 XCDs x 4 MiB L2)
//   workgroup = 512 threads = 8 waves, tile = 256 corpus rows x 256 queries, K step 64.
//   wave (wm, wn) owns 128 corpus rows x 64 queries = 8 x 4 MFMA 16x16 accumulators.
//   The CORPUS is the MFMA A operand, so an accumulator column (lane & 15) is ONE query:
//   a lane needs only 4 running thresholds in registers to filter its 128 scores.
//   LDS: 2 stages x (32 KiB corpus + 32 KiB query) filled by global_load_lds (16 B/lane),
//   rows of 128 B XOR-swizzled on the 16-B chunk index by (row>>1)&7 so every
//   ds_read_b128 lane group touches 16 distinct slots of the 256-B bank row.  The swizzle
//   is applied to the per-lane SOURCE address (LDS-DMA writes lane-linear).
//   A workgroup = (query tile t, corpus split s): it walks the tiles of its split with the
//   running per-query candidate lists (global memory, L2 resident) and thresholds (LDS).
//   One wave of workgroups: S = floor(CUs / T) splits per query tile (T <= 64 per launch); blocks go
//   to XCDs round-robin, so XCD x gets a contiguous run of the tile-major (t, s) order -- at T = 40
//   five query tiles (1.9 MiB, L2-resident across corpus tiles) x all six corpus streams, each
//   shared by those tiles' workgroups.
//
// Top-k filter (exact)
//   Per query a threshold thr certified by ">= k EARLIER rows score >= thr"; a score is listed
//   only if it beats thr (strict: a later row that ties loses the (score desc, row asc)
//   tie-break).  Certificates: (a) k <= 16: every lane tracks the two largest per-tile maxima it
//   has seen for each of its 4 query columns; the minimum over the 8 lanes that share a query
//   (2 waves x 4 lane groups) of their 2nd-largest is a score that >= 16 earlier rows reach
//   (LDS ds_min, double-buffered per tile); the first tile bootstraps from its own scores and
//   passes on '>='.  (b) any k: the k-th best of a compacted list.
//   (c) k < 16: after tiles 0-7, 15, 31, 63, ... of a split the k-th LARGEST of the 16 certified maxima
//   replaces their minimum (one thread per query, bitonic network in registers): ~2x fewer listings.
//   (d) 16 < k <= 64: no row-count certificate; every query is compacted after tiles 0, 1, 3, 7, ...
//   Lists: each of the 8 lanes that share a query owns a private 64-entry segment of the
//   query's list (count kept in a register during the push, committed to LDS after the tile's
//   barrier): a push is a compare and one predicated 8-byte store, no atomics, no waits.
//   A full segment raises a flag: the tile is replayed in 4 sub-rounds (<= 8 pushes per
//   segment each) with the affected queries compacted in between.  Compaction = one wave per
//   query: keys staged in LDS, MSB-first radix select of the k-th key (skipped when <= 64 keys are
//   staged), rank by counting among the selected, sorted write-back into a 64-entry "kept" area,
//   segments emptied, thr raised to the k-th.  Adversarial inputs (every tile beats the last) take
//   the replay path every tile: slower, never wrong.
//
// Main loop
//   One barrier per K step.  The next stage's 8 LDS-DMA loads per wave are issued (inline asm, scalar
//   base + 32-bit voffset) at the top of a step; fragment reads are software-pipelined over two
//   register sets (the MFMAs of k-half 1 of the previous step run while the reads of this step's
//   half 0 land); the first K step of a tile uses a zero C operand instead of cleared accumulators.
//
// This file: K2 with its compaction helpers, its instance table and launcher.  K2s is in bf_stream.hip, the merges in
// bf_merge.hip, the launch logic in bf_index.hip.
#include "bf_kernels.h"

namespace mrag {

constexpr int STAGE_BYTES = (TM + TQ) * BK * 2; // 64 KiB
constexpr int GEMM_LDS = 2 * STAGE_BYTES;       // 128 KiB
constexpr int DENSE_TILES = 8;            // tiles of a split filtered by the mask + LDS path (see the epilogue)
constexpr int K_CERT = 16;                // k served by the 16-row threshold certificate

constexpr int OFF_TAU = GEMM_LDS;               // float[256]      k-th best after a compaction
constexpr int OFF_KCNT = OFF_TAU + 1024;        // int[256]        kept entries
constexpr int OFF_SCNT = OFF_KCNT + 1024;       // int[256][8]     committed segment counts
constexpr int OFF_STAT = OFF_SCNT + 8192;       // uint[2][256]    certificates, orderable bits
constexpr int OFF_FLAGS = OFF_STAT + 2048;      // int[4]
constexpr int OFF_RM = OFF_FLAGS + 16;          // float[4 columns][2][512 threads]: each lane's two largest
                                                // per-tile maxima per query column (kept out of the VGPR budget)
constexpr int LDS_TOTAL = OFF_RM + 4 * 2 * NTHR * 4;
constexpr int OFF_RCNT = LDS_TOTAL;             // RANGE instances: int[256] rows >= the floor per query of this split
constexpr int LDS_TOTAL_RANGE = OFF_RCNT + 1024;

// Cache policy of the LDS-DMA stage loads (written into their asm string), measured on one box: the five workgroups of an
// XCD that share a corpus stream rely on each other's lines staying in L2 for a moment -- nt on the corpus loads made the
// kernel 13 % SLOWER (13.5 -> 15.2 ms at 10 k x 1M); the query chunks are re-read for every corpus tile (L2-resident).
// Both operands: default policy.  (The streaming kernel reads every corpus byte once and does use nt: bf_stream.hip.)

// K walk of the batch kernel: every corpus tile walks its K steps first-to-last.  Walking the K steps of every other tile
// last-to-first (so that the query K slices a workgroup has just used are the ones it asks for next: the VERDICT r2 #1a
// experiment) was measured round 3, same box, interleaved (tools/ab.sh): 10 000 x 1 M x 768 13.83 / 13.88 / 13.90 ms
// forward vs 14.05 / 14.01 / 14.02 (by global parity) and 14.02 / 14.06 / 14.02 (by split parity): 1.2 % SLOWER;
// 1 000 x 1 M 1.593-1.600 vs 1.593-1.613; C2 unchanged.  It also made a row's fp32 accumulation order depend on its tile
// parity (sharded != unsharded in the last bit).  Not taken.

// One wave compacts query q: the k best of its kept area + 8 segments go (sorted, best first)
// into the kept area, the segments are emptied, tau_c rises to the k-th.  The keys are staged
// through `scratch` (>= QCAP u64 of LDS: the stage buffer the K loop has just consumed), then
// ranked by counting with broadcast LDS reads.  Register-light on purpose (it shares the
// kernel's 256-VGPR budget with the 128 accumulators); slow, and rare by construction.

// Select the k best of the `total` unique keys staged in `scratch` (one wave) and write them, sorted
// best first, into the query's kept area; tau_c rises to the k-th.  MSB-first radix select, 8 bits
// per pass over an LDS histogram: each pass narrows the bucket that holds the k-th key; it stops as
// soon as that bucket is needed whole (typically after 3-5 passes).  The <= 64 selected keys are
// then ranked by counting.  ~600 instructions whatever `total` is (rank-by-counting over all the
// entries was ~20 000 at 576 entries, which made k > 16 -- no row-count certificate, thresholds
// driven by compaction alone -- 3-5x slower than k <= 16).
// scratch layout (8 KiB per wave): keys[QCAP] u64 | hist[256] u32 | sel[KMAX] u64
template <bool WIDE = false>   // WIDE: eight candidate reads in flight in the ranking loop (16 more VGPRs: end-of-split tail only)
__device__ __forceinline__ void rank_and_keep(uint2* __restrict__ lst, int q, int k, int lane,
                                              uint64_t* __restrict__ scratch, int total) {
  float* tau_c = (float*)(smem + OFF_TAU);
  int* kcnt = (int*)(smem + OFF_KCNT);
  int* scnt = (int*)(smem + OFF_SCNT);
  uint32_t* hist = (uint32_t*)(scratch + QCAP);
  uint64_t* sel = scratch + QCAP + 128;
  int shift = 0;               // keys with (key >> shift) >= prefix are selected once the loop ends
  uint64_t prefix = 0ull;
  // <= 64 staged keys (the usual case at the end of a split, after pruning): one key per lane, ranked
  // directly below -- no selection pass at all
  if (total > 64) {
    int need = k;
    for (shift = 56; shift >= 0; shift -= 8) {
      *(uint4*)&hist[lane * 4] = make_uint4(0u, 0u, 0u, 0u);
      __builtin_amdgcn_wave_barrier();
      for (int i = lane; i < total; i += 64) {
        const uint64_t key = scratch[i];
        const bool active = shift == 56 || (key >> (shift + 8)) == prefix;
        if (active) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
      }
      __builtin_amdgcn_wave_barrier();
      const uint4 h = *(const uint4*)&hist[lane * 4];      // bins 4*lane .. 4*lane+3
      const int mine = (int)(h.x + h.y + h.z + h.w);
      int suf = mine;                                       // inclusive suffix sum over lanes >= this one
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_down(suf, off);
        if (lane + off < 64) suf += v;
      }
      int cum = suf - mine;                                 // keys in bins above this lane's
      int found = -1, above = 0, inb = 0;
      const int hb[4] = {(int)h.x, (int)h.y, (int)h.z, (int)h.w};
#pragma unroll
      for (int b = 3; b >= 0; --b) {
        if (found < 0 && cum < need && cum + hb[b] >= need) { found = lane * 4 + b; above = cum; inb = hb[b]; }
        cum += hb[b];
      }
      const unsigned long long who = __ballot(found >= 0);
      const int src = __builtin_ctzll(who);
      const int digit = __shfl(found, src);
      above = __shfl(above, src);
      inb = __shfl(inb, src);
      need -= above;
      prefix = (prefix << 8) | (uint64_t)digit;
      if (inb == need) break;                               // the whole bucket is selected
    }
    if (shift < 0) shift = 0;
  }
  int nsel = total;
  const uint64_t* cand = scratch;
  if (total > 64) {
    // gather the selected keys (exactly k of them)
    nsel = 0;
    for (int base = 0; base < total; base += 64) {
      const int i = base + lane;
      const uint64_t key = i < total ? scratch[i] : 0ull;
      const bool pick = i < total && (key >> shift) >= prefix;
      const unsigned long long bal = __ballot(pick);
      if (pick) sel[nsel + __popcll(bal & ((1ull << lane) - 1ull))] = key;
      nsel += __popcll(bal);
    }
    cand = sel;
  }
  __builtin_amdgcn_wave_barrier();
  const uint64_t my = lane < nsel ? cand[lane] : 0ull;
  int rank = 0;
  // eight broadcast reads in flight per step (one at a time, every step waits out an LDS round trip);
  // slots past nsel hold stale keys: masked by the index test
  if constexpr (WIDE) {
    for (int j0 = 0; j0 < nsel; j0 += 8) {
      uint64_t c8[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) c8[t] = cand[(j0 + t) & 63];
#pragma unroll
      for (int t = 0; t < 8; ++t) rank += (j0 + t < nsel && c8[t] > my) ? 1 : 0;
    }
  } else {
    for (int j = 0; j < nsel; ++j) rank += (cand[j] > my) ? 1 : 0;
  }
  if (lane < nsel && rank < k) {
    const uint32_t sb = __float_as_uint(ord_f32((uint32_t)(my >> 32)));
    lst[rank] = make_uint2(sb, 0xFFFFFFFFu - (uint32_t)my);
    if (rank == k - 1) tau_c[q] = __uint_as_float(sb);
  }
  if (lane == 0) kcnt[q] = min(nsel, k);
  if (lane < NGRP) scnt[q * NGRP + lane] = 0;
}

// End of the split: cut the lists of queries q0..q0+3 to their k best.  A query's entries sit in up to
// nine places (kept area + 8 segments, 576 slots) but number only a few dozen, so they are enumerated
// DENSELY: entry e of query q lives in the place whose running count covers e.  One 8-byte load per lane
// fetches the first 64 entries of a query (usually all of them); the loads of the four queries are issued
// before any is used (the accumulators are dead here); entries below the query's final certified
// threshold are dropped before ranking.  (Walking all nine 64-slot chunks per query made this tail 15 % of
// the kernel at 125 k rows per GPU.)
__device__ __forceinline__ int tail_slot(const int (&pre)[NGRP + 1], int e) {
  // pre[0] = kept entries, pre[g+1] = pre[g] + entries of segment g; e < pre[NGRP]
  int idx = e;                                    // inside the kept area
#pragma unroll
  for (int g = 0; g < NGRP; ++g)
    if (e >= pre[g]) idx = KEPT + g * SEG + (e - pre[g]);
  return idx;
}

// NB queries per call.  Phase A (unrolled, small): one load per query into registers, then parked in
// LDS (`park`, NB x 64 entries).  Phase B (a run-time loop, so the selection code exists once): prune,
// stage keys, rank.  `scratch` = the 8-KiB rank_and_keep work area of this wave.
template <int NB, bool WIDE = false>
__device__ __forceinline__ void tail_compact(uint2* __restrict__ wg_list, int q0, int k, int lane,
                                             uint64_t* __restrict__ scratch, uint2* __restrict__ park, const float* thr_lds) {
  const int* kcnt = (const int*)(smem + OFF_KCNT);
  const int* scnt = (const int*)(smem + OFF_SCNT);
  {
    uint2 first[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int q = q0 + u;
      int pre[NGRP + 1];
      pre[0] = kcnt[q];
#pragma unroll
      for (int g = 0; g < NGRP; ++g) pre[g + 1] = pre[g] + min(scnt[q * NGRP + g], SEG);
      first[u] = make_uint2(0u, 0u);
      if (lane < pre[NGRP]) first[u] = wg_list[(size_t)q * QCAP + tail_slot(pre, lane)];
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) park[u * 64 + lane] = first[u];
  }
#pragma unroll 1
  for (int u = 0; u < NB; ++u) {
    const int q = q0 + u;
    const uint2* lst = wg_list + (size_t)q * QCAP;
    int pre_u[NGRP + 1];
    pre_u[0] = kcnt[q];
#pragma unroll
    for (int g = 0; g < NGRP; ++g) pre_u[g + 1] = pre_u[g] + min(scnt[q * NGRP + g], SEG);
    const int n_ent = pre_u[NGRP];
    if (n_ent == 0) continue;   // nothing listed (padding query of a partial tile / IVF group): counts are already zero
    const float th = thr_lds[q];
    int total = 0;
    {   // entries 0..63: parked in LDS by phase A.  (Kept apart from the global loads below: merged into one
        // loop hipcc selects between the two POINTERS and issues a flat load, whose wait also covers the
        // previous query's stores -- 2 000 cycles per query.)
      const uint2 en = park[u * 64 + lane];
      const bool valid = lane < n_ent && __uint_as_float(en.x) >= th;
      const unsigned long long bal = __ballot(valid);
      if (valid) scratch[__popcll(bal & ((1ull << lane) - 1ull))] = make_key(en.x, en.y);
      total = __popcll(bal);
    }
    for (int base = 64; base < n_ent; base += 64) {
      const int e = base + lane;
      uint2 en = make_uint2(0u, 0u);
      if (e < n_ent) en = lst[tail_slot(pre_u, e)];
      const bool valid = e < n_ent && __uint_as_float(en.x) >= th;
      const unsigned long long bal = __ballot(valid);
      if (valid) scratch[total + __popcll(bal & ((1ull << lane) - 1ull))] = make_key(en.x, en.y);
      total += __popcll(bal);
    }
    rank_and_keep<WIDE>(wg_list + (size_t)q * QCAP, q, k, lane, scratch, total);
  }
}

__device__ __forceinline__ void compact_query(uint2* __restrict__ lst, int q, int k,
                                              int lane, uint64_t* __restrict__ scratch, float keep_thr) {
  // replay-path compaction of ONE query (register-light: the 128 accumulators are live here)
  int* kcnt = (int*)(smem + OFF_KCNT);
  int* scnt = (int*)(smem + OFF_SCNT);
  const int kc = kcnt[q];
  int total = 0;
  {
#pragma unroll 1
    for (int r = 0; r < QCAP / 64; ++r) {
      const int idx = r * 64 + lane;
      bool valid;
      if (idx < KEPT) valid = idx < kc;
      else valid = ((idx - KEPT) & (SEG - 1)) < min(scnt[q * NGRP + ((idx - KEPT) / SEG)], SEG);
      uint64_t key = 0ull;
      if (valid) {
        const uint2 e = lst[idx];
        valid = __uint_as_float(e.x) >= keep_thr;       // entries below a certified threshold cannot be in the top k
        if (valid) key = make_key(e.x, e.y);            // never 0 for a valid entry (row < 2^31)
      }
      const unsigned long long bal = __ballot(valid);
      if (valid) scratch[total + __popcll(bal & ((1ull << lane) - 1ull))] = key;
      total += __popcll(bal);
    }
  }
  // (one wave: program order + the LDS queue order make the staged keys visible to every lane)
  rank_and_keep(lst, q, k, lane, scratch, total);
}

// Owner wave w (queries 32w .. 32w+31) compacts every query that has a segment above `limit`.
template <int QPW>
__device__ __forceinline__ void compact_owned(uint2* __restrict__ wg_list, int w, int lane, int k, int limit,
                                              uint64_t* __restrict__ scratch) {
  const int* scnt = (const int*)(smem + OFF_SCNT);
  const int q = w * QPW + (lane & (QPW - 1));
  bool need = false;
  if (lane < QPW) {
#pragma unroll
    for (int g = 0; g < NGRP; ++g) need |= scnt[q * NGRP + g] > limit;
  }
  unsigned long long m = __ballot(need);
  while (m) {
    const int b = __builtin_ctzll(m);
    m &= m - 1;
    const int qq = w * QPW + b;
    compact_query(wg_list + (size_t)qq * QCAP, qq, k, lane, scratch, -INFINITY);
  }
}

// NF = 16-query column groups per wave: 4 -> 8 waves (2 x 4) of 128 x 64, two per SIMD, 256 VGPRs each;
//                                        8 -> 4 waves (2 x 2) of 128 x 128, ONE per SIMD, 512 VGPRs each
// DESC: descriptor mode (IVF list scan) -- its block decoding and its partial-query-tile loads exist only in that
// instance, the dense (t, s) instance carries neither.
// FILT: filtered search (path M, dense instances only): rows whose bit in p.allow is clear score -inf in the epilogue,
// exactly like the rows past the corpus in a partial last tile, so they are never listed and the certificates stay sound.
// RANGE: range search (dense instances only): every threshold starts at next_below(p.floor) and only rises from there, so
// only rows >= the floor are listed; the rows >= floor of each query are counted once per tile (before the push, so a
// replayed tile is not counted twice) into LDS and written to the workgroup's count slots at the end of the split.
template <int DT, int NF, bool DESC, bool FILT = false, bool RANGE = false>
__global__ __launch_bounds__(64 * 2 * (16 / NF), NF == 4 ? 2 : 1) void bf_gemm_topk_kernel(BfParams p) {
  static_assert(!(FILT && DESC), "filtered search runs the dense instance only");
  static_assert(!(RANGE && DESC), "range search runs the dense instance only");
  constexpr int WN = 16 / NF;            // waves along the query dimension
  constexpr int NW = 2 * WN;             // waves per workgroup
  constexpr int NT = 64 * NW;            // threads per workgroup
  constexpr int CPW = 32 / NW;           // 1-KiB DMA chunks per wave per operand and stage
  constexpr int QPW = TQ / NW;           // queries whose lists a wave owns (compaction)
  typedef typename Mfma<DT>::frag frag;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w / WN, wn = w % WN;
  // held clock = d(s_memtime) / d(s_memrealtime) x 100 MHz over workgroup 0's lifetime (MI355X_MICROARCH.md, DVFS
  // item 6): two stamps at entry, two at exit, written by one lane to a buffer nothing else reads; p.clock is
  // NULL unless the caller asked for the reading (bench.py's "held_clock_ghz")
  if (!DESC && p.clock && blockIdx.x == 0 && tid == 0) {
    p.clock[0] = (long long)__builtin_amdgcn_s_memtime();
    p.clock[1] = (long long)__builtin_amdgcn_s_memrealtime();
  }

  // ---- block -> (query tile, corpus tile range) ----------------------------------------------
  int wg, q_row0, nq_local, tile_lo, tile_hi, rows_end;
  if (DESC) {
    // descriptor mode: one workgroup = one IVF list x up to 256 of the queries that probe it
    const int* d = p.wg_desc + (size_t)blockIdx.x * 8;
    wg = blockIdx.x;
    q_row0 = d[0]; nq_local = d[1]; tile_lo = d[2]; tile_hi = d[3]; rows_end = d[4];
  } else {
    int t, s;
    const int b = blockIdx.x;
    if (p.xcd_map) {
      // XCD-aware: blocks go to XCDs round-robin (b & 7); give each XCD a CONTIGUOUS run of the tile-major
      // (t, s) order: an XCD then works on grid/8/S query tiles (5 at T = 40: 1.9 MB of queries, L2-resident
      // across corpus tiles) against all S corpus streams, each shared by those query tiles' workgroups
      const int per = (int)gridDim.x >> 3;
      const int lin = (b & 7) * per + (b >> 3);
      t = lin / p.S;
      s = lin - t * p.S;
    } else {
      s = b % p.S;
      t = b / p.S;
    }
    wg = t * p.S + s;
    q_row0 = t * TQ;
    nq_local = p.nq - q_row0;
    tile_lo = (int)(((long long)s * p.n_ctiles) / p.S);
    tile_hi = (int)(((long long)(s + 1) * p.n_ctiles) / p.S);
    rows_end = p.n_rows;
  }
  uint2* wg_list = p.list + (size_t)wg * TQ * QCAP;
  const int ksteps = p.ksteps;

  float* tau_c = (float*)(smem + OFF_TAU);
  int* kcnt = (int*)(smem + OFF_KCNT);
  int* scnt = (int*)(smem + OFF_SCNT);
  uint32_t* stat = (uint32_t*)(smem + OFF_STAT);   // [2][256] orderable bits, ds_min target
  int* flags = (int*)(smem + OFF_FLAGS);
  uint32_t* rm = (uint32_t*)(smem + OFF_RM);
  int* rcnt = (int*)(smem + OFF_RCNT);   // RANGE only (inside LDS_TOTAL_RANGE)
  const float fnb = RANGE ? next_below(p.floor) : -INFINITY;   // RANGE: a score is listed / counted iff it beats fnb
  if (tid < TQ) {
    tau_c[tid] = fnb;
    if constexpr (RANGE) rcnt[tid] = 0;
    kcnt[tid] = 0;
    stat[tid] = 0xFFFFFFFFu;
    stat[TQ + tid] = 0xFFFFFFFFu;
  }
  for (int i = tid; i < TQ * NGRP; i += NT) scnt[i] = 0;
  if (tid == 0) flags[0] = 0;

  // ---- LDS-DMA source offsets: wave w fills 1-KiB chunks 4w..4w+3 of each operand ---------
  // chunk c = 8 rows x 128 B; lane l -> row r = 8c + (l>>3), physical 16-B chunk l&7,
  // logical chunk (l&7) ^ ((r>>1)&7) = (l&7) ^ ((4c + (l>>4)) & 7).  Chunks c and c+2 share the
  // per-lane part, so ONE 32-bit voffset per chunk parity is enough; the chunk's row block goes
  // into the scalar base (scalar-base + 32-bit-voffset form, no 64-bit per-lane addresses).
  const uint32_t row_b = (uint32_t)p.ld * 2u;                       // bytes per row
  const uint32_t voff_e = (uint32_t)(lane >> 3) * row_b + (uint32_t)(((lane & 7) ^ (lane >> 4)) * 16);        // even chunks
  const uint32_t voff_o = (uint32_t)(lane >> 3) * row_b + (uint32_t)(((lane & 7) ^ (4 + (lane >> 4))) * 16);  // odd chunks
  const char* q_ptr = (const char*)(p.queries + (size_t)q_row0 * p.ld) + (size_t)(CPW * w) * 8 * row_b;
  const size_t tile_bytes = (size_t)TM * p.ld * 2;
  const uint32_t chunk_b = 8u * row_b;                               // 8 rows

  // One stage = 2*CPW LDS-DMA loads per wave (CPW corpus chunks, CPW query chunks), issued from inline
  // asm two at a time.  hipcc does not count them: every wait for them is an explicit s_waitcnt vmcnt
  // below.  M0 (LDS destination base) is written inside the statement that uses it and restored after.
  constexpr int NPART = CPW;   // two chunks per part, two operands
  auto stage_part = [&](const char* a, const char* b, int buf, int part) {   // first half of the parts: corpus chunks; second half: query chunks
    const int op = part / (NPART / 2), i = (part % (NPART / 2)) * 2;
    if (op == 1 && (CPW * w + i) * 8 >= nq_local && DESC) return;
    const char* base = op ? b : a;
    const uint32_t la = (uint32_t)(buf * STAGE_BYTES + op * A_BYTES + (CPW * w + i) * 1024);   // wave-uniform
    const char* c0 = base + (size_t)i * chunk_b;
    const char* c1 = c0 + chunk_b;
    uint32_t keep;
    // Both operands use the default cache policy (see the top of the file) and the two statements are the same text.  They
    // stay two: written as one (inline, or in a helper), hipcc orders the scalar address arithmetic around the loads
    // differently in every instance of the kernel, and this kernel's code is pinned by comparison with its measured build.
    if (op == 0) {   // corpus chunks: streamed once per workgroup (cache policy: default, see the top of the file)
      asm volatile(
          "s_mov_b32 %0, m0\n\t"
          "s_mov_b32 m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\t"
          "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %4\n\t"
          "s_mov_b32 m0, %0"
          : "=&s"(keep)
          : "v"(voff_e), "v"(voff_o), "s"(c0), "s"(c1), "s"(la)
          : "memory", "scc");
    } else {         // query chunks: re-read for every corpus tile, default policy (L2-resident)
      asm volatile(
          "s_mov_b32 %0, m0\n\t"
          "s_mov_b32 m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\t"
          "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %4\n\t"
          "s_mov_b32 m0, %0"
          : "=&s"(keep)
          : "v"(voff_e), "v"(voff_o), "s"(c0), "s"(c1), "s"(la)
          : "memory", "scc");
    }
  };
  auto stage = [&](const char* a, const char* b, int buf) {
    static_assert(CPW == 4 || CPW == 8, "stage_part covers 4 or 8 chunks per operand and wave");
#pragma unroll
    for (int part = 0; part < NPART; ++part) stage_part(a, b, buf, part);
  };

  // ---- fragment read offsets ------------------------------------------------------------
  const int frow = lane & 15;
  const int fsw = frow >> 1;
  const int a_rd = (wm * 128 + frow) * 128;
  const int b_rd = A_BYTES + (wn * (16 * NF) + frow) * 128;
  const int ph0 = (((lane >> 4)) ^ fsw) * 16;      // k sub-step 0: logical chunks 0..3
  // k sub-step 1 reads logical chunks 4..7: ((4 + x) ^ fsw) * 16 == ph0 ^ 64

  f32x4 acc[8][NF];
#pragma unroll
  for (int mf = 0; mf < 8; ++mf)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) acc[mf][nf] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // prefetch cursor: (tile, k step) of the NEXT stage to issue, advanced with scalar adds only
  const int n_tiles = tile_hi - tile_lo;
  const char* a_tile = (const char*)p.corpus + (size_t)tile_lo * tile_bytes + (size_t)(CPW * w) * 8 * row_b;   // tile being prefetched (+ this wave's row block)
  int pf_kk = 0, pf_left = n_tiles * ksteps;
  int buf = 0;
  if (pf_left > 0) {
    const int ko = pf_kk * (BK * 2);
    stage(a_tile + ko, q_ptr + ko, 0);
    --pf_left;
    if (++pf_kk == ksteps) { pf_kk = 0; a_tile += tile_bytes; }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // One K step: prefetch the next stage, then this stage's fragment reads + 64 MFMAs per wave.
  // PENDING: the previous K step of this corpus tile left its k-half-1 fragments in f1a/f1b;
  // !PENDING = first K step of a corpus tile: its MFMAs start from a zero C operand (an inline
  // constant), so the accumulators are never cleared by separate instructions.
  frag f1a[8], f1b[NF];
  auto kstep = [&](auto pending_tag) {
    constexpr bool PENDING = decltype(pending_tag)::value;
    // Two of the next stage's eight DMA loads go out at the top of the step; in a PENDING step the other six
    // follow two at a time between the pending MFMAs (corpus chunks first: they can miss L2), so that the wave
    // feeds the MFMA pipe again after 2 DMA issues instead of 8 (all at the top: 13.38 ms; 4 + 4: 13.21; 2 + 6: 13.22
    // vs 13.38 in a second pairing).
    const bool do_stage = pf_left > 0;
    const int st_ko = pf_kk * (BK * 2);
    const char* st_a = a_tile + st_ko;
    const char* st_b = q_ptr + st_ko;
    const int st_buf = buf ^ 1;
    if (do_stage) {
      --pf_left;
      if (++pf_kk == ksteps) { pf_kk = 0; a_tile += tile_bytes; }
#pragma unroll
      for (int pp = 0; pp < NPART / 4; ++pp) stage_part(st_a, st_b, st_buf, pp);
      if (!PENDING || DT == MRAG_DT_FP8) {
#pragma unroll
        for (int pp = NPART / 4; pp < NPART; ++pp) stage_part(st_a, st_b, st_buf, pp);
      }
    }
    const char* sb = smem + buf * STAGE_BYTES;
    buf ^= 1;
    if constexpr (DT == MRAG_DT_FP8) {
      // fp8: ONE MFMA per (mf, nf) and step, nothing carried over to the next step.  The B fragments and A rows mf 0-1
      // (12 reads) go first; then the MFMAs of mf run while the reads of mf + 2 land (4 MFMAs, 2 reads, six times).
      const int ph1 = ph0 ^ 64;
      frag g0a[8], g1a[8], g0b[NF], g1b[NF];
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        g0b[nf] = *(const frag*)(sb + b_rd + nf * 2048 + ph0);
        g1b[nf] = *(const frag*)(sb + b_rd + nf * 2048 + ph1);
      }
#pragma unroll
      for (int mf = 0; mf < 8; ++mf) {
        g0a[mf] = *(const frag*)(sb + a_rd + mf * 2048 + ph0);
        g1a[mf] = *(const frag*)(sb + a_rd + mf * 2048 + ph1);
      }
#pragma unroll
      for (int mf = 0; mf < 8; ++mf)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf)
          acc[mf][nf] = Mfma<DT>::run2(g0a[mf], g1a[mf], g0b[nf], g1b[nf], PENDING ? acc[mf][nf] : (f32x4){0.f, 0.f, 0.f, 0.f});
      __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);
#define MRAG_SGB8 __builtin_amdgcn_sched_group_barrier(0x008, NF, 0); __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      MRAG_SGB8 MRAG_SGB8 MRAG_SGB8 MRAG_SGB8 MRAG_SGB8 MRAG_SGB8
#undef MRAG_SGB8
      __builtin_amdgcn_sched_group_barrier(0x008, 2 * NF, 0);
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // as below: the buffer may be restaged after the next barrier
    } else {
      // Software-pipelined fragment reads, two register sets.  The 12 reads of k half 0 are issued
      // first; the 32 MFMAs of k half 1 of the PREVIOUS step (operands already in registers) run
      // while they land; then the 32 MFMAs of half 0 run with the 12 reads of half 1 interleaved.
      // The MFMA pipe never waits on a read it has just issued (hipcc's own order re-reads two
      // fragments per 4-8 MFMAs and waits on each: 65 % MFMA duty at 2.15 GHz in the reads + MFMA
      // ablation).  Accumulation order is unchanged: half 0, half 1 of every K step in sequence.
      const int ph1 = ph0 ^ 64;
      frag f0a[8], f0b[NF];
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) f0b[nf] = *(const frag*)(sb + b_rd + nf * 2048 + ph0);
#pragma unroll
      for (int mf = 0; mf < 8; ++mf) f0a[mf] = *(const frag*)(sb + a_rd + mf * 2048 + ph0);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (PENDING) {
#pragma unroll
        for (int part = 0; part < 4; ++part) {
#pragma unroll
          for (int mf = 2 * part; mf < 2 * part + 2; ++mf)
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) acc[mf][nf] = Mfma<DT>::run(f1a[mf], f1b[nf], acc[mf][nf]);
          if (part < 3) {
            __builtin_amdgcn_sched_barrier(0);
            if (do_stage) {
#pragma unroll
              for (int pp = 0; pp < NPART / 4; ++pp) stage_part(st_a, st_b, st_buf, (1 + part) * (NPART / 4) + pp);
            }
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) f1b[nf] = *(const frag*)(sb + b_rd + nf * 2048 + ph1);
#pragma unroll
      for (int mf = 0; mf < 8; ++mf) f1a[mf] = *(const frag*)(sb + a_rd + mf * 2048 + ph1);
#pragma unroll
      for (int mf = 0; mf < 8; ++mf)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf)
          acc[mf][nf] = Mfma<DT>::run(f0a[mf], f0b[nf], PENDING ? acc[mf][nf] : (f32x4){0.f, 0.f, 0.f, 0.f});
      // pin the interleave: 4 MFMAs, then 2 / 1 LDS reads, eight times (12 reads under 32 MFMAs)
#define MRAG_SGB(n_rd) __builtin_amdgcn_sched_group_barrier(0x008, 4, 0); __builtin_amdgcn_sched_group_barrier(0x100, n_rd, 0);
      MRAG_SGB(2) MRAG_SGB(1) MRAG_SGB(2) MRAG_SGB(1) MRAG_SGB(2) MRAG_SGB(1) MRAG_SGB(2) MRAG_SGB(1)
#undef MRAG_SGB
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // every fragment read of this stage buffer has returned before the next barrier lets it be restaged
    }
  };
  auto kstep_sync = [&]() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the stage prefetched during this step has landed
    __syncthreads();
  };

  for (int ti = 0; ti < n_tiles; ++ti) {
    // allow-set words of this wave's 128 rows of the tile (wave-uniform: one scalar load, issued before the K loop so
    // that its latency hides under the tile's MFMAs)
    u32x4 allow_w = {~0u, ~0u, ~0u, ~0u};
    if constexpr (FILT)
      allow_w = *(const __attribute__((address_space(4))) u32x4*)(p.allow + ((size_t)(tile_lo + ti) * TM + wm * 128) / 32);
    kstep(std::false_type{});
    for (int kk = 1; kk < ksteps; ++kk) {
      kstep_sync();
      kstep(std::true_type{});
    }
    if constexpr (DT != MRAG_DT_FP8) {   // drain: k half 1 of the last K step (fp8: nothing pending)
#pragma unroll
      for (int mf = 0; mf < 8; ++mf)
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) acc[mf][nf] = Mfma<DT>::run(f1a[mf], f1b[nf], acc[mf][nf]);
    }
    {
      // =========================== fused top-k epilogue ===================================
      const int tile = tile_lo + ti;   // ti = tile index inside the split
      // lane-derived values are recomputed from an opaque copy so that nothing the epilogue
      // needs is hoisted out of the K loop (the loop body is near the 256-VGPR budget)
      int elane = lane;
      asm volatile("" : "+v"(elane));
      const int row0 = tile * TM + wm * 128 + (elane >> 4) * 4;  // + mf*16 + j
      const int q0 = wn * (16 * NF) + (elane & 15);              // + nf*16
      const int grp = wm * 4 + (elane >> 4);                     // this lane's segment of each of its queries
      const bool certify = p.k <= K_CERT;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the stage prefetched during the last K step has landed (issued a K step ago: no stall)
      if ((tile + 1) * TM > rows_end) {
#pragma unroll
        for (int mf = 0; mf < 8; ++mf)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (row0 + mf * 16 + j >= rows_end) {
#pragma unroll
              for (int nf = 0; nf < NF; ++nf) acc[mf][nf][j] = -INFINITY;
            }
      }
      if constexpr (FILT) {
        // rows row0 + mf*16 + j: word mf/2 of the wave's four, bit (mf&1)*16 + (lane>>4)*4 + j; an all-allowed half-tile
        // skips the selects (wave-uniform branch)
        if ((allow_w.x & allow_w.y & allow_w.z & allow_w.w) != ~0u) {
          const uint32_t aw[4] = {allow_w.x, allow_w.y, allow_w.z, allow_w.w};
          const int lsh = (elane >> 4) * 4;
#pragma unroll
          for (int mf = 0; mf < 8; ++mf) {
            const uint32_t nib = aw[mf >> 1] >> ((mf & 1) * 16 + lsh);
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (!((nib >> j) & 1u)) {
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) acc[mf][nf][j] = -INFINITY;
              }
          }
        }
      }
      float thr[NF];
      uint32_t* stat_cur = stat + (ti & 1) * TQ;        // certificate built from tiles <= ti
      uint32_t* stat_prev = stat + ((ti & 1) ^ 1) * TQ;  // certificate from tiles < ti
      if (ti == 0) {
        // ---- first tile: tau0 = min over the query's 8 lanes of the lane's 2nd largest score
        // IN this tile; >= 16 rows are >= tau0, so pass on '>=' (as '> next_below').
        if (certify) {
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) {
            float m1 = -INFINITY, m2 = -INFINITY;
#pragma unroll
            for (int mf = 0; mf < 8; ++mf)
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const float v = acc[mf][nf][j];
                m2 = fmaxf(m2, fminf(m1, v));
                m1 = fmaxf(m1, v);
              }
            rm[(nf * 2 + 0) * NT + tid] = __float_as_uint(m1);
            rm[(nf * 2 + 1) * NT + tid] = __float_as_uint(m2);
            float x = m2;
            x = fminf(x, __shfl_xor(x, 16));
            x = fminf(x, __shfl_xor(x, 32));
            if (elane < 16) lds_min_u32(&stat_cur[q0 + nf * 16], f32_ord(x));
          }
          __syncthreads();
          if constexpr (DESC) if (p.k < K_CERT) {   // descriptor instance only: in the dense instance the extra code costs the K loop registers (+2 % measured)
            // Sharper bootstrap: the k-th LARGEST of the query's 16 certified maxima (8 lanes x top 2, distinct rows
            // of this tile) -- k rows reach it, so it certifies like tau0 (which is their 16th largest) and sits
            // near the true k-th best.  It matters most where a workgroup sees ONE tile (IVF list scan: a 150-row
            // list leaves lanes with fewer than two valid rows, tau0 = -inf, every row listed and every query sent
            // through the radix select at the end: 70 % of that kernel).  Rank by counting, 16 work items per
            // query, register-light (the accumulators are live here).
#pragma unroll 1
            for (int wi = tid; wi < min(nq_local, TQ) * 16; wi += NT) {      // (padding queries list nothing: skipped)
              const int ql = wi >> 4, vi = wi & 15;
              const int cq = ql & 15, cnf = (ql >> 4) & (NF - 1), cwn = ql / (16 * NF);
              const uint32_t* col = rm + (cnf * 2) * NT + cwn * 64 + cq;    // + t*NT + ((o>>2)*WN)*64 + (o&3)*16
              float v16[16];
#pragma unroll
              for (int j = 0; j < 16; ++j) v16[j] = __uint_as_float(col[(j & 1) * NT + ((j >> 3) * WN) * 64 + ((j >> 1) & 3) * 16]);   // 16 reads in flight
              float mine = v16[0];
#pragma unroll
              for (int j = 1; j < 16; ++j) mine = (vi == j) ? v16[j] : mine;
              int rank = 0;
#pragma unroll
              for (int j = 0; j < 16; ++j) rank += (v16[j] > mine || (v16[j] == mine && j < vi)) ? 1 : 0;
              if (rank == p.k - 1 && mine > -INFINITY) {
                stat_cur[ql] = f32_ord(mine);
                tau_c[ql] = mine;
              }
            }
            __syncthreads();
          }
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) thr[nf] = next_below(ord_f32(stat_cur[q0 + nf * 16]));
          if constexpr (RANGE) {
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) thr[nf] = fmaxf(thr[nf], fnb);
          }
        } else {
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) thr[nf] = fnb;
        }
      } else {
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
          const float sc = certify ? ord_f32(stat_prev[q0 + nf * 16]) : -INFINITY;
          thr[nf] = fmaxf(sc, tau_c[q0 + nf * 16]);
        }
      }
#pragma unroll
      for (int nf = 0; nf < NF; ++nf)
        if (q0 + nf * 16 >= nq_local) thr[nf] = INFINITY;   // padding queries never list anything
      if constexpr (RANGE) {
        // rows >= floor of this lane's 32 scores per query column (rows past the corpus and disallowed rows are -inf here);
        // a wave-uniform skip for columns nobody reaches, then the 8 lanes of a query are summed into its LDS counter
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
          float tm = -INFINITY;
#pragma unroll
          for (int mf = 0; mf < 8; ++mf) tm = fmaxf(tm, fmaxf(fmaxf(acc[mf][nf][0], acc[mf][nf][1]), fmaxf(acc[mf][nf][2], acc[mf][nf][3])));
          if (!__any(tm > fnb)) continue;
          int c = 0;
#pragma unroll
          for (int mf = 0; mf < 8; ++mf)
#pragma unroll
            for (int j = 0; j < 4; ++j) c += acc[mf][nf][j] > fnb ? 1 : 0;
          if (q0 + nf * 16 >= nq_local) c = 0;   // padding queries never count
          c += __shfl_xor(c, 16);
          c += __shfl_xor(c, 32);
          if (elane < 16 && c) atomicAdd(&rcnt[q0 + nf * 16], c);
        }
      }
      int cseg[NF];   // this lane's segment fill, per query column
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) cseg[nf] = scnt[(q0 + nf * 16) * NGRP + grp];
      if (ti < DENSE_TILES) __builtin_amdgcn_s_barrier();   // every wave is done reading the stage buffer the dense push pass reuses as scratch

      // ---- push: attempt 0 = whole tile at once; a full segment -> replay in 4 sub-rounds ------
      int attempt = 0, round = 0;
      float tmax[NF];
      while (true) {
        int rbase = row0;
        asm volatile("" : "+v"(rbase));   // keep the 128 store operands from being pre-formed outside this loop
        if (ti < DENSE_TILES) {
          // (a) first tiles of a split: some lane passes in almost every accumulator
          // Filter, per query column of this lane (32 scores): lane maximum first; when some lane of
          // the wave beats its threshold, every lane builds a 32-bit pass mask (straight-line code,
          // no branches), parks its 32 scores in LDS ([accumulator][thread] x 16 B: the stage buffer
          // the K loop has just consumed) and a short wave-uniform loop stores one passing score per
          // lane per trip, fetched back from LDS by bit index (registers cannot be indexed at run time).
          // ~140 instructions per column whatever the pass rate -- the early tiles of a split pass
          // somewhere in almost every accumulator, which made per-accumulator branching 4x dearer.
          char* stg = smem + (buf ^ 1) * STAGE_BYTES + tid * 16;
  #pragma unroll
          for (int nf = 0; nf < NF; ++nf) {
            float tm = acc[0][nf][0];
  #pragma unroll
            for (int mf = 0; mf < 8; ++mf) tm = fmaxf(tm, fmaxf(fmaxf(acc[mf][nf][0], acc[mf][nf][1]), fmaxf(acc[mf][nf][2], acc[mf][nf][3])));
            tmax[nf] = tm;
            if (!__any(tm > thr[nf])) continue;
            uint32_t pm = 0u;
  #pragma unroll
            for (int mf = 7; mf >= 0; --mf)
  #pragma unroll
              for (int j = 3; j >= 0; --j) pm = (pm << 1) | (acc[mf][nf][j] > thr[nf] ? 1u : 0u);   // bit = mf*4 + j
            if (attempt) pm &= 0xFFu << (8 * round);            // replay: 2 accumulators (<= 8 pushes/segment) per round
  #pragma unroll
            for (int mf = 0; mf < 8; ++mf) *(f32x4*)(stg + mf * (NT * 16)) = acc[mf][nf];
            const int q = q0 + nf * 16;
            uint2* lst = wg_list + (size_t)q * QCAP + KEPT + grp * SEG;
            int c = cseg[nf];
            while (__any(pm != 0u)) {
              if (pm) {
                const int b = __builtin_ctz(pm);
                pm &= pm - 1u;
                const float v = *(const float*)(stg + (b >> 2) * (NT * 16) + (b & 3) * 4);
                if (c < SEG) lst[c] = make_uint2(__float_as_uint(v), (uint32_t)(rbase + (b >> 2) * 16 + (b & 3)));
                ++c;
              }
            }
            cseg[nf] = c;
          }
        } else {
          // (b) later tiles: passes are sparse.  Two-level filter: max of each 4-score group (one MFMA
          // accumulator) and a wave-uniform test against the column's threshold; only a group in which
          // some lane beats its threshold runs the store path.
  #pragma unroll
          for (int nf = 0; nf < NF; ++nf) {
            const int q = q0 + nf * 16;
            uint2* lst = wg_list + (size_t)q * QCAP + KEPT + grp * SEG;
            float tm = -INFINITY;
            int c = cseg[nf];
            // all eight group tests first (8 v_cmp into 8 SGPR pairs, back to back), then scalar-only
            // branches on the saved masks: a v_cmp -> s_cbranch_vcc pair per group serialises the vector
            // and scalar pipes (~33 cycles per test measured)
            unsigned long long hit[8];
  #pragma unroll
            for (int mf = 0; mf < 8; ++mf) {
              const f32x4 a = acc[mf][nf];
              const float m4 = fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3]));
              tm = fmaxf(tm, m4);
              hit[mf] = __ballot(m4 > thr[nf]);
            }
  #pragma unroll
            for (int mf = 0; mf < 8; ++mf) {
              const f32x4 a = acc[mf][nf];
              if (attempt && (mf >> 1) != round) continue;      // replay: 2 accumulators (<= 8 pushes/segment) per round
              if (hit[mf] == 0ull) continue;
  #pragma unroll
              for (int j = 0; j < 4; ++j) {
                if (a[j] > thr[nf]) {
                  if (c < SEG) {
                    uint32_t sv = __float_as_uint(a[j]);
                    asm volatile("" : "+v"(sv));   // form the {score,row} pair HERE, not hoisted out of the tile loop (spills)
                    lst[c] = make_uint2(sv, (uint32_t)(rbase + mf * 16 + j));
                  }
                  ++c;
                }
              }
            }
            cseg[nf] = c;
            tmax[nf] = tm;
          }
        }
        {
          bool over = false;
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) over |= cseg[nf] > SEG;
          if (over) lds_store_u32(&flags[0], 1u);
        }
        if (attempt == 0 && certify && ti != 0) {
          // fold this tile's maxima into the running certificate used from the NEXT tile on
          // (the four columns as four independent chains: all loads, then all stores, then the shuffles --
          // written column by column the LDS read -> write -> shuffle -> atomic chain ran serially, 3 % of a tile)
          float o1[NF], o2[NF], x[NF];
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) {
            o1[nf] = __uint_as_float(rm[(nf * 2 + 0) * NT + tid]);
            o2[nf] = __uint_as_float(rm[(nf * 2 + 1) * NT + tid]);
          }
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) {
            const float n2 = fmaxf(o2[nf], fminf(o1[nf], tmax[nf])), n1 = fmaxf(o1[nf], tmax[nf]);
            rm[(nf * 2 + 0) * NT + tid] = __float_as_uint(n1);
            rm[(nf * 2 + 1) * NT + tid] = __float_as_uint(n2);
            x[nf] = n2;
          }
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) x[nf] = fminf(x[nf], __shfl_xor(x[nf], 16));
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) x[nf] = fminf(x[nf], __shfl_xor(x[nf], 32));
#pragma unroll
          for (int nf = 0; nf < NF; ++nf)
            if (elane < 16) lds_min_u32(&stat_cur[q0 + nf * 16], f32_ord(x[nf]));
        }
        // This barrier also publishes the stage prefetched during the last K step (every wave waited
        // for its own LDS-DMA loads at the top of the epilogue), so the common path needs no second
        // barrier per tile.  It is a RAW barrier behind an LDS-only wait: the list stores of this tile
        // stay in flight across it (nobody reads the lists before one of the full __syncthreads() of the
        // replay / compaction / end-of-split paths) -- __syncthreads() here made every wave sit out the
        // completion latency of its last 8-byte store on every tile.
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (attempt == 0) {
          if (!flags[0]) {
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) scnt[(q0 + nf * 16) * NGRP + grp] = cseg[nf];   // commit
            if (tid < TQ) stat_prev[tid] = 0xFFFFFFFFu;   // becomes stat_cur of tile ti+1
            break;
          }
          __syncthreads();               // everyone has seen the flag; committed counts are still pre-tile
          if (tid == 0) flags[0] = 0;
          attempt = 1;
          round = 0;
        } else {
#pragma unroll
          for (int nf = 0; nf < NF; ++nf) scnt[(q0 + nf * 16) * NGRP + grp] = cseg[nf];     // commit (cannot overflow)
          if (round == 3) {
            if (tid < TQ) stat_prev[tid] = 0xFFFFFFFFu;
            break;
          }
          ++round;
          __syncthreads();
        }
        // replay step: make room (every segment <= SEG - 8), then reload counts and thresholds
        // LDS scratch: the stage buffer this K step has just consumed (free until the next stage() call)
        compact_owned<QPW>(wg_list, w, elane, p.k, SEG - 8, (uint64_t*)(smem + (buf ^ 1) * STAGE_BYTES + w * 8192));
        __syncthreads();
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
          cseg[nf] = scnt[(q0 + nf * 16) * NGRP + grp];
          float th = tau_c[q0 + nf * 16];
          if (q0 + nf * 16 >= nq_local) th = INFINITY;
          thr[nf] = fmaxf(thr[nf], th);
        }
      }
      // Sharper certificate, refreshed after tiles 0..7, 15, 31, 63, ... of the split: the min over the
      // 8 lanes of their 2nd largest maxima (stat) sits near the 38th best score so far; the k-th
      // LARGEST of the 16 certified maxima (8 lanes x top 2, all distinct earlier rows) is just as valid
      // -- k rows reach it -- and close to the k-th best.  One thread per query sorts the 16 values
      // (bitonic network in registers) and raises tau_c.  Simulated list pushes per (query, split) at
      // k = 10: 231 -> 112 (an exact k-th-best threshold: 88).
      if (certify && p.k < K_CERT && (!DESC || ti != 0) && (ti < 8 || ((ti + 1) & ti) == 0) && ti + 1 < n_tiles) {   // (descriptor mode, tile 0: done in its bootstrap)
        if (tid < TQ) {
          const int cq = tid & 15, cnf = (tid >> 4) & 3, cwn = tid >> 6;
          float v[16];
#pragma unroll
          for (int o = 0; o < 8; ++o) {   // owner lanes of query `tid`: wave row o>>2, lane group o&3
            const int owner = ((o >> 2) * WN + cwn) * 64 + (o & 3) * 16 + cq;
            v[2 * o] = __uint_as_float(rm[(cnf * 2 + 0) * NT + owner]);
            v[2 * o + 1] = __uint_as_float(rm[(cnf * 2 + 1) * NT + owner]);
          }
#pragma unroll
          for (int kk2 = 2; kk2 <= 16; kk2 <<= 1)
#pragma unroll
            for (int j = kk2 >> 1; j > 0; j >>= 1)
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                const int l = i ^ j;
                if (l > i) {
                  const float lo = fminf(v[i], v[l]), hi = fmaxf(v[i], v[l]);
                  const bool desc = (i & kk2) == 0;          // descending overall: v[0] largest
                  v[i] = desc ? hi : lo;
                  v[l] = desc ? lo : hi;
                }
              }
          float sel = v[15];
#pragma unroll
          for (int i = 14; i >= 0; --i) sel = (i == p.k - 1) ? v[i] : sel;
          tau_c[tid] = fmaxf(tau_c[tid], sel);
        }
      }
      // With one K step per tile nothing else separates this tile's flag / certificate words from the
      // next tile's epilogue; the forced compaction below uses the scratch buffer after the barrier.
      bool resync = ksteps == 1;
      if (!certify && ((ti + 1) & ti) == 0 && ti + 1 < n_tiles) {
        resync = true;
        // k > K_CERT has no row-count certificate: thresholds come from compaction alone (tau_c =
        // the k-th best listed so far).  Compact every query after tiles 0, 1, 3, 7, 15, ... of the
        // split: each interval then lists ~k entries per query (the rows seen double, the rate of
        // rows beating a k-th-best threshold halves), so segments practically never fill up.
        __syncthreads();   // all pushes of this tile are in the lists; nobody still parks scores in the stage buffer
        // (the accumulators are dead here: the batched-load form used at the end of the split fits)
        uint64_t* scr = (uint64_t*)(smem + (buf ^ 1) * STAGE_BYTES + w * 8192);
#pragma unroll 1
        // (work area + parking: this wave's 8 KiB of the consumed stage buffer; 4 queries per pass keep the parking at 2 KiB)
        for (int qq = 0; qq < QPW; qq += 4)
          tail_compact<4>(wg_list, w * QPW + qq, p.k, elane, scr, (uint2*)(scr + 768), tau_c);
      }
      if (resync) __syncthreads();
      // (the accumulators are not cleared: the first K step of the next tile starts from a zero C operand)
      // The K loop's lane constants may have been spilled around the epilogue.  Touch them HERE so
      // that the compiler's reload (and its s_waitcnt vmcnt, which would also drain the LDS-DMA
      // prefetch it cannot see) sits at the end of the epilogue, not inside the next K step.
      asm volatile("" :: "v"(a_rd), "v"(b_rd), "v"(ph0), "v"(voff_e), "v"(voff_o));
    }
  }

  __syncthreads();
  // ---- end of the split: every query's list is cut to its k best (sorted) so that K4 only has to
  // merge S x k entries.  Entries below the final certified threshold are dropped before ranking
  // (typically ~25 of ~170 survive), which is what keeps this tail at ~1 % of the workgroup's time.
  if (n_tiles > 0) {
    const uint32_t* stat_last = stat + ((n_tiles - 1) & 1) * TQ;
    uint64_t* scratch = (uint64_t*)(smem + w * 8192);
    // 16 queries per pass: two memory latencies per wave for its 32 lists (they are spread over GBs of
    // list space, i.e. they come from HBM).  Both stage buffers are free here: per wave 8 KiB work area
    // + 8 KiB of parking.  The final thresholds go through the (now idle) tau_c words.
    if (p.k <= K_CERT) {
      for (int i = lane; i < QPW; i += 64) { const int q = w * QPW + i; tau_c[q] = fmaxf(tau_c[q], ord_f32(stat_last[q])); }
    }
    constexpr int TB = 16;
    uint2* park = (uint2*)(smem + NW * 8192 + w * 8192);
    for (int qq = 0; qq < QPW; qq += TB) tail_compact<TB, true>(wg_list, w * QPW + qq, p.k, lane, scratch, park, tau_c);
  }
  __syncthreads();
  if (!DESC && p.clock && blockIdx.x == 0 && tid == 0) {
    p.clock[2] = (long long)__builtin_amdgcn_s_memtime();
    p.clock[3] = (long long)__builtin_amdgcn_s_memrealtime();
  }
  if (tid < TQ) p.counts[(size_t)wg * TQ + tid] = kcnt[tid];
  if constexpr (RANGE) if (tid < TQ) p.rcounts[(size_t)wg * TQ + tid] = rcnt[tid];
}

// K2 launcher.  The kernel is templated on the wave tiling; only the 8-wave form (NF = 4) is built:
// the 4-wave / one-wave-per-SIMD form (NF = 8, 256 accumulator registers per lane) is correct but
// hipcc's allocation of the 256-AGPR tile spills into the K loop (98 ms vs 13.6 ms, round-1 measurement).
// Instance table: column 1 = descriptor mode (DESC, reads p.wg_desc), 2 = filtered dense (FILT, reads p.allow), 3 = range
// (RANGE, reads p.floor, writes p.rcounts), 4 = range + filtered.  Row 2 = the fp8 scan copy (mrag_index_search_fp8): plain
// dense instance only.
int launch_k2(int dtype, bool desc, bool filt, bool range, size_t grid, hipStream_t stream, const BfParams& p) {
  typedef void (*K2Fn)(BfParams);
  static const K2Fn fns[3][5] = {{bf_gemm_topk_kernel<MRAG_F16, 4, false>, bf_gemm_topk_kernel<MRAG_F16, 4, true>,
                                  bf_gemm_topk_kernel<MRAG_F16, 4, false, true>, bf_gemm_topk_kernel<MRAG_F16, 4, false, false, true>,
                                  bf_gemm_topk_kernel<MRAG_F16, 4, false, true, true>},
                                 {bf_gemm_topk_kernel<MRAG_BF16, 4, false>, bf_gemm_topk_kernel<MRAG_BF16, 4, true>,
                                  bf_gemm_topk_kernel<MRAG_BF16, 4, false, true>, bf_gemm_topk_kernel<MRAG_BF16, 4, false, false, true>,
                                  bf_gemm_topk_kernel<MRAG_BF16, 4, false, true, true>},
                                 {bf_gemm_topk_kernel<MRAG_DT_FP8, 4, false>, nullptr, nullptr, nullptr, nullptr}};
  const int di = dtype == MRAG_F16 ? 0 : (dtype == MRAG_BF16 ? 1 : 2), de = range ? (filt ? 4 : 3) : (desc ? 1 : (filt ? 2 : 0));
  if (range && (di > 1 || desc)) return fail(MRAG_ERR_UNSUPPORTED, "range search serves the dense 16-bit index only");
  if (!fns[di][de]) return fail(MRAG_ERR_UNSUPPORTED, "the fp8 scan serves the plain dense search only");
  const int lds = range ? LDS_TOTAL_RANGE : LDS_TOTAL;
  MRAG_TRY(set_max_lds((const void*)fns[di][de], lds));
  if (!grid) return MRAG_OK;
  hipLaunchKernelGGL(fns[di][de], dim3((unsigned)grid), dim3(NTHR), lds, stream, p);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

}  // namespace mrag
