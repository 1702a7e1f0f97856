// The merges of the dense search: every K2 / K2s workgroup left each query's k best (sorted) in its kept area; these
// kernels select the k best of all of them per query, order (score desc, row asc), slots past the corpus (-inf, -1).
//   K4   bf_merge_kernel          one wave per query, any number of regions in batches of 64 (batch regime, descriptor mode)
//   K4s  bf_merge_sorted_kernel   online regime / wide batch: only the heads of the sorted lists, through LDS
//   K4w  bf_merge_wide_kernel     the queries K4s flags: radix select straight from global memory
// + the range count sum and the wide-batch verifier, and launch_merge, which issues the right ones after a launch.
#include "bf_kernels.h"

namespace mrag {

// ------------------------------------------------------------------------------------------
// K4: one wave per query selects the k best of the S workgroups' lists (kept + 8 segments each).
// ------------------------------------------------------------------------------------------
// LDS the merge is launched with: one batch of up to 64 regions (k entries each) on top of the carried best --
// 1 KiB at S = 6, k = 10 instead of a fixed 33 KiB, i.e. 32 instead of 4 resident waves per CU (K4 over 10 000
// queries: 164 -> ~60 us)
static inline int merge_lds_entries(int n_regions, int k) { return std::min(n_regions, 64) * k + KMAX; }

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), off), lo = __shfl_xor((uint32_t)v, off);
    const uint64_t o = ((uint64_t)hi << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}

// k best keys of keys[0..fill) -> best[0..nsel), best first (keys are unique: the row is in the key)
__device__ __forceinline__ int merge_extract(const uint64_t* keys, int fill, int k, uint64_t* best, int lane) {
  uint64_t last = ~0ull;
  const int nsel = min(k, fill);
  for (int i = 0; i < nsel; ++i) {
    uint64_t m = 0ull;
    for (int e = lane; e < fill; e += 64) {
      const uint64_t key = keys[e];
      if (key < last && key > m) m = key;
    }
    m = wave_max_u64(m);
    if (lane == 0) best[i] = m;
    last = m;
  }
  return nsel;
}

// One wave per query.  Every K2 workgroup left the query's k best (sorted) in its kept area; 64
// of them are gathered at a time, one per lane, into LDS at offsets from a wave prefix sum, then
// the k best are extracted by k wave-wide max passes.
__global__ __launch_bounds__(64) void bf_merge_kernel(MergeParams p) {
  uint64_t* keys = (uint64_t*)smem;          // [cap] dynamic (merge_lds_entries)
  __shared__ uint64_t best[KMAX];
  const int lane = threadIdx.x;
  const int64_t q = blockIdx.x;
  if (q >= p.nq) return;
  const int t = (int)(q / TQ), ql = (int)(q % TQ);
  const int k = p.k;
  const int n_regions = p.pair_loc ? p.nprobe : p.S;   // one region (the kept area, <= k entries) per K2 workgroup
  int fill = 0;
  for (int r0 = 0; r0 < n_regions; r0 += 64) {
    const int r = r0 + lane;
    int c = 0;
    size_t base = 0;
    if (r < n_regions) {
      size_t wq;
      bool ok = true;
      if (p.pair_loc) {
        const int2 loc = p.pair_loc[q * p.nprobe + r];
        ok = loc.x >= 0;
        wq = (size_t)(ok ? loc.x : 0) * TQ + (size_t)loc.y;
      } else {
        wq = (size_t)(t * p.S + r) * TQ + ql;
      }
      if (ok) c = p.counts[wq];
      base = wq * QCAP;
    }
    int incl = c;   // inclusive wave prefix sum
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int v = __shfl_up(incl, off);
      if (lane >= off) incl += v;
    }
    const int total = __shfl(incl, 63);
    if (fill + total > p.cap) {   // make room: fold what is staged into the running best
      __syncthreads();
      const int nb = merge_extract(keys, fill, k, best, lane);
      __syncthreads();
      for (int i = lane; i < nb; i += 64) keys[i] = best[i];
      fill = nb;
    }
    const int off0 = fill + incl - c;
    // eight entries of the lane's region in flight at a time (written one load per trip, every trip sat out a full
    // memory round trip: the lists were written by other CUs, so they come from beyond L2 -- 41 us for ONE query's
    // 256 regions in the online regime)
    int cmax = c;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cmax = max(cmax, __shfl_xor(cmax, off));
    for (int i0 = 0; i0 < cmax; i0 += 8) {
      uint2 e[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) e[u] = (i0 + u < c) ? p.list[base + i0 + u] : make_uint2(0u, 0u);
      if (p.row_ids) {
#pragma unroll
        for (int u = 0; u < 8; ++u) if (i0 + u < c) e[u].y = (uint32_t)p.row_ids[e[u].y];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) if (i0 + u < c) keys[off0 + i0 + u] = make_key(e[u].x, e[u].y);
    }
    fill += total;
  }
  __syncthreads();
  const int nbest = merge_extract(keys, fill, k, best, lane);
  __syncthreads();
  for (int i = lane; i < k; i += 64) {
    float sc = -INFINITY;
    int64_t id = -1;
    if (i < nbest) {
      const uint64_t key = best[i];
      sc = ord_f32((uint32_t)(key >> 32));
      id = p.id_base + (int64_t)(0xFFFFFFFFu - (uint32_t)key);
    }
    p.out_scores[q * k + i] = sc;
    p.out_ids[q * k + i] = id;
  }
}

// K4s, the merge of the online regime (a handful of queries x up to 256 splits, k <= 256): every split left its k best
// SORTED, and the global top k draws on average k/S entries from each, so only the heads of the lists are read.  One
// 256-thread workgroup per query, thread = region: round 1 loads 8 entries of every region into LDS and radix-selects
// the k-th largest of what is loaded (T); a region whose last loaded entry still reaches T may hold more of the top k
// and loads 8 more; repeat until no region does.  Then every unloaded entry is below its region's last loaded one,
// hence below T: the k largest loaded keys ARE the global top k.  Typically one round, 2 048 entries instead of S * k
// (the one-wave K4 walked 256 regions in four dependent batches: 41 us of a 0.30 ms search; the global-memory radix
// select K4w took 0.27 ms at k = 200).  A query whose loads would not fit the LDS budget is flagged and left to K4w.
constexpr int MS_CAP = 12288;          // keys staged in LDS (96 KiB)

// k-th largest of the (more than k, unique) keys of a key source as a (shift, prefix) pair: selected <=> (key >> shift) >=
// prefix.  src(i, key) -> bool yields the key of index slot i of n, or false for an empty slot.  MSB-first radix select, 8
// bits per pass over an LDS histogram: each pass narrows the bucket that holds the k-th key, and it stops as soon as that
// bucket is needed whole.  All 256 threads; hist[256] and pick[3] (digit, keys above it, keys in its bin) are LDS scratch.
template <class KeySrc>
__device__ __forceinline__ void block_radix_kth(KeySrc src, int n, int k, uint32_t* hist, int* pick, int tid,
                                                int& shift_out, uint64_t& prefix_out) {
  const int lane = tid & 63;
  int need = k, shift = 56;
  uint64_t prefix = 0ull;
  for (; shift >= 0; shift -= 8) {
    hist[tid] = 0u;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
      uint64_t key;
      if (src(i, key) && (shift == 56 || (key >> (shift + 8)) == prefix)) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {           // wave 0: bins 4*lane .. 4*lane+3, suffix sums over the lanes above
      const int hb[4] = {(int)hist[lane * 4], (int)hist[lane * 4 + 1], (int)hist[lane * 4 + 2], (int)hist[lane * 4 + 3]};
      const int mine = hb[0] + hb[1] + hb[2] + hb[3];
      int suf = mine;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_down(suf, off);
        if (lane + off < 64) suf += v;
      }
      int cum = suf - mine;
#pragma unroll
      for (int b = 3; b >= 0; --b) {
        if (cum < need && cum + hb[b] >= need) { pick[0] = lane * 4 + b; pick[1] = cum; pick[2] = hb[b]; }
        cum += hb[b];
      }
    }
    __syncthreads();
    const int digit = pick[0], above = pick[1], inb = pick[2];
    need -= above;
    prefix = (prefix << 8) | (uint64_t)digit;
    if (inb == need) break;   // the whole bucket is selected
  }
  if (shift < 0) shift = 0;
  shift_out = shift;
  prefix_out = prefix;
}

// The shared tail of K4s and K4w: the selected keys of the source (at most k: keys are unique, the row is in the key) are
// gathered into sel, ranked by counting and written to query q's output row; slots past them are (-inf, -1).  All 256
// threads; *s_nsel is an LDS counter the kernel zeroed before its last barrier.
template <class KeySrc>
__device__ __forceinline__ void merge_write_selected(const MergeParams& p, int64_t q, KeySrc src, int n, int shift, uint64_t prefix,
                                                     uint64_t* sel, int* s_nsel, int tid) {
  const int k = p.k;
  for (int i = tid; i < n; i += 256) {
    uint64_t key;
    if (src(i, key) && (key >> shift) >= prefix) sel[atomicAdd(s_nsel, 1)] = key;
  }
  __syncthreads();
  const int nsel = *s_nsel;
  if (tid < nsel) {
    const uint64_t my = sel[tid];
    int rank = 0;
    for (int j = 0; j < nsel; ++j) rank += sel[j] > my ? 1 : 0;
    p.out_scores[q * k + rank] = ord_f32((uint32_t)(my >> 32));
    p.out_ids[q * k + rank] = p.id_base + (int64_t)(0xFFFFFFFFu - (uint32_t)my);
  }
  for (int i = nsel + tid; i < k; i += 256) { p.out_scores[q * k + i] = -INFINITY; p.out_ids[q * k + i] = -1; }
}

__global__ __launch_bounds__(256) void bf_merge_sorted_kernel(MergeParams p, int* __restrict__ fallback, int cap) {
  uint64_t* keys = (uint64_t*)smem;        // [MS_CAP] dynamic
  __shared__ uint32_t hist[256];
  __shared__ uint64_t sel[KMAX_WIDE];
  __shared__ int pick[3];
  __shared__ int s_total, s_more, s_nsel;
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  if (q >= p.nq) return;
  const int t = (int)(q / TQ), ql = (int)(q % TQ);
  const int k = p.k, S = p.S;
  int c = 0;
  size_t base = 0;
  if (tid < S) {
    const size_t wq = (size_t)(t * S + tid) * TQ + ql;
    c = min(p.counts[wq], k);
    base = wq * QCAP;
  }
  if (tid == 0) { s_total = 0; s_nsel = 0; }
  int loaded = 0, shift = 0;
  uint64_t last = ~0ull, prefix = 0ull;     // T = (shift, prefix); (0, 0) selects everything
  bool overflow = false;
  auto staged = [&](int i, uint64_t& key) -> bool { key = keys[i]; return true; };
  for (int round = 0; round < 64; ++round) {
    if (tid == 0) s_more = 0;
    __syncthreads();
    const bool want = loaded < c && (last >> shift) >= prefix;
    const int n_new = want ? min(8, c - loaded) : 0;
    int slot = 0;
    if (n_new) { slot = atomicAdd(&s_total, n_new); atomicOr(&s_more, 1); }
    __syncthreads();
    if (!s_more) break;
    if (s_total > cap) { overflow = true; break; }        // (uniform: s_total is read after the barrier)
    if (n_new) {
      uint2 e[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) e[u] = u < n_new ? p.list[base + loaded + u] : make_uint2(0u, 0u);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (u < n_new) { last = make_key(e[u].x, e[u].y); keys[slot + u] = last; }    // sorted: the last one loaded is the region's smallest so far
      loaded += n_new;
    }
    __syncthreads();
    const int n = s_total;
    if (n > k) block_radix_kth(staged, n, k, hist, pick, tid, shift, prefix);
    else { shift = 0; prefix = 0ull; }
  }
  if (tid == 0) fallback[q] = overflow ? 1 : 0;
  if (overflow) return;                      // K4w redoes this query from global memory
  merge_write_selected(p, q, staged, s_total, shift, prefix, sel, &s_nsel, tid);   // min(s_total, k) keys
}

// K4w (fallback of K4s; 64 < k <= 256, the online regime with the reference's 200-candidate pool): one 256-thread workgroup
// per query selects the k best of the S regions' sorted lists straight from global memory (S*k <= 65 536
// keys, L2-resident): the radix select of the k-th key (block_radix_kth) over the lists themselves, then the tail of
// K4s.  Same order as K4: (score desc, row asc); slots past the corpus are (-inf, -1).
__global__ __launch_bounds__(256) void bf_merge_wide_kernel(MergeParams p, const int* __restrict__ only_flagged) {
  if (only_flagged && !only_flagged[blockIdx.x]) return;   // K4s handled this query
  __shared__ uint32_t hist[256];
  __shared__ uint64_t sel[KMAX_WIDE];
  __shared__ int cnts[256];
  __shared__ int s_pick[3];     // digit, keys above it, keys in its bin
  __shared__ int s_nsel;
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  if (q >= p.nq) return;
  const int t = (int)(q / TQ), ql = (int)(q % TQ);
  const int k = p.k, S = p.S;
  cnts[tid] = tid < S ? min(p.counts[(size_t)(t * S + tid) * TQ + ql], k) : 0;
  if (tid == 0) s_nsel = 0;
  __syncthreads();
  int total = 0;
  for (int r = 0; r < S; ++r) total += cnts[r];
  const int span = S * k;       // entry idx -> (region idx / k, slot idx % k)
  auto fetch = [&](int idx, uint64_t& key) -> bool {
    const int r = idx / k, i = idx - r * k;
    if (i >= cnts[r]) return false;
    const uint2 e = p.list[((size_t)(t * S + r) * TQ + ql) * QCAP + i];
    key = make_key(e.x, e.y);
    return true;
  };
  int shift = 0;
  uint64_t prefix = 0ull;
  if (total > k) block_radix_kth(fetch, span, k, hist, s_pick, tid, shift, prefix);
  merge_write_selected(p, q, fetch, span, shift, prefix, sel, &s_nsel, tid);   // min(total, k) keys
}

// range search: out[q] = the sum of query q's count slots over the S splits of its query tile (one wave per query)
__global__ __launch_bounds__(64) void range_count_sum_kernel(const int* __restrict__ slots, int S, int64_t nq, int64_t* __restrict__ out) {
  const int64_t q = blockIdx.x;
  const int lane = threadIdx.x;
  if (q >= nq) return;
  const int t = (int)(q / TQ), ql = (int)(q % TQ);
  long long c = 0;
  for (int s = lane; s < S; s += 64) c += slots[(size_t)(t * S + s) * TQ + ql];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if (lane == 0) out[q] = (int64_t)c;
}

// ------------------------------------------------------------------------------------------
// Wide batches (64 < k <= 256, more than a handful of queries -- batch evaluation with the reference's 200-candidate pool,
// config/settings.yaml:101-102): the batch kernel keeps at most KMAX = 64 entries per (query, corpus split), so it runs
// with k' = 64 over S >= 4k / 64 splits and the merge takes the k best of the S x 64 candidates.  That answer is exact
// unless some split held MORE than 64 of the query's true top k; this kernel checks it: a split whose list is full and
// whose worst kept entry still beats the merged k-th entry may have dropped rows that belong in the answer.  Flagged
// queries (a handful per 10 000 on i.i.d. rows; many when a query's neighbours sit in adjacent rows) are redone exactly
// by the streaming kernel.  One thread per query.
__global__ void bf_wide_verify_kernel(const uint2* __restrict__ list, const int* __restrict__ counts, int S, int k_kept, int k,
                                      int64_t nq, const float* __restrict__ out_scores, const int64_t* __restrict__ out_ids,
                                      int64_t id_base, int* __restrict__ need) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const int t = (int)(q / TQ), ql = (int)(q % TQ);
  const int64_t tid_ = out_ids[q * k + k - 1];
  const uint64_t key_tau = tid_ < 0 ? 0ull : make_key(__float_as_uint(out_scores[q * k + k - 1]), (uint32_t)(tid_ - id_base));
  int bad = 0;
  for (int s = 0; s < S; ++s) {
    const size_t wq = (size_t)(t * S + s) * TQ + ql;
    if (counts[wq] >= k_kept) {
      const uint2 e = list[wq * QCAP + (k_kept - 1)];
      if (make_key(e.x, e.y) > key_tau) bad = 1;
    }
  }
  need[q] = bad;
}

int launch_range_sum(const int* slots, int S, int64_t nq, int64_t* out, hipStream_t stream) {
  if (!out || nq <= 0) return MRAG_OK;
  hipLaunchKernelGGL(range_count_sum_kernel, dim3((unsigned)nq), dim3(64), 0, stream, slots, S, nq, out);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

int launch_merge(MergeParams mp, int* flags, int* need, hipStream_t stream) {
  const unsigned nq = (unsigned)mp.nq;
  mp.cap = merge_lds_entries(mp.pair_loc ? mp.nprobe : mp.S, mp.k);
  if (!flags) {
    hipLaunchKernelGGL(bf_merge_kernel, dim3(nq), dim3(64), (size_t)mp.cap * 8, stream, mp);
  } else {
    // K4s (heads of the sorted lists through LDS) + K4w for the queries it flags (adversarial layouts only)
    MRAG_TRY(set_max_lds((const void*)bf_merge_sorted_kernel, MS_CAP * 8));
    static const int env_cap = [] { const char* e = getenv("MRAG_K4S_CAP"); return e ? std::max(0, std::min(atoi(e), MS_CAP)) : MS_CAP; }();   // test knob of the online regime: 0 sends every query to K4w
    hipLaunchKernelGGL(bf_merge_sorted_kernel, dim3(nq), dim3(256), (size_t)MS_CAP * 8, stream, mp, flags, need ? MS_CAP : env_cap);
    hipLaunchKernelGGL(bf_merge_wide_kernel, dim3(nq), dim3(256), 0, stream, mp, (const int*)flags);
    if (need)   // wide batch: the batch kernel kept KMAX entries per (query, split)
      hipLaunchKernelGGL(bf_wide_verify_kernel, dim3((nq + 255) / 256), dim3(256), 0, stream, mp.list, mp.counts, mp.S, KMAX, mp.k, mp.nq,
                         (const float*)mp.out_scores, (const int64_t*)mp.out_ids, mp.id_base, need);
  }
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

}  // namespace mrag
