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
#include "bf_kernels.h"

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
int launch_collapse_heads(const float* in_sc, const int64_t* in_id, int64_t nq, int scan_k, const int32_t* key_of, int64_t n_rows,
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
int64_t collapse_mask_words(int64_t n_rows) { return round_up(std::max<int64_t>(n_rows, 1), TM) / 32; }

int launch_collapse_mask(const int32_t* key_of, int64_t n_rows, const int32_t* found, const int32_t* word, int k, uint32_t* bits,
                         hipStream_t stream) {
  hipLaunchKernelGGL(collapse_mask_kernel, dim3((unsigned)(collapse_mask_words(n_rows) / 8)), dim3(256), 0, stream, key_of, n_rows,
                     found, word, k, bits);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

}  // namespace mrag
