// What the dense-index sources (bf_*.hip) share among themselves: the
// tile and list constants, the kernel parameter blocks, the orderable-key and LDS helpers, the regime rule and the plain
// host launchers each source exports.  Internal to those sources; what other translation units use is in common.h.
#pragma once
#include "common.h"
#include <type_traits>

#include <math.h>
#include <cmath>
#include <stdlib.h>
#include <algorithm>

namespace mrag {

constexpr int TM = 256;   // corpus rows per tile
constexpr int TQ = 256;   // queries per tile
constexpr int BK = 64;    // K elements per stage
constexpr int NTHR = 512;
constexpr int A_BYTES = TM * BK * 2;            // 32 KiB

constexpr int NGRP = 8;                   // lanes (2 waves x 4 lane groups) that share a query
constexpr int SEG = 64;                   // private list segment per (query, lane group)
constexpr int KEPT = 64;                  // compacted entries per query (= largest k)
constexpr int QCAP = KEPT + NGRP * SEG;   // 576 list entries per (workgroup, query)
constexpr int KMAX = KEPT;                // largest k of the batch kernel (K2) and of the IVF list scan
constexpr int KMAX_WIDE = 256;            // largest k of the streaming kernel (K2s) and of the dense index: the reference's
                                          // dense pool is 200 candidates per question (config/settings.yaml:101-102,
                                          // retrieval_backend.py:218)
constexpr int SQ = 16;                    // query columns per block of the streaming kernel (one MFMA B fragment)

struct BfParams {
  const uint16_t* corpus;   // [n_cap][ld]
  const uint16_t* queries;  // [T*256][ld]
  int ld;                   // padded dim (elements), multiple of 64
  int ksteps;               // ld / 64
  int n_rows;               // valid corpus rows
  int n_ctiles;             // ceil(n_rows / 256)
  int nq;                   // valid queries (rows >= nq of the last query tile are padding)
  int T;                    // query tiles
  int S;                    // corpus splits
  int k;
  int xcd_map;              // 0: plain map; else S % 8 == 0 and this many query tiles share an XCD at a time
  const int* wg_desc;       // descriptor mode (IVF list scan): per workgroup {query row0, valid queries,
                            // first tile, end tile, end row, 0,0,0}; NULL = dense (t, s) decomposition
  long long* clock;         // 4 words or NULL: workgroup 0's s_memtime / s_memrealtime at entry and exit
  uint2* list;              // [T*S][256][QCAP]  {score bits, local row}: one 8-byte store per push
  int* counts;              // [T*S][256] entries left in the kept area
  const uint32_t* allow;    // FILT instances: allow-set bitset (bit r%32 of word r/32), padded with zero words to whole tiles
  float floor;              // RANGE instances: score floor (finite); rows scoring >= floor are listed and counted
  int* rcounts;             // RANGE instances: [T*S][256] rows >= floor per (workgroup, query), one slot each
};

struct StreamParams {
  const uint16_t* corpus;
  const uint16_t* queries;   // [>= 16 rows][ld], rows >= nq are zero
  int ld, ksteps, n_rows, n_ctiles, nq, S, k;
  uint2* list;               // K4 layout: [(wg*256 + q)*QCAP + i]
  int* counts;               // [wg*256 + q]
  const uint32_t* allow;     // FILT instances: allow-set bitset, as BfParams::allow
  float floor;               // RANGE instances: score floor, as BfParams::floor
  int* rcounts;              // RANGE instances: [wg*256 + q] rows >= floor of the workgroup's split
};

struct MergeParams {
  const uint2* list;
  const int* counts;
  int T, S, k;
  int64_t nq;
  int64_t id_base;
  const int2* pair_loc;     // descriptor mode: [nq][nprobe] (workgroup, slot) of each probe, wg < 0 = none
  int nprobe;
  const int64_t* row_ids;   // descriptor mode: stored position -> original row (ties break on it)
  int cap;                  // K4: LDS key slots of this launch (filled in by launch_merge)
  float* out_scores;   // [nq][k]
  int64_t* out_ids;    // [nq][k]
};

// The regime of a dense search of nq queries over n_rows rows: bf_launch runs it, AUTO's filter rule plans for it.
enum BfRegime { BF_STREAM, BF_WIDE_BATCH, BF_BATCH };
static inline BfRegime bf_regime(int64_t nq, int k, int64_t n_rows, bool force_stream) {
  const int64_t n_ctiles = (n_rows + TM - 1) / TM;
  if (k > KMAX && nq > 32 && n_ctiles >= 64) return BF_WIDE_BATCH;
  if (k > KMAX || force_stream || (nq <= (k > 32 ? 8 : SQ) && n_ctiles >= 8)) return BF_STREAM;
  return BF_BATCH;
}

// ---- host launchers the dense sources export to each other (every pointer is a device pointer) ----
// the maximum dynamic LDS of a kernel, set once per process (bf_index.hip)
int set_max_lds(const void* fn, int bytes);
// K2 (bf_batch.hip): the instance for dtype x (descriptor mode | filtered | range | range + filtered) over `grid` workgroups
int launch_k2(int dtype, bool desc, bool filt, bool range, size_t grid, hipStream_t stream, const BfParams& p);
// K2s (bf_stream.hip): the instance for dtype x filtered x range x (wide: 8 queries with 512-entry lists, k > 32) over p.S workgroups
int launch_k2s(int dtype, bool filt, bool range, bool wide, hipStream_t stream, const StreamParams& p);
// The merge after a K2 / K2s launch (bf_merge.hip).  flags == NULL: K4.  Otherwise K4s, then K4w for the queries K4s
// flags in flags[0 .. nq); need != NULL (wide batch): then the verifier, need[q] = 1 where query q must be redone.
int launch_merge(MergeParams mp, int* flags, int* need, hipStream_t stream);
// range search (bf_merge.hip): the per-query sums of the count slots of one launch (T query tiles x S splits) -> out[0 .. nq)
int launch_range_sum(const int* slots, int S, int64_t nq, int64_t* out, hipStream_t stream);

// ---- limits of the composite searches that tests and documents cite (each search's kernels, launchers and entry points are
// in its own source) ----
// bf_rerank_batch.hip: rows per descriptor of the batched candidate lookup.  Each of the 4 waves amortises the one read of its
// question's query row over 16 stored rows (6 % extra traffic), the reference's 200-candidate pool still spreads over 4
// workgroups, and a 10 000 x 200 batch is 40 000 workgroups -- some 150 per CU, so a tail does not show.
constexpr int RERANK_ROWS = 64;
// bf_filter_batch.hip: largest set the scan route of mrag_index_search_sets serves: the register-path capacity of the select
// kernel (SEL_CAP in ivf_scan.hip, 256 threads x 32 entries).  The project's own constant, not a tuned one: a measured
// crossover would replace it, with its measurement in DESIGN.md.
constexpr int SETS_SCAN_MAX_ROWS = 8192;
// bf_groups.hip: one workgroup per question sorts its queries * k entries in LDS (fuse.hip's limit)
constexpr int GROUPS_MAX_ENTRIES = 4096;
// bf_collapse.hip: one thread per list entry bounds a list at this many entries (= KMAX_WIDE, the deepest search)
constexpr int COLLAPSE_MAX_SCAN = 256;
// bf_neighbors.hip: one workgroup per question sorts its seeds * (2 * window + 1) entries in LDS, one thread per seed walks
// the keys; the distance and the seed position of an entry share 16 bits (5 + 8)
constexpr int NEIGHBORS_MAX_ENTRIES = 4096;
constexpr int NEIGHBORS_MAX_SEEDS = 256;
constexpr int NEIGHBORS_MAX_WINDOW = 16;
constexpr int NEIGHBORS_MAX_M = 4096;

// the padded size of a question that one workgroup sorts in LDS (bf_groups.hip, bf_neighbors.hip): the power of two >= n, >= 2
__host__ __device__ inline int groups_pow2(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

#if defined(__HIPCC__)
// bitonic sort of perm[0 .. P) (P a power of two, distinct elements) under a strict total order; ends on a barrier
template <class Less>
__device__ inline void groups_sort(unsigned short* perm, int P, Less less) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += blockDim.x) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
        const unsigned short a = perm[i], b = perm[l];
        if (less((int)b, (int)a) == ((i & k) == 0)) { perm[i] = b; perm[l] = a; }
      }
      __syncthreads();
    }
}

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_vptr;
typedef const __attribute__((address_space(1))) void* glb_vptr;

__device__ __forceinline__ uint32_t f32_ord(float f) {
  uint32_t b = __float_as_uint(f);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float ord_f32(uint32_t o) {
  uint32_t b = o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu);
  return __uint_as_float(b);
}
// largest float strictly below x in comparison order (x finite or -inf; -inf stays -inf)
__device__ __forceinline__ float next_below(float x) {
  if (x == -INFINITY) return x;
  float nb = ord_f32(f32_ord(x) - 1u);
  if (nb == x) nb = ord_f32(f32_ord(nb) - 1u);   // +0.0 -> -0.0 compares equal: step once more
  return nb;
}
// larger key = better: higher score first, then LOWER row
__device__ __forceinline__ uint64_t make_key(uint32_t score_bits, uint32_t row) {
  return ((uint64_t)f32_ord(__uint_as_float(score_bits)) << 32) | (uint64_t)(0xFFFFFFFFu - row);
}

template <int DT> struct Mfma;
template <> struct Mfma<MRAG_F16> {
  typedef f16x8 frag;
  static __device__ __forceinline__ f32x4 run(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};
template <> struct Mfma<MRAG_BF16> {
  typedef bf16x8 frag;
  static __device__ __forceinline__ f32x4 run(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};
// fp8 scan copy: the block-scaled 16x16x128 form, one MFMA per two 16-byte fragment reads (common.h)
template <> struct Mfma<MRAG_DT_FP8> : MfmaFp8 {};

extern __shared__ __attribute__((aligned(16))) char smem[];

// Note on waits: the LDS-DMA stage loads are issued from inline asm, so hipcc does not know an
// LDS write is pending on the VM counter and ordinary LDS accesses in the epilogue get lgkmcnt
// waits only (with the __builtin_amdgcn_global_load_lds form every LDS access was guarded by
// s_waitcnt vmcnt(0), draining the prefetch and every outstanding list store per access).
__device__ __forceinline__ uint32_t lds_off(const void* p) {
  return (uint32_t)(size_t)(const __attribute__((address_space(3))) char*)p;
}
__device__ __forceinline__ uint32_t lds_load_u32(const void* p) {
  uint32_t v;
  asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(lds_off(p)) : "memory");
  return v;
}
__device__ __forceinline__ void lds_min_u32(void* p, uint32_t x) {
  asm volatile("ds_min_u32 %0, %1" : : "v"(lds_off(p)), "v"(x) : "memory");
}
__device__ __forceinline__ void lds_store_u32(void* p, uint32_t x) {
  asm volatile("ds_write_b32 %0, %1" : : "v"(lds_off(p)), "v"(x) : "memory");
}
#endif

}  // namespace mrag
