// Neighbour expansion of search hits (mrag_index_expand_neighbors): the graph channel of the hybrid retrieval.  Every stored
// row carries one int32 key (CollapseState::keys, mrag_index_set_row_keys); the RUN of a row is the maximal interval of
// consecutive rows with its key -- one document's sentences -- and the neighbours of a row are the adjacent rows of its run
// (the reference's next_in_doc edges, edge_builder.py:106-120).  Per question, from its row of seed ids:
//   a seed id of -1 or outside [id_base, id_base + n) is skipped; seed r reaches [max(run_lo, r - w), min(run_hi, r + w)];
//   per distinct reached row c: dist = min |c - r| over the seeds that reach c, seed = the lowest seed position attaining it,
//   score = decay[dist]; the rows are ordered by (dist asc, seed position asc, row asc) and the first m are written as
//   (score, id_base + c, dist, seed position); the slots past the distinct rows hold (-inf, -1, -1, -1).
// Integer only and exact: this is the multi-source BFS of graph_utils.expand_qmatch_neighbors (graph_utils.py:58-129) over
// chain graphs, as a mapping row -> (score, distance) (DESIGN.md §3 "Graph channel").
//
//   grid       one workgroup per question; blockDim = half the padded entry count, 64 .. 1024 threads
//   entries    n = seed_stride * (2w + 1): entry e = j * (2w + 1) + (d + w) is the row r_j + d of seed position j, -w <= d <= w;
//              entries outside the seed's reach and entries of skipped seeds are padding.  P = the power of two >= n (>= 2).
//   LDS        static: the seeds' rows and reaches, 3 x 4 x 256 bytes, and the decay table (17 floats): 3 140 bytes.
//              dynamic, 9 P bytes, sized by the launch (every question of a call has the same n):
//                row    4 P       int32 local row, -1 = padding
//                ds     2 P       dist << 8 | seed position (5 + 8 bits): the order of (dist, seed position) is the order of ds
//                perm   2 P       entry indexes, sorted twice in place
//                head   1 P       by entry: 1 = the entry that represents its row
//              36 KiB + 3 KiB at the limit of 4096 entries -- below the 64 KiB a kernel gets without raising its dynamic-LDS
//              limit.  As in bf_groups.hip both sorts read row / ds THROUGH perm (data-dependent addresses); staging, perm,
//              head and the outputs are unit stride per array.
//   walk       one thread per seed (a loop when there are more seeds than threads) reads at most w keys to each side of its
//              row, every index checked against [0, n) before the read, and leaves (row, lo, hi) in LDS
//   sort 1     groups_sort (bf_kernels.h) by (real before padding, row asc, ds asc, entry asc): the first entry of a row's run
//              of entries has its smallest distance, and among those the lowest seed position
//   heads      head[e] = 1 for the first entry of every row
//   sort 2     groups_sort by (head before the rest, ds asc, row asc)
//   output     slot r < m: the r-th entry of sort 2 if it is a head, else (-inf, -1, -1, -1)
// Plain vector loads and stores only; 14 VGPRs, no scratch.  A question's outputs depend on its own seed row alone.
#include "bf_index.h"

namespace mrag {

static_assert(9 * NEIGHBORS_MAX_ENTRIES + 3 * 4 * NEIGHBORS_MAX_SEEDS + 4 * (NEIGHBORS_MAX_WINDOW + 1) <= 65536,
              "the neighbour expansion stays inside the default dynamic-LDS limit");
static_assert(NEIGHBORS_MAX_WINDOW < 32 && NEIGHBORS_MAX_SEEDS <= 256, "dist and seed position share 16 bits (5 + 8)");
static_assert(NEIGHBORS_MAX_ENTRIES <= 65536, "perm holds entry indexes in 16 bits");

struct NeighborsDecay { float v[NEIGHBORS_MAX_WINDOW + 1]; };   // by value in the kernel arguments

static inline size_t neighbors_lds_bytes(int P) { return (size_t)9 * P; }

__global__ __launch_bounds__(1024) void neighbors_kernel(const int64_t* __restrict__ seeds, int seed_stride, int window,
                                                         NeighborsDecay decay, const int32_t* __restrict__ key_of,
                                                         int64_t n_rows, int64_t id_base, int m, float* __restrict__ out_sc,
                                                         int64_t* __restrict__ out_id, int32_t* __restrict__ out_dist,
                                                         int32_t* __restrict__ out_seed) {
  extern __shared__ __attribute__((aligned(16))) char neighbors_lds[];
  __shared__ int32_t s_seed[NEIGHBORS_MAX_SEEDS], s_lo[NEIGHBORS_MAX_SEEDS], s_hi[NEIGHBORS_MAX_SEEDS];
  __shared__ float s_decay[NEIGHBORS_MAX_WINDOW + 1];
  const int tid = threadIdx.x, T = blockDim.x;
  const int64_t q = blockIdx.x;
  const int span = 2 * window + 1, n = seed_stride * span;   // <= NEIGHBORS_MAX_ENTRIES (validated on the host)
  const int P = groups_pow2(n);
  int32_t* s_row = (int32_t*)neighbors_lds;
  unsigned short* s_ds = (unsigned short*)(s_row + P);
  unsigned short* perm = s_ds + P;
  unsigned char* head = (unsigned char*)(perm + P);

  if (tid == 0) {
#pragma unroll
    for (int d = 0; d <= NEIGHBORS_MAX_WINDOW; ++d) s_decay[d] = decay.v[d];
  }
  // 0) one thread per seed: its local row and its reach inside its run
  for (int j = tid; j < seed_stride; j += T) {
    const int64_t id = seeds[(size_t)q * seed_stride + j];
    int32_t r = -1, lo = 0, hi = -1;
    if (id != -1 && id >= id_base && (uint64_t)id - (uint64_t)id_base < (uint64_t)n_rows) {
      r = (int32_t)(id - id_base);
      const int32_t key = key_of[r];
      lo = hi = r;
      for (int t = 1; t <= window; ++t) {
        if (r - t < 0 || key_of[r - t] != key) break;
        lo = r - t;
      }
      for (int t = 1; t <= window; ++t) {
        if ((int64_t)r + t >= n_rows || key_of[r + t] != key) break;
        hi = r + t;
      }
    }
    s_seed[j] = r; s_lo[j] = lo; s_hi[j] = hi;
  }
  __syncthreads();

  for (int e = tid; e < P; e += T) {
    int32_t row = -1;
    unsigned short ds = 0xFFFF;
    if (e < n) {
      const int j = e / span, d = e - j * span - window;
      const int32_t c = s_seed[j] + d;
      if (s_seed[j] >= 0 && c >= s_lo[j] && c <= s_hi[j]) row = c;
      ds = (unsigned short)(((d < 0 ? -d : d) << 8) | j);
    }
    s_row[e] = row;
    s_ds[e] = ds;
    perm[e] = (unsigned short)e;
    head[e] = 0;
  }
  __syncthreads();

  // 1) real entries before the padding, then (row asc, dist asc, seed position asc)
  groups_sort(perm, P, [=](int a, int b) {
    const int32_t ra = s_row[a], rb = s_row[b];
    if (rb < 0) return ra >= 0 || a < b;
    if (ra < 0) return false;
    if (ra != rb) return ra < rb;
    const unsigned short da = s_ds[a], db = s_ds[b];
    if (da != db) return da < db;
    return a < b;
  });

  // 2) the first entry of a row represents it
  for (int p = tid; p < P; p += T) {
    const int e = perm[p];
    const int32_t row = s_row[e];
    if (row >= 0 && (p == 0 || s_row[perm[p - 1]] != row)) head[e] = 1;
  }
  __syncthreads();

  // 3) heads first, by (dist asc, seed position asc, row asc): two heads never share a row
  groups_sort(perm, P, [=](int a, int b) {
    const int ha = head[a], hb = head[b];
    if (!hb) return ha || a < b;
    if (!ha) return false;
    const unsigned short da = s_ds[a], db = s_ds[b];
    if (da != db) return da < db;
    return s_row[a] < s_row[b];
  });

  // 4) the first m heads, then (-inf, -1, -1, -1)
  for (int r = tid; r < m; r += T) {
    float sc = -INFINITY;
    int64_t id = -1;
    int32_t dist = -1, seed = -1;
    if (r < P) {
      const int e = perm[r];
      if (head[e]) {
        dist = s_ds[e] >> 8;
        seed = s_ds[e] & 255;
        sc = s_decay[dist];
        id = id_base + s_row[e];
      }
    }
    const size_t o = (size_t)q * m + r;
    out_sc[o] = sc;
    out_id[o] = id;
    if (out_dist) out_dist[o] = dist;
    if (out_seed) out_seed[o] = seed;
  }
}

// nq >= 1 questions of seed_stride * (2 * window + 1) <= NEIGHBORS_MAX_ENTRIES entries each; every pointer is a device
// pointer (key_of may be NULL over an empty index: no seed is valid then), out_dist / out_seed may be NULL
static int launch_neighbors(const int64_t* seeds, int64_t nq, int seed_stride, int window, const NeighborsDecay& decay,
                            const int32_t* key_of, int64_t n_rows, int64_t id_base, int m, float* out_sc, int64_t* out_id,
                            int32_t* out_dist, int32_t* out_seed, hipStream_t stream) {
  const int n = seed_stride * (2 * window + 1);
  if (window > NEIGHBORS_MAX_WINDOW || seed_stride > NEIGHBORS_MAX_SEEDS || n > NEIGHBORS_MAX_ENTRIES || m > NEIGHBORS_MAX_M)
    return fail(MRAG_ERR_UNSUPPORTED, "neighbour expansion of %d seeds at window %d to m = %d exceeds its limits", seed_stride, window, m);
  if (nq > 2147483647ll) return fail(MRAG_ERR_UNSUPPORTED, "%lld questions exceed one launch", (long long)nq);
  const int P = groups_pow2(n), T = std::min(1024, std::max(64, P / 2));
  hipLaunchKernelGGL(neighbors_kernel, dim3((unsigned)nq), dim3((unsigned)T), neighbors_lds_bytes(P), stream, seeds, seed_stride, window,
                     decay, key_of, n_rows, id_base, m, out_sc, out_id, out_dist, out_seed);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

}  // namespace mrag

using namespace mrag;

extern "C" {

int mrag_index_expand_neighbors(mrag_handle h, const int64_t* seeds, int64_t nq, int seed_stride, int seeds_is_device, int window,
                                const float* decay, int m, float* out_scores, int64_t* out_ids, int32_t* out_dist,
                                int32_t* out_seed, int out_is_device, void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  if (nq < 0) return fail(MRAG_ERR_INVALID, "nq < 0");
  if (seed_stride < 0) return fail(MRAG_ERR_INVALID, "seed_stride < 0");
  if (m < 1) return fail(MRAG_ERR_INVALID, "m must be positive");
  if (window < 0) return fail(MRAG_ERR_INVALID, "window < 0");
  if (window > NEIGHBORS_MAX_WINDOW) return fail(MRAG_ERR_UNSUPPORTED, "window = %d exceeds %d", window, NEIGHBORS_MAX_WINDOW);
  if (seed_stride > NEIGHBORS_MAX_SEEDS)
    return fail(MRAG_ERR_UNSUPPORTED, "seed_stride = %d exceeds %d seeds per question", seed_stride, NEIGHBORS_MAX_SEEDS);
  const int entries = seed_stride * (2 * window + 1);
  if (entries > NEIGHBORS_MAX_ENTRIES)
    return fail(MRAG_ERR_UNSUPPORTED, "%d seeds x (2 x %d + 1) = %d entries in one question exceed %d", seed_stride, window, entries,
                NEIGHBORS_MAX_ENTRIES);
  if (m > NEIGHBORS_MAX_M) return fail(MRAG_ERR_UNSUPPORTED, "m = %d exceeds %d", m, NEIGHBORS_MAX_M);
  if (nq == 0) return MRAG_OK;
  if (nq > (1ll << 26)) return fail(MRAG_ERR_UNSUPPORTED, "nq too large for one call; batch the questions");
  if (!decay || !out_scores || !out_ids || (seed_stride > 0 && !seeds)) return fail(MRAG_ERR_INVALID, "NULL buffer");
  NeighborsDecay dk;
  for (int d = 0; d <= NEIGHBORS_MAX_WINDOW; ++d) {
    if (d > window) { dk.v[d] = dk.v[window]; continue; }
    if (!std::isfinite(decay[d])) return fail(MRAG_ERR_INVALID, "decay[%d] is not finite", d);
    if (d > 0 && decay[d] > decay[d - 1])
      return fail(MRAG_ERR_INVALID, "decay increases at distance %d (%g -> %g)", d, (double)decay[d - 1], (double)decay[d]);
    dk.v[d] = decay[d];
  }
  const CollapseState& ck = ix->collapse;
  if (ck.n < 0 && ix->n > 0) return fail(MRAG_ERR_INVALID, "no row keys set on this index (mrag_index_set_row_keys)");
  if (ck.n >= 0 && ck.n != ix->n)
    return fail(MRAG_ERR_INVALID, "row keys were set for %lld rows, the index holds %lld: set them again", (long long)ck.n, (long long)ix->n);
  if (ix->n > 2147483647ll) return fail(MRAG_ERR_UNSUPPORTED, "%lld rows exceed the int32 rows of the expansion", (long long)ix->n);
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  NeighborsState& w = ix->neighbors;
  w.last.open();

  const size_t ns = (size_t)nq * seed_stride, no = (size_t)nq * m;
  const int64_t* d_seeds = seeds;
  if (!seeds_is_device && ns > 0) MRAG_TRY(w.seeds.ensure(ns * 8));
  float* d_sc = out_scores;
  int64_t* d_id = out_ids;
  int32_t *d_dist = out_dist, *d_seed = out_seed;
  if (!out_is_device) {                                    // (ids | scores | dist | seed), downloaded in one piece
    MRAG_TRY(w.out.ensure(no * 20));
    d_id = (int64_t*)w.out.p;
    d_sc = (float*)(d_id + no);
    d_dist = out_dist ? (int32_t*)(d_sc + no) : nullptr;
    d_seed = out_seed ? (int32_t*)(d_sc + 2 * no) : nullptr;
    w.host.resize(no * 20);
  }
  const bool host_side = (!seeds_is_device && ns > 0) || !out_is_device;
  auto enqueue = [&]() -> int {
    if (!seeds_is_device && ns > 0) {
      MRAG_HIP(hipMemcpyAsync(w.seeds.p, seeds, ns * 8, hipMemcpyHostToDevice, stream));
      d_seeds = (const int64_t*)w.seeds.p;
    }
    MRAG_TRY(launch_neighbors(d_seeds, nq, seed_stride, window, dk, (const int32_t*)ck.keys.p, ix->n, ix->id_base, m, d_sc, d_id, d_dist,
                              d_seed, stream));
    if (!out_is_device) MRAG_HIP(hipMemcpyAsync(w.host.data(), w.out.p, no * 20, hipMemcpyDeviceToHost, stream));
    return MRAG_OK;
  };
  if (host_side) MRAG_TRY(run_synced(stream, enqueue));
  else MRAG_TRY(enqueue());
  if (!out_is_device) {
    const char* hp = w.host.data();
    memcpy(out_ids, hp, no * 8);
    memcpy(out_scores, hp + no * 8, no * 4);
    if (out_dist) memcpy(out_dist, hp + no * 12, no * 4);
    if (out_seed) memcpy(out_seed, hp + no * 16, no * 4);
  }
  w.last.close(nq, entries, window);
  return MRAG_OK;
}

int mrag_index_last_neighbors(mrag_handle h, int64_t* out_questions, int64_t* out_max_entries, int64_t* out_window) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  return ix->neighbors.last.read("neighbour expansion", out_questions, out_max_entries, out_window);
}

}  // extern "C"
