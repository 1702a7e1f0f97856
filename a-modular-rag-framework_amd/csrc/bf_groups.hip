// Grouped max-merge of dense search results (mrag_index_search_groups): several query vectors that are ONE question.
// The search leaves [nq][k] (score, id) lists on the device, each in the index's declared order (score desc, id asc),
// padded with (-inf, -1); question g owns the queries group_ptr[g] .. group_ptr[g+1).  Per question:
//   drop the padding (id -1); per distinct id keep its largest score, among equal scores the lowest query position inside
//   the group; order the survivors by (score desc, id asc); write the first k as (score, id, which = that query position);
//   the slots past the distinct ids hold (-inf, -1, -1); an empty group is such a row.
// Exact: the union of the per-query top-k lists holds the top-k of the row-wise maximum over the group's queries, ties
// included (DESIGN.md §3 "Grouped queries").
//
//   grid       one workgroup per question; blockDim = half the largest question's padded size, 64 .. 1024 threads
//   LDS        dynamic, sized by the largest question of the launch; a question of n = q * k entries works on P = the power
//              of two >= n (at least 2).  Entry e = j * k + r is slot r of the group's j-th query: `which` is e / k and is
//              not stored.  The entries are staged ONCE and stay until the outputs are written:
//                id     8 P       int64, after id_base
//                score  4 P
//                perm   2 P       entry indexes, sorted twice in place
//                head   1 P       by entry: 1 = the entry that represents its id
//              15 P bytes: 7.5 KiB for a question of 2 queries at k = 200 (P = 512), 60 KiB at the limit of 4096 entries --
//              below the 64 KiB a kernel gets without raising its dynamic-LDS limit, two workgroups per 160 KiB CU.
//              Both sorts read score / id THROUGH perm, so their LDS addresses are data dependent whatever the layout; the
//              sequential accesses (staging, perm itself, head, the outputs) are unit stride per array: 4-byte and 8-byte
//              arrays conflict free, neighbouring 2-byte / 1-byte elements share a dword, which is a broadcast.
//   sort 1     bitonic over entry indexes by (real before padding, id asc, score desc, entry asc).  Scores are compared as
//              floats, never as bit patterns: -0.0 == +0.0, and the lower entry -- the lower query position -- stays in
//              front.  The first entry of an id run is the one kept.
//   heads      head[e] = 1 for the first entry of every id run
//   sort 2     bitonic over the same perm by (head before the rest, score desc, id asc)
//   output     slot r < k: the r-th entry of sort 2 if it is a head, else (-inf, -1, -1)
// Work per question: O(P log^2 P) compare-exchanges in LDS; global memory is read once and written once.  A question's
// three outputs depend on its own entries alone (P on its own n; blockDim only shares the work out).
#include "bf_index.h"

namespace mrag {

static_assert(15 * GROUPS_MAX_ENTRIES <= 65536, "the grouped merge stays inside the default dynamic-LDS limit");

static inline size_t groups_lds_bytes(int P) { return (size_t)15 * P; }

// (groups_pow2 and groups_sort, which bf_neighbors.hip uses too, are in bf_kernels.h)

__global__ __launch_bounds__(1024) void groups_merge_kernel(const float* __restrict__ in_sc, const int64_t* __restrict__ in_id,
                                                            const int64_t* __restrict__ group_ptr, int k,
                                                            float* __restrict__ out_sc, int64_t* __restrict__ out_id,
                                                            int32_t* __restrict__ out_which) {
  extern __shared__ __attribute__((aligned(16))) char groups_lds[];
  const int g = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int64_t q0 = group_ptr[g];
  const int n = (int)(group_ptr[g + 1] - q0) * k;          // <= GROUPS_MAX_ENTRIES (validated on the host)
  const int P = groups_pow2(n);
  int64_t* s_id = (int64_t*)groups_lds;
  float* s_sc = (float*)(s_id + P);
  unsigned short* perm = (unsigned short*)(s_sc + P);
  unsigned char* head = (unsigned char*)(perm + P);

  // the group's lists are consecutive: entry e is element e of in_sc / in_id behind query q0
  for (int e = tid; e < P; e += T) {
    s_id[e] = e < n ? in_id[(size_t)q0 * k + e] : (int64_t)-1;
    s_sc[e] = e < n ? in_sc[(size_t)q0 * k + e] : -INFINITY;
    perm[e] = (unsigned short)e;
    head[e] = 0;
  }
  __syncthreads();

  // 1) real entries before the padding, then (id asc, score desc, entry asc)
  groups_sort(perm, P, [=](int a, int b) {
    const int64_t ia = s_id[a], ib = s_id[b];
    if (ib == -1) return ia != -1 || a < b;
    if (ia == -1) return false;
    if (ia != ib) return ia < ib;
    const float sa = s_sc[a], sb = s_sc[b];
    if (sa > sb) return true;
    if (sa < sb) return false;
    return a < b;
  });

  // 2) the first entry of an id run represents the id
  for (int p = tid; p < P; p += T) {
    const int e = perm[p];
    const int64_t id = s_id[e];
    if (id != -1 && (p == 0 || s_id[perm[p - 1]] != id)) head[e] = 1;
  }
  __syncthreads();

  // 3) heads first, by (score desc, id asc): two heads never share an id
  groups_sort(perm, P, [=](int a, int b) {
    const int ha = head[a], hb = head[b];
    if (!hb) return ha || a < b;
    if (!ha) return false;
    const float sa = s_sc[a], sb = s_sc[b];
    if (sa > sb) return true;
    if (sa < sb) return false;
    return s_id[a] < s_id[b];
  });

  // 4) the first k heads, then (-inf, -1, -1)
  for (int r = tid; r < k; r += T) {
    float sc = -INFINITY;
    int64_t id = -1;
    int32_t which = -1;
    if (r < P) {
      const int e = perm[r];
      if (head[e]) { sc = s_sc[e]; id = s_id[e]; which = e / k; }
    }
    const size_t o = (size_t)g * k + r;
    out_sc[o] = sc;
    out_id[o] = id;
    if (out_which) out_which[o] = which;
  }
}

// n_groups >= 1 questions of at most max_entries = (largest group) * k <= GROUPS_MAX_ENTRIES entries each; every pointer
// is a device pointer, in_sc / in_id are the [nq][k] lists of a search, out_which may be NULL
static int launch_groups_merge(const float* in_sc, const int64_t* in_id, const int64_t* group_ptr, int64_t n_groups, int k, int max_entries,
                        float* out_sc, int64_t* out_id, int32_t* out_which, hipStream_t stream) {
  if (max_entries > GROUPS_MAX_ENTRIES) return fail(MRAG_ERR_UNSUPPORTED, "%d entries in one question exceed %d", max_entries, GROUPS_MAX_ENTRIES);
  if (n_groups > 2147483647ll) return fail(MRAG_ERR_UNSUPPORTED, "%lld questions exceed one launch", (long long)n_groups);
  const int P = groups_pow2(max_entries), T = std::min(1024, std::max(64, P / 2));
  const size_t lds = groups_lds_bytes(P);
  if (lds > 65536) return fail(MRAG_ERR_UNSUPPORTED, "%zu bytes of LDS for one question exceed 65536", lds);
  hipLaunchKernelGGL(groups_merge_kernel, dim3((unsigned)n_groups), dim3((unsigned)T), lds, stream, in_sc, in_id, group_ptr, k, out_sc,
                     out_id, out_which);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

// group_ptr [n_groups + 1] against the nq queries and k; *q_max = the queries of the largest question
static int groups_check_ptr(const int64_t* group_ptr, int64_t n_groups, int64_t nq, int k, int64_t* q_max) {
  MRAG_TRY(check_csr(group_ptr, n_groups, "group_ptr", "question"));
  if (group_ptr[n_groups] != nq)
    return fail(MRAG_ERR_INVALID, "group_ptr ends at %lld behind question %lld, not at nq = %lld", (long long)group_ptr[n_groups],
                (long long)n_groups - 1, (long long)nq);
  *q_max = 0;
  for (int64_t g = 0; g < n_groups; ++g) {
    const int64_t q = group_ptr[g + 1] - group_ptr[g];
    if (q * k > GROUPS_MAX_ENTRIES)
      return fail(MRAG_ERR_UNSUPPORTED, "question %lld has %lld queries x k = %d = %lld entries, more than %d", (long long)g, (long long)q,
                  k, (long long)(q * k), GROUPS_MAX_ENTRIES);
    *q_max = std::max(*q_max, q);
  }
  return MRAG_OK;
}

}  // namespace mrag

using namespace mrag;

extern "C" {

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
  int64_t q_max = 0;
  MRAG_TRY(groups_check_ptr(group_ptr, n_groups, nq, k, &q_max));
  if (allow) MRAG_TRY(check_allow_args(allow_rows, ix->n, allow_format, MRAG_FILTER_AUTO, "filter"));
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  GroupsState& w = ix->groups;
  w.last.open();

  // ---- one search of all nq queries into index-owned scratch (mrag_index_max_k is 256 for every nq: never cut)
  ListScratch in;
  MRAG_TRY(in.bind(w.in, (size_t)nq * k));
  if (nq > 0) {
    if (allow)
      MRAG_TRY(search_allowed(ix, queries, nq, q_dtype, normalize, queries_is_device, k, nullptr, allow, allow_rows, allow_format, 0,
                              MRAG_FILTER_AUTO, in.scores, in.ids, nullptr, 1, stream));
    else
      MRAG_TRY(bf_search(ix, queries, nq, q_dtype, normalize, queries_is_device, k, in.scores, in.ids, 1, stream));
  }

  // ---- one merge launch, straight into device outputs
  w.host.assign(group_ptr, group_ptr + n_groups + 1);
  MRAG_TRY(w.ptr.ensure((size_t)(n_groups + 1) * 8));
  OutTriple out;
  MRAG_TRY(out.bind(w.out, (size_t)n_groups * k, out_scores, out_ids, out_which, out_is_device, false));
  MRAG_HIP(hipMemcpyAsync(w.ptr.p, w.host.data(), (size_t)(n_groups + 1) * 8, hipMemcpyHostToDevice, stream));
  MRAG_TRY(launch_groups_merge(in.scores, in.ids, (const int64_t*)w.ptr.p, n_groups, k, (int)(q_max * k), out.scores, out.ids, out.third,
                               stream));
  MRAG_TRY(out.copy_back(stream));
  w.last.close(nq, n_groups, q_max * k);
  return MRAG_OK;
}

int mrag_index_last_groups(mrag_handle h, int64_t* out_queries, int64_t* out_groups, int64_t* out_max_entries) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  return ix->groups.last.read("search over grouped queries", out_queries, out_groups, out_max_entries);
}

}  // extern "C"
