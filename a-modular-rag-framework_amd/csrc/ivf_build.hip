// The IVF-flat index's build side: create / destroy, centroids (set, get, k-means training on the device), add with row
// growth, and the regroup of the rows by list that every search starts from.  IvfIndex is in ivf_index.h.
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
//   The (list -> queries) regrouping of step 2 runs on the device (count / plan / scatter kernels of ivf_search.hip);
//   only the workgroup count comes back to the host.
#include "ivf_index.h"

namespace mrag {

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

int ivf_gather_rows(const uint16_t* src, const int64_t* idx, int64_t n, int ld, uint16_t* dst, int zero_fill, hipStream_t stream) {
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, src, idx, n, ld, dst, zero_fill);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

// Room for `need` rows.  The new owners are filled and settled, then moved into place: a failure leaves the index as it was.
static int ivf_grow(IvfIndex* ix, int64_t need, hipStream_t stream) {
  if (need <= ix->cap) return MRAG_OK;
  int64_t cap = bf_round_rows(std::max<int64_t>(need, ix->cap + ix->cap / 2));
  DevArray<uint16_t> nr;
  DevArray<int32_t> na;
  MRAG_TRY(nr.alloc((size_t)cap * ix->ld * 2, "the IVF rows"));
  MRAG_TRY(na.alloc((size_t)cap * 4, "the IVF assignments"));
  MRAG_HIP(hipMemsetAsync(nr, 0, (size_t)cap * ix->ld * 2, stream));
  if (ix->n) {
    MRAG_HIP(hipMemcpyAsync(nr, ix->raw, (size_t)ix->n * ix->ld * 2, hipMemcpyDeviceToDevice, stream));
    MRAG_HIP(hipMemcpyAsync(na, ix->assign, (size_t)ix->n * 4, hipMemcpyDeviceToDevice, stream));
  }
  MRAG_HIP(hipStreamSynchronize(stream));
  ix->raw.swap(nr); ix->assign.swap(na); ix->cap = cap;
  return MRAG_OK;
}

BfLaunch ivf_launch(IvfIndex* ix, const uint16_t* corpus, int64_t n_rows, const void* queries, int64_t nq, hipStream_t stream) {
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

int ivf_prepare(IvfIndex* ix, const IvfRows& r, uint16_t* dst, hipStream_t stream) {
  const void* src = r.p;
  if (!r.is_device) {
    const size_t bytes = (size_t)r.n * ix->dim * dtype_size(r.dtype);
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

// The regroup.  Everything new -- the list layout, the regrouped rows, their ids, the fp8 copy -- is built beside what the
// index holds and moved into place once the stream has settled: a failure part-way leaves the index as it was.
int ivf_finalize(IvfIndex* ix, hipStream_t stream) {
  if (!ix->dirty) return MRAG_OK;
  const int64_t n = ix->n;
  std::vector<int32_t> a((size_t)n);
  if (n) MRAG_HIP(hipMemcpyAsync(a.data(), ix->assign, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
  MRAG_HIP(hipStreamSynchronize(stream));
  std::vector<int> list_count(ix->nlist, 0), list_tile_lo(ix->nlist, 0);
  for (int64_t i = 0; i < n; ++i) list_count[a[i]]++;
  int64_t tiles = 0;
  for (int l = 0; l < ix->nlist; ++l) { list_tile_lo[l] = (int)tiles; tiles += (list_count[l] + 255) / 256; }
  const int64_t ns = std::max<int64_t>(tiles, 1) * 256;
  std::vector<int64_t> perm((size_t)ns, -1);
  std::vector<int64_t> cur(ix->nlist);
  for (int l = 0; l < ix->nlist; ++l) cur[l] = (int64_t)list_tile_lo[l] * 256;
  for (int64_t i = 0; i < n; ++i) perm[cur[a[i]]++] = i;
  DevArray<uint16_t> sorted;
  DevArray<int64_t> row_ids;
  DevArray<uint8_t> sorted8;
  MRAG_TRY(sorted.alloc((size_t)ns * ix->ld * 2, "the regrouped rows"));
  MRAG_TRY(row_ids.alloc((size_t)ns * 8, "the regrouped row ids"));
  MRAG_TRY(run_synced(stream, [&]() -> int {   // (perm and the layout vectors are read by the copies)
    MRAG_HIP(hipMemcpyAsync(row_ids, perm.data(), (size_t)ns * 8, hipMemcpyHostToDevice, stream));
    MRAG_TRY(ivf_gather_rows(ix->raw ? (const uint16_t*)ix->raw : (const uint16_t*)sorted, row_ids, ns, ix->ld, sorted, 1, stream));
    if (ix->f8.on) MRAG_TRY(ivf_build_sorted8(ix, sorted, ns, sorted8, stream));
    MRAG_TRY(ix->d_list_count.ensure((size_t)ix->nlist * 4));
    MRAG_TRY(ix->d_list_tile_lo.ensure((size_t)ix->nlist * 4));
    MRAG_HIP(hipMemcpyAsync(ix->d_list_count.p, list_count.data(), (size_t)ix->nlist * 4, hipMemcpyHostToDevice, stream));
    MRAG_HIP(hipMemcpyAsync(ix->d_list_tile_lo.p, list_tile_lo.data(), (size_t)ix->nlist * 4, hipMemcpyHostToDevice, stream));
    return MRAG_OK;
  }));
  ix->sorted.swap(sorted); ix->row_ids.swap(row_ids); ix->f8.sorted8.swap(sorted8);
  ix->n_sorted = ns;
  ix->list_count.swap(list_count); ix->list_tile_lo.swap(list_tile_lo);
  ix->max_list_rows = ix->list_count.empty() ? 0 : *std::max_element(ix->list_count.begin(), ix->list_count.end());
  ix->range.inv_valid = false;
  ix->dirty = false;
  return MRAG_OK;
}

// one k-means update of the centroids from the assignments `ids` of the prepared rows x [n][ld]
static int ivf_kmeans_update(IvfIndex* ix, const uint16_t* xr, const int64_t* idp, int64_t n, hipStream_t stream) {
  MRAG_HIP(hipMemsetAsync(ix->sums.p, 0, (size_t)ix->nlist * ix->dim * 4, stream));
  MRAG_HIP(hipMemsetAsync(ix->cnts.p, 0, (size_t)ix->nlist * 4, stream));
  const dim3 g((unsigned)((n + 3) / 4)), b(256);
  const dim3 g2((unsigned)(((int64_t)ix->nlist * ix->dim + 255) / 256));
  const bool mean = ix->metric != MRAG_METRIC_COSINE;   // inner product: centroid = mean of its rows, not their sum
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
  return launch_prep_rows(ix->sums.p, MRAG_F32, ix->nlist, ix->dim, ix->cen, ix->ld, ix->dtype, ix->metric == MRAG_METRIC_COSINE, stream);
}

// nlist distinct rows of n (Floyd's sampling from splitmix64(seed)), in ascending row order
static std::vector<int64_t> ivf_pick_rows(int64_t n, int nlist, uint64_t seed) {
  std::vector<int64_t> chosen;
  uint64_t s = seed;
  for (int64_t j = n - nlist; j < n; ++j) {
    int64_t t = (int64_t)(splitmix64(s) % (uint64_t)(j + 1));
    if (std::find(chosen.begin(), chosen.end(), t) != chosen.end()) t = j;
    chosen.push_back(t);
  }
  std::sort(chosen.begin(), chosen.end());
  return chosen;
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
  ix->f8.ld8 = (int)round_up(dim, FP8_K);
  ix->nlist = nlist; ix->metric = metric; ix->dtype = storage_dtype;
  const size_t cb = (size_t)bf_round_rows(nlist) * ix->ld * 2;
  int st = ix->cen.alloc(cb, "the centroids");
  if (st == MRAG_OK) (void)hipMemset(ix->cen, 0, cb);
  for (Event* e : {&ix->ev_begin, &ix->ev_count_begin, &ix->ev_end})
    if (st == MRAG_OK) st = e->create(true);
  if (st != MRAG_OK) { delete ix; return st; }
  *out = register_object(ix);
  return MRAG_OK;
}

int mrag_ivf_destroy(mrag_handle h) { return destroy_object(h, KIND_IVF); }

int mrag_ivf_set_centroids(mrag_handle h, const void* centroids, int src_dtype, int normalize, int is_device, void* stream_) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (!centroids || !dtype_size(src_dtype)) return fail(MRAG_ERR_INVALID, "bad centroid buffer / dtype");
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
  if (!rows || !dtype_size(src_dtype)) return fail(MRAG_ERR_INVALID, "bad rows buffer / dtype");
  if (n < ix->nlist) return fail(MRAG_ERR_INVALID, "need at least nlist = %d training rows, got %lld", ix->nlist, (long long)n);
  if (ix->n) return fail(MRAG_ERR_INVALID, "train before adding rows");
  if (iters < 0) return fail(MRAG_ERR_INVALID, "iters < 0");
  MRAG_TRY(use_device(ix->device));
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t npad = bf_round_rows(n);
  DevBuf x, dpick, ids, sc;   // the prepared rows, the initial rows' numbers, the assignments and their scores
  MRAG_TRY(x.ensure((size_t)npad * ix->ld * 2));
  MRAG_TRY(dpick.ensure((size_t)ix->nlist * 8));
  MRAG_TRY(ids.ensure((size_t)n * 8));
  MRAG_TRY(sc.ensure((size_t)n * 4));
  MRAG_TRY(ix->sums.ensure((size_t)ix->nlist * ix->dim * 4));
  MRAG_TRY(ix->cnts.ensure((size_t)ix->nlist * 4));
  const std::vector<int64_t> pick = ivf_pick_rows(n, ix->nlist, seed);
  // the rows, and the initial centroids gathered from them (run_synced: the copies read the caller's rows and `pick`)
  MRAG_TRY(run_synced(stream, [&]() -> int {
    MRAG_HIP(hipMemsetAsync(x.p, 0, (size_t)npad * ix->ld * 2, stream));
    MRAG_TRY(ivf_prepare(ix, {rows, n, src_dtype, normalize, rows_is_device}, (uint16_t*)x.p, stream));
    MRAG_HIP(hipMemcpyAsync(dpick.p, pick.data(), (size_t)ix->nlist * 8, hipMemcpyHostToDevice, stream));
    return ivf_gather_rows((const uint16_t*)x.p, (const int64_t*)dpick.p, (int64_t)ix->nlist, ix->ld, ix->cen, 1, stream);
  }));
  for (int it = 0; it < iters; ++it) {
    MRAG_TRY(ivf_assign_rows(ix, (const uint16_t*)x.p, n, (int64_t*)ids.p, (float*)sc.p, stream));
    MRAG_TRY(ivf_kmeans_update(ix, (const uint16_t*)x.p, (const int64_t*)ids.p, n, stream));
  }
  MRAG_HIP(hipStreamSynchronize(stream));
  ix->has_centroids = true;
  return MRAG_OK;
}

int mrag_ivf_add(mrag_handle h, const void* rows, int64_t n, int src_dtype, int normalize, int rows_is_device, void* stream_) {
  IvfIndex* ix = (IvfIndex*)lookup(h, KIND_IVF);
  if (!ix) return MRAG_ERR_INVALID;
  if (n < 0) return fail(MRAG_ERR_INVALID, "n < 0");
  if (n == 0) return MRAG_OK;
  if (!rows || !dtype_size(src_dtype)) return fail(MRAG_ERR_INVALID, "bad rows buffer / dtype");
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
