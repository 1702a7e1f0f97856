/*
 * mrag.h -- C ABI of the MI355X-native dense-retrieval hot path (libmrag_hip.so).
 *
 * Drop-in boundary for the embedding + cosine top-k path of
 * AndyUkJ/A-Modular-RAG-Framework.  The reference is pure Python and has no FFI of
 * its own; each entry point below names the reference code it replaces
 * (paths relative to the reference checkout).  Binding a maintainer would add:
 * INTEGRATION.md (ctypes).
 *
 * Conventions
 *   - every function returns an int status: MRAG_OK (0) or a negative MRAG_ERR_*;
 *     mrag_last_error() returns a thread-local message for the last failure.
 *   - handles are opaque uint64 values; 0 is never a valid handle.
 *   - all buffers are caller-owned, plain pointers + sizes.  A pointer argument is
 *     a HOST pointer unless the matching *_is_device flag is non-zero, in which
 *     case it is a device pointer on the handle's device (e.g. a torch tensor's
 *     data_ptr()).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls
 *     with device outputs are asynchronous on that stream; calls with host outputs
 *     return after the results have landed.
 *   - one call in flight per handle (the reference is single-threaded).
 *   - there is NO CPU fallback: without a usable GPU every compute entry point
 *     fails with MRAG_ERR_NO_DEVICE.
 */
#ifndef MRAG_H_
#define MRAG_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRAG_ABI_VERSION 1

#define MRAG_OK 0
#define MRAG_ERR_INVALID (-1)     /* bad argument / bad handle */
#define MRAG_ERR_NO_DEVICE (-2)   /* no HIP device, or device index out of range */
#define MRAG_ERR_HIP (-3)         /* a HIP runtime call failed */
#define MRAG_ERR_OOM (-4)         /* device or host allocation failed */
#define MRAG_ERR_UNSUPPORTED (-5) /* valid request this build cannot serve (e.g. k too large) */

typedef uint64_t mrag_handle;

enum mrag_dtype { MRAG_F32 = 0, MRAG_F16 = 1, MRAG_BF16 = 2, MRAG_F64 = 3 };
enum mrag_metric { MRAG_METRIC_COSINE = 0, MRAG_METRIC_IP = 1 };
enum mrag_pool { MRAG_POOL_MEAN = 0, MRAG_POOL_CLS = 1 };

/* ---- library ------------------------------------------------------------------ */
int mrag_abi_version(void);
const char* mrag_last_error(void);
int mrag_device_count(int* out_count);

/* ---- a1/a2: pairwise cosine, replaces DenseReranker._cosine x N ------------------
 * app/modules/retrieval/retrieval_backend.py:192-197 (formula, zero/length guards)
 * and :245 (one query against every candidate).  fp64 on the device:
 * out[i] = dot(q, c_i) / (|q| * |c_i|), 0.0 when either norm is 0.  `cands` is
 * row-major [n, dim] fp64.  A dimension mismatch between query and candidates is the
 * caller's to map to 0.0 (the reference compares list lengths, :193). */
int mrag_cosine_f64(int device, const double* query, const double* cands, int64_t n, int dim,
                    double* out_scores, int is_device, void* stream);

/* all-pairs form (SURVEY 8f "next" rows): out[i*n+j] = cosine(x_i, x_j), fp64, same zero-norm rule.
 * Serves the semantic-edge pass of graph construction (app/modules/graph_construction/
 * edge_builder.py:146-169: per pair three norms + one dot, edge if sim >= threshold) and the
 * pairwise term of MMR (app/utils/similarity.py:33-62) in one launch instead of n^2 Python calls. */
int mrag_cosine_matrix_f64(int device, const double* x, int64_t n, int dim, double* out, int is_device, void* stream);
/* adjacent rows (embed-mode segmentation, app/modules/graph_construction/segmenter.py:32-50):
 * out[i] = dot(x_i, x_{i+1}) / (|x_i| * |x_{i+1}| + eps) for i < n-1 -- eps = 1e-9 sits INSIDE the denominator
 * there and a zero vector gives 0/eps = 0, not a special case.  Host buffers, fp64. */
int mrag_cosine_adjacent_f64(int device, const double* x, int64_t n, int dim, double eps, double* out, void* stream);

/* ---- a7 at corpus scale: brute-force cosine / inner-product top-k ----------------
 * Replaces "score every candidate, sort descending, truncate" --
 * retrieval_backend.py:245 + :371-372 (and retrieval_adapter.py:129-131) -- over the
 * whole docs.jsonl corpus (ingest row order, my_code/ingest_hotpotqa.py:73-81).
 * Rows are stored in HBM as fp16/bf16 [n, dim padded to 64]; tie-break is
 * (score desc, row id asc). */
int mrag_index_create(int dim, int metric, int storage_dtype, int device, mrag_handle* out);
int mrag_index_destroy(mrag_handle h);
int mrag_index_reserve(mrag_handle h, int64_t n_rows);
/* append n rows (row-major [n, dim] of src_dtype).  normalize != 0: L2-normalise each
 * row (fp64 norm, zero rows stay zero -> cosine 0.0 like :197) before rounding once to
 * the storage dtype; normalize == 0: rows are rounded/stored as given. */
int mrag_index_add(mrag_handle h, const void* rows, int64_t n, int src_dtype, int normalize,
                   int rows_is_device, void* stream);
int mrag_index_size(mrag_handle h, int64_t* out_rows);
int mrag_index_dim(mrag_handle h, int* out_dim);
/* ids reported by search = id_base + local row (row-sharded corpora) */
int mrag_index_set_id_base(mrag_handle h, int64_t id_base);
/* copy stored (rounded) rows [row0, row0+n) back as fp32 [n, dim] -- for tests/caches */
int mrag_index_get_rows(mrag_handle h, int64_t row0, int64_t n, float* out, int out_is_device, void* stream);
/* largest k mrag_index_search serves for a batch of nq queries (256: the reference's dense pool is 200
 * candidates per question, config/settings.yaml:101-102 / retrieval_backend.py:218,276).  k <= 64 runs
 * the fused batch kernel; 64 < k <= 256 runs the streaming kernel 8 queries per launch (exact, HBM-bound) for up
 * to 32 queries, and for larger batches the batch kernel at k' = 64 per corpus split + merge + an exactness check,
 * with the few queries the check flags redone by the streaming kernel (such a search synchronises the stream once). */
int mrag_index_max_k(int64_t nq, int* out_k);
/* measurement hook: queries the LAST 64 < k <= 256 batch search (any index of this process) had to redo through the
 * streaming kernel because one corpus split held more than 64 of their true top k (0 for every other kind of search). */
int mrag_index_last_wide_redone(int64_t* out_queries);
/* top-k of every query against every stored row.  out_scores [nq,k] fp32 descending,
 * out_ids [nq,k] int64; slots past the corpus size hold (-inf, -1).  k > mrag_index_max_k:
 * MRAG_ERR_UNSUPPORTED (never a silent clamp). */
int mrag_index_search(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize,
                      int queries_is_device, int k, float* out_scores, int64_t* out_ids,
                      int out_is_device, void* stream);
/* Filtered search: the top-k of the ALLOWED rows only (restrict to a set of documents, a tenant or a date range, leave
 * out passages already shown; the reference's DenseReranker.score scores a candidate pool, retrieval_backend.py:215-247).
 * `allow` is an allow-set over the local rows 0 .. size-1 (before id_base): MRAG_ALLOW_BITS32 = uint32 words, bit r%32
 * of word r/32 (ceil(size/32) words); MRAG_ALLOW_BYTES = one byte per row, nonzero = allowed (packed to bits on the
 * device).  allow_rows must equal the index size.  Order, k limits and the (-inf, -1) tail as mrag_index_search: slots
 * past the number of allowed rows are (-inf, -1); no allowed row gives an all-(-inf, -1) result.  An all-allowed set
 * returns exactly what mrag_index_search returns.
 * path: MRAG_FILTER_MASK scores every row and drops the disallowed ones inside the search kernels (no extra memory);
 * MRAG_FILTER_COMPACT gathers the allowed rows into an index-owned scratch corpus and searches only those (work
 * proportional to the allowed rows); MRAG_FILTER_AUTO picks one from (nq, k, size, allowed rows, dim).
 * Sync behaviour with device outputs: a HOST allow-set is counted on the host, so AUTO and both paths stay
 * asynchronous on `stream` (the mask itself is copied to the device before the call returns).  With a DEVICE allow-set,
 * MRAG_FILTER_MASK is fully asynchronous (capturable); AUTO and MRAG_FILTER_COMPACT read the allowed-row count back
 * once (one stream synchronisation).  The wide path (64 < k <= 256, more than 32 queries) synchronises once as in
 * mrag_index_search.  Host outputs: the call returns after the results have landed. */
enum mrag_filter_path { MRAG_FILTER_AUTO = 0, MRAG_FILTER_MASK = 1, MRAG_FILTER_COMPACT = 2 };
enum mrag_allow_format { MRAG_ALLOW_BITS32 = 0, MRAG_ALLOW_BYTES = 1 };
int mrag_index_search_filtered(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize,
                               int queries_is_device, int k, const void* allow, int64_t allow_rows, int allow_format,
                               int allow_is_device, int path, float* out_scores, int64_t* out_ids, int out_is_device,
                               void* stream);
/* path the LAST filtered search on this handle took (MRAG_FILTER_MASK / MRAG_FILTER_COMPACT) and its allowed-row count.
 * Blocks until that search is done when the count is still on the device (device allow-set, MRAG_FILTER_MASK). */
int mrag_index_last_filter(mrag_handle h, int* out_path, int64_t* out_allowed);
/* Range search: the rows scoring >= min_score ("every passage with cosine >= t"), with an exact count.  Per query, with c =
 * the number of searched rows whose score is >= min_score (inclusive): out_scores / out_ids hold the best min(k, c) of them,
 * (score desc, row asc), ids = id_base + row; the slots after them are (-inf, -1); out_counts[q] = c exactly (int64, in the
 * memory space of the other outputs), so a query is truncated when out_counts[q] > k.  The score is the one the plain search
 * computes (fp32 accumulation over the stored 16-bit row and the prepared query), and the search is exact in every regime.
 * min_score must be finite (NaN / +-inf: MRAG_ERR_INVALID); 1 <= k <= mrag_index_max_k.  A floor below every score
 * returns exactly what mrag_index_search (or, with an allow-set, mrag_index_search_filtered) returns, with counts = the
 * searched rows; a floor above every score returns all (-inf, -1) and zero counts.
 * allow == NULL searches every row; otherwise allow, allow_rows, allow_format, allow_is_device and filter_path are those of
 * mrag_index_search_filtered (same AUTO rule, same record for mrag_index_last_filter).  Sync behaviour, streams, host and
 * device outputs and mrag_index_last_timing as mrag_index_search / mrag_index_search_filtered.  The fp8 scan copy has no
 * range mode. */
int mrag_index_search_range(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device,
                            int k, float min_score, const void* allow, int64_t allow_rows, int allow_format, int allow_is_device,
                            int filter_path, float* out_scores, int64_t* out_ids, int64_t* out_counts, int out_is_device,
                            void* stream);
/* fp8 scan copy + exact re-rank (cosine indexes).  mrag_index_enable_fp8 keeps, next to the 16-bit rows, an OCP e4m3fn
 * copy rows8 [capacity][ld8], ld8 = dim rounded up to 128: byte (r, c) = e4m3fn(clamp(256 * x, -448, 448)), x the STORED
 * 16-bit value of row r (exact in fp32), rounded to nearest even; pad rows and pad columns are 0.  |x| <= 1 for unit rows,
 * so 256 * x fills the normal range without overflow.  The copy is built from the rows already stored when it is enabled
 * (the call synchronises the device; idempotent) and kept current by every later add and reserve; it costs ld8 bytes per
 * row of capacity.  A non-cosine index gets MRAG_ERR_INVALID.
 * mrag_index_search_fp8: 1 <= k <= 64 and k <= refine <= 64 (refine = 0: mrag_index_fp8_default_refine(k) =
 * min(64, max(40, 4k))); anything else, or an index without the copy, is MRAG_ERR_INVALID.  Each query is prepared as in
 * mrag_index_search (normalize, rounding to the storage dtype) and quantised with its own power of two 2^e, chosen so
 * that max |q * 2^e| lies in [128, 256) (a zero query stays zero).  The top-`refine` rows by fp8 score (block-scaled
 * MFMA, fp32 accumulation) are the candidates; up to 16 queries take the streaming kernel, more the batch kernel.  The
 * candidates are then re-scored exactly: fp32 dot product of the prepared 16-bit query with the stored 16-bit row, so
 * the returned scores are exact-path scores (equal to the plain search's up to fp32 summation order), never fp8 scores.
 * Output: the k best candidates by that score, (score desc, row asc), ids = id_base + row; slots past the candidates
 * found (fewer than k rows) are (-inf, -1).  The result is approximate only in WHICH rows are returned: a true top-k row
 * that the fp8 ranking leaves outside the refine pool is missed.  Sync behaviour as mrag_index_search.
 * mrag_index_get_rows_fp8: bytes of rows [row0, row0 + n) as [n, dim] uint8 (tests).  mrag_index_last_fp8: refine and
 * regime of the last fp8 search on the handle.  mrag_index_last_timing covers fp8 searches too: gemm = the fp8 candidate
 * kernel(s), total = the whole call. */
enum mrag_fp8_regime { MRAG_FP8_BATCH = 0, MRAG_FP8_STREAM = 1 };
int mrag_index_enable_fp8(mrag_handle h);
int mrag_index_get_rows_fp8(mrag_handle h, int64_t row0, int64_t n, uint8_t* out, int out_is_device, void* stream);
int mrag_index_fp8_default_refine(int k, int* out);
int mrag_index_search_fp8(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device,
                          int k, int refine, float* out_scores, int64_t* out_ids, int out_is_device, void* stream);
int mrag_index_last_fp8(mrag_handle h, int* out_refine, int* out_regime);
/* the re-ranker's candidate lookup by row id.  Replaces the 1 + ceil(N/bs) embed calls +
 * N x _cosine of DenseReranker.score (retrieval_backend.py:227-245) for candidates whose rows are already
 * in the index: out_scores[i] = <query, stored row row_ids[i]> (the cosine when rows and query are
 * normalised); an id outside [0, size) scores 0.0 like an unusable vector (:193-197).  Host buffers. */
int mrag_index_score_rows(mrag_handle h, const void* query, int q_dtype, int normalize, const int64_t* row_ids,
                          int64_t n, float* out_scores, void* stream);
/* The same lookup for a batch of questions in one launch: mrag_rerank_batch.h, included below. */
/* timing hooks for bench.py: device time in ms of the dominant kernel (fused similarity
 * GEMM + top-k) and of the whole search of the LAST mrag_index_search call, measured with
 * hipEvents on the stream the kernels were launched on.  Blocks until that call is done. */
int mrag_index_last_timing(mrag_handle h, float* out_gemm_ms, float* out_total_ms);
/* held shader clock under the fused kernel (SURVEY 8d "record held clock"): with the reading enabled, workgroup 0
 * of the batch kernel stamps s_memtime / s_memrealtime at entry and exit; last_clock = d(cycles) / d(100 MHz ticks).
 * MRAG_ERR_UNSUPPORTED when the last search ran the streaming kernel (no stamps). */
int mrag_index_measure_clock(mrag_handle h, int enable);
int mrag_index_last_clock(mrag_handle h, float* out_ghz);

/* ---- 8e: host-side merge of per-shard partial top-k ------------------------------
 * scores [nparts, nq, k] fp32 and ids [nparts, nq, k] int64 (ids < 0 = empty slot), as
 * gathered by the RCCL all-gather.  Result ordered by (score desc, id asc). */
int mrag_topk_merge(const float* scores, const int64_t* ids, int nparts, int64_t nq, int k,
                    float* out_scores, int64_t* out_ids, int nthreads);

/* the same merge for buffers that already sit in HBM (the RCCL all-gather output): every pointer is a
 * device pointer on `device`, asynchronous on `stream`.  Each part must be sorted (score desc, id asc)
 * with its empty slots last, as mrag_index_search produces them.  Serves nparts <= 64 and
 * nparts * k <= 2048; larger requests return MRAG_ERR_UNSUPPORTED (use the host merge). */
int mrag_topk_merge_device(int device, const float* scores, const int64_t* ids, int nparts, int64_t nq, int k,
                           float* out_scores, int64_t* out_ids, void* stream);
/* the exchange's packed form (ONE all-gather of 8-byte words): word = (fp32 score bits << 32) | shard-local row
 * (id - id_base as 32 bits; 0xFFFFFFFF = empty slot).  pack: n = nq * k device entries -> words; an id outside
 * [id_base, id_base + 2^32 - 1) ORs 1 into *bad_flag (device int, may be NULL) -- nothing is wrapped silently.
 * merge_packed: the gathered words [nparts, nq, k] + the parts' first global rows bases[nparts] (device) -> [nq, k], same order
 * and limits as mrag_topk_merge_device (the words are unpacked on their way into LDS: no pass over the gathered buffer). */
int mrag_pack_partial_device(int device, const float* scores, const int64_t* ids, int64_t n, int64_t id_base,
                             int64_t* words, int* bad_flag, void* stream);
int mrag_topk_merge_packed_device(int device, const int64_t* words, const int64_t* bases, int nparts, int64_t nq, int k,
                                  float* out_scores, int64_t* out_ids, void* stream);

/* ---- IVF-flat (BASELINE.json config 5; no counterpart in the reference) ----------- */
int mrag_ivf_create(int dim, int nlist, int metric, int storage_dtype, int device, mrag_handle* out);
int mrag_ivf_destroy(mrag_handle h);
/* spherical k-means on the device, seeded: init = rows picked by the host from `seed` */
int mrag_ivf_train(mrag_handle h, const void* rows, int64_t n, int src_dtype, int normalize,
                   int rows_is_device, int iters, uint64_t seed, void* stream);
int mrag_ivf_set_centroids(mrag_handle h, const void* centroids, int src_dtype, int normalize,
                           int is_device, void* stream);
int mrag_ivf_get_centroids(mrag_handle h, float* out, int out_is_device, void* stream);
int mrag_ivf_add(mrag_handle h, const void* rows, int64_t n, int src_dtype, int normalize,
                 int rows_is_device, void* stream);
int mrag_ivf_size(mrag_handle h, int64_t* out_rows);
int mrag_ivf_set_id_base(mrag_handle h, int64_t id_base);
/* list id of every stored row, in insertion order */
int mrag_ivf_get_assignments(mrag_handle h, int32_t* out, int out_is_device, void* stream);
/* top-k over the `nprobe` nearest lists of every query (nprobe 1..256, or nlist = exhaustive); k <= 64.
 * Order and tie-break as mrag_index_search: (score desc, original row asc); missing entries (-inf, -1).
 * With queries AND results in device memory the call is asynchronous on `stream`; with host buffers it
 * returns when they are complete.  Batches are cut internally so that a chunk's fp32 score segments fit the
 * score buffer (MRAG_IVF_SCORES_MB, default 4096; 0 = always the fused GEMM + top-k kernel). */
int mrag_ivf_search(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize,
                    int queries_is_device, int nprobe, int k, float* out_scores, int64_t* out_ids,
                    int out_is_device, void* stream);
/* Filtered IVF search: the same allow-set contract as mrag_index_search_filtered.  `allow` covers the local rows 0 .. size-1
 * in insertion order, before id_base (MRAG_ALLOW_BITS32 or MRAG_ALLOW_BYTES, host or device, allow_rows == size).  Results:
 * (score desc, original row asc), ids = row + id_base, slots past the allowed candidates (-inf, -1); k <= 64, nprobe as
 * mrag_ivf_search.
 *   MRAG_IVF_FILTER_PROBE (path P, filter-aware probing): a list is LIVE when it holds at least one allowed row.  Every
 *     query probes its `nprobe` best live lists, ranked by (centroid score desc, list id asc); a list without an allowed
 *     row is never probed.  The result is the top-k of the allowed rows of those lists.  With fewer than nprobe live
 *     lists all of them are probed, and the answer is exactly the filtered brute-force one.
 *     When every list holds at least one row, an all-allowed set gives exactly what mrag_ivf_search gives (scores and ids).
 *     An EMPTY list (k-means can leave one) is dead under any allow-set: P probes the next live list in its place, while
 *     mrag_ivf_search spends a probe on it -- there P can find more rows than the plain search.
 *   MRAG_IVF_FILTER_EXACT (path E): the top-k over all allowed rows = filtered brute force (the dense filtered search over
 *     the rows in insertion order).  nprobe == nlist always runs E; so does a P search whose score segments would not fit
 *     the score buffer (MRAG_IVF_SCORES_MB, 0 included), as the fused list-scan kernel has no filtered form.
 *   MRAG_IVF_FILTER_AUTO: E when the allowed rows are few enough that scanning them all costs less than the probed scan
 *     (mrag_ivf_choose_filter_path).  Where AUTO picks E the answer can only improve on P.
 * list_allowed (optional, NULL = computed from `allow`): allowed rows per list [nlist] int32, in the memory space of
 * `allow`; only path P reads it, to decide which lists are live.  A sharded index passes the counts summed over its ranks,
 * so that every rank probes the same lists.
 * Sync behaviour: a HOST allow-set is counted on the host and the call stays asynchronous (with device queries and
 * outputs); with a DEVICE allow-set AUTO and E read the allowed count back once, forced P stays asynchronous on `stream`.
 * Host queries or outputs: the call returns after the results have landed. */
enum mrag_ivf_filter_path { MRAG_IVF_FILTER_AUTO = 0, MRAG_IVF_FILTER_PROBE = 1, MRAG_IVF_FILTER_EXACT = 2 };
int mrag_ivf_search_filtered(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device,
                             int nprobe, int k, const void* allow, int64_t allow_rows, int allow_format, int allow_is_device,
                             const int32_t* list_allowed, int path, float* out_scores, int64_t* out_ids, int out_is_device,
                             void* stream);
/* allowed rows per list of an allow-set (formats and sizes as above) -> out_counts [nlist] int32 (host or device) */
int mrag_ivf_allowed_per_list(mrag_handle h, const void* allow, int64_t allow_rows, int allow_format, int allow_is_device,
                              int32_t* out_counts, int out_is_device, void* stream);
/* AUTO's rule, handle-free (no GPU needed): E when nprobe >= nlist or allowed_rows <= c * nprobe * total_rows / nlist, with
 * c measured per regime (a few queries / a batch).  A sharded caller applies it to the global counts and passes the
 * explicit path to every rank.  *out_path = MRAG_IVF_FILTER_PROBE or MRAG_IVF_FILTER_EXACT. */
int mrag_ivf_choose_filter_path(int64_t nq, int k, int nprobe, int nlist, int64_t total_rows, int64_t allowed_rows, int dim,
                                int* out_path);
/* path (PROBE / EXACT), allowed rows and live lists of the LAST filtered search on this handle; live lists is -2 when the
 * search ran path E (lists are not consulted there).  Blocks until that search is done when a figure is still on the device. */
int mrag_ivf_last_filter(mrag_handle h, int* out_path, int64_t* out_allowed, int* out_live_lists);
/* Range search over the probed lists (the IVF form of mrag_index_search_range; serves the semantic_sim edge pass,
 * edge_builder.py:146-169: every pair of rows with cosine >= a threshold, at corpus sizes where the exact join is too slow).
 * Per query, over the rows of its `nprobe` probed lists ONLY (probe selection as mrag_ivf_search), with c = the number of
 * those rows whose fp32 score is >= min_score (inclusive): out_scores / out_ids hold the best min(k, c) of them, (score desc,
 * original row asc), ids = row + id_base; the slots after them are (-inf, -1); out_counts[q] = c exactly (int64, in the memory
 * space of the other outputs).  c is a lower bound of the dense index's count and equals it when every list is probed.
 * The scores are the ones mrag_ivf_search returns; a floor below every score returns exactly its result.
 * exclude_rows (optional, NULL = none): int64 [nq] in host or device memory (exclude_is_device), a LOCAL row (before id_base)
 * per query or -1.  That row is neither listed nor counted; other rows with the same values stay.  A host value outside
 * [-1, size) is MRAG_ERR_INVALID; a device value outside [0, size) means none.
 * 1 <= k <= 256, min_score finite, nprobe as mrag_ivf_search (MRAG_ERR_INVALID otherwise).  The search runs in the
 * score-segment regime only: with more than 256 probed lists per query (nprobe = nlist > 256), with MRAG_IVF_SCORES_MB = 0,
 * or when the score segments of one chunk exceed the score buffer it returns MRAG_ERR_UNSUPPORTED and writes no answer.
 * There is no allow-set form.  Batches are cut into chunks as in mrag_ivf_search; sync behaviour as there (device queries,
 * device exclude_rows or none, and device outputs: asynchronous on `stream`). */
int mrag_ivf_search_range(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device,
                          int nprobe, int k, float min_score, const int64_t* exclude_rows, int exclude_is_device,
                          float* out_scores, int64_t* out_ids, int64_t* out_counts, int out_is_device, void* stream);
/* Neighbour join (edge_builder.py:146-169 over an indexed corpus): the stored rows [row0, row0 + n) as the queries of
 * mrag_ivf_search_range, each excluding itself (exclude = row0 + i).  The rows are taken device to device from the index's
 * copy in insertion order, in the storage dtype as stored: no normalisation, no fp32 round trip.  Outputs are device
 * buffers [n][k], [n][k], [n]; asynchronous on `stream`.  Limits and refusals as mrag_ivf_search_range. */
int mrag_ivf_self_join(mrag_handle h, int64_t row0, int64_t n, int nprobe, int k, float min_score,
                       float* out_scores, int64_t* out_ids, int64_t* out_counts, void* stream);
/* fp8 scan copy + exact re-rank over the probed lists (cosine indexes): the contract of mrag_index_search_fp8, applied to
 * the rows of the probed lists.  mrag_ivf_enable_fp8 keeps, next to the regrouped 16-bit rows the list scan streams, an OCP
 * e4m3fn copy [stored positions][ld8], ld8 = dim rounded up to 128: byte = e4m3fn(clamp(256 * x, -448, 448)), x the STORED
 * 16-bit value, rounded to nearest even; pad rows and pad columns are 0.  It is rebuilt wherever the rows are regrouped (the
 * first search after an add), and built once by the call itself when rows are already there (the call synchronises the
 * device; idempotent); it costs ld8 bytes per stored position.  A non-cosine index gets MRAG_ERR_INVALID.
 * mrag_ivf_search_fp8: 1 <= k <= 64 and k <= refine <= 64 (refine = 0: mrag_index_fp8_default_refine(k)); anything else, or
 * an index without the copy, is MRAG_ERR_INVALID.  Probe selection is that of mrag_ivf_search (16-bit centroids): the same
 * lists are probed.  Each query is prepared as in mrag_ivf_search and quantised with its own power of two 2^e, max
 * |q * 2^e| in [128, 256) (a zero query stays zero).  The top-`refine` rows of the query's probed lists by fp8 score
 * (block-scaled MFMA, fp32 accumulation) are the candidates; each is re-scored as the fp32 dot product of the prepared
 * 16-bit query with the stored 16-bit row.  Output: the k best by that score, (score desc, original row asc), ids = row +
 * id_base; slots past the candidates are (-inf, -1).  Returned scores are never fp8 scores; the result is approximate only
 * in WHICH rows are returned, and equals mrag_ivf_search's (up to fp32 summation order) when a query's probed lists hold
 * at most `refine` rows.  The search runs in the score-segment regime only: with more than 256 probed lists per query
 * (nprobe = nlist > 256), with MRAG_IVF_SCORES_MB = 0, or when the score segments of one chunk exceed the score buffer it
 * returns MRAG_ERR_UNSUPPORTED and writes no answer.  There is no allow-set form and no range form.  Batches are cut into
 * chunks as in mrag_ivf_search; sync behaviour as there (device queries and device outputs: asynchronous on `stream`).
 * mrag_ivf_get_rows_fp8: fp8 bytes of the original rows [row0, row0 + n), in insertion order, as [n, dim] uint8, read from
 * the regrouped copy through the row -> position map (regroups first if rows were added; for the tests).
 * mrag_ivf_last_fp8: refine of the last fp8 search on the handle. */
int mrag_ivf_enable_fp8(mrag_handle h);
int mrag_ivf_get_rows_fp8(mrag_handle h, int64_t row0, int64_t n, uint8_t* out, int out_is_device, void* stream);
int mrag_ivf_search_fp8(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int queries_is_device,
                        int nprobe, int k, int refine, float* out_scores, int64_t* out_ids, int out_is_device, void* stream);
int mrag_ivf_last_fp8(mrag_handle h, int* out_refine);
/* measurement hooks for bench.py (like mrag_index_last_timing): device ms of the list scan (scan + per-query selection kernels, or the fused kernel) and of the
 * whole LAST mrag_ivf_search, mrag_ivf_search_filtered, mrag_ivf_search_range, mrag_ivf_self_join or mrag_ivf_search_fp8 (hipEvents on its stream; filtered: the
 * list scan + selection on path P, the search kernel on path E; fp8: the fp8 scan + the candidate selection, the total covers the query quantisation and the
 * re-rank too), the rows that scan streamed (sum over its
 * workgroups of their list's length: x ld x 2 = the algorithmic HBM bytes; x ld8 for an fp8 search) and its workgroup count. */
int mrag_ivf_last_timing(mrag_handle h, float* out_scan_ms, float* out_total_ms, int64_t* out_scanned_rows, int* out_n_wg);

/* ---- a5: sentence-encoder forward, fills the LLMProvider.embed slot ---------------
 * app/core/providers/base.py:6, called as embed(model=, texts=, require=) from
 * app/core/llm_router.py:115.  BERT-family encoder (MiniLM-L6 / bge-base shapes,
 * SURVEY 8c): embeddings + LayerNorm, L x {MHA, erf-GELU FFN, post-LN}, pooling,
 * optional L2 normalisation.  Tokenisation stays on the host. */
typedef struct mrag_encoder_config {
  int32_t vocab_size;
  int32_t hidden;
  int32_t layers;
  int32_t heads;
  int32_t intermediate;
  int32_t max_position;
  int32_t type_vocab_size;
  float layer_norm_eps;
  int32_t compute_dtype; /* MRAG_F16 or MRAG_BF16 */
} mrag_encoder_config;

int mrag_encoder_create(const mrag_encoder_config* cfg, int device, mrag_handle* out);
int mrag_encoder_destroy(mrag_handle h);
/* upload one named fp32 parameter (HF BertModel state_dict names, e.g.
 * "embeddings.word_embeddings.weight", "encoder.layer.3.attention.self.query.bias") */
int mrag_encoder_set_param(mrag_handle h, const char* name, const float* data, int64_t numel,
                           int is_device, void* stream);
/* number of parameters still missing (0 = ready) */
int mrag_encoder_missing_params(mrag_handle h, int* out_missing);
/* ids/mask int32 [B,S]; out fp32 [B,hidden] */
int mrag_encoder_forward(mrag_handle h, const int32_t* ids, const int32_t* mask, int B, int S,
                         float* out, int pool, int normalize, int io_is_device, void* stream);
/* measurement hook for bench.py: device ms of the LAST forward's kernels (embeddings .. pooling), from
 * hipEvents on its stream; the ids/mask H2D and the output D2H are outside the bracket. */
int mrag_encoder_last_timing(mrag_handle h, float* out_ms);

/* ---- 8f-3: the BM25 text channel on the device -------------------------------------
 * Replaces BM25LiteIndex.search (app/modules/retrieval/text_index.py:59-97: per candidate document
 * _score_doc over the query tokens, max / sum merge over the expanded queries, sort descending, top_k) and
 * feeds the fusion of retrieval_backend.py:353-372.  The index is built on the host exactly like
 * text_index.py:36-52 (same tokeniser, tf / df / doc_lens / avgdl) and uploaded as CSR postings:
 *   indptr[n_terms+1], post_doc[nnz] (ascending inside a term), post_tf[nnz],
 *   doc_norm[d] = k1 * (1 - b + b * dl_d / avgdl)   (the length term of :66), k1_plus_1 = k1 + 1.
 * search: n_queries token lists (q_ptr[n_queries+1] into q_terms / q_idf; a token outside the vocabulary is
 * id -1; q_idf = the reference's _idf of that token, :54-56).  fp64 throughout; a document's score is the
 * reference's left-to-right sum bit for bit.  merge_sum = 0: max over the queries (alpha_merge="max"), 1: sum.
 * Output: out_n <= k (doc, score) pairs, (score desc, doc asc), scores > 0 only.  Host buffers of k slots; the
 * slots past out_n are overwritten with (-1, 0.0). */
int mrag_bm25_create(int device, int64_t n_docs, int64_t n_terms, const int64_t* indptr, const int32_t* post_doc,
                     const int32_t* post_tf, const double* doc_norm, double k1_plus_1, mrag_handle* out);
int mrag_bm25_destroy(mrag_handle h);
int mrag_bm25_search(mrag_handle h, int n_queries, const int32_t* q_ptr, const int32_t* q_terms, const double* q_idf,
                     int merge_sum, int k, int64_t* out_docs, double* out_scores, int* out_n, void* stream);
/* The same search for a batch of questions, optionally over an allow-set of documents: mrag_bm25_batch.h, included below. */

/* a7 on the device: the fusion arithmetic of HybridRetrievalBackend.run (retrieval_backend.py:336-372).
 * keys / scores hold the text, graph and dense channel entries back to back (n_text, n_graph, n_dense); a key is
 * the rank of the hit's NORMALISED id (:283-294) among all ids of the call, so ascending key = ascending id.
 * Per channel: dedupe by key (strictly larger score wins, :336-348), min-max (:296-301); union:
 * alpha_t*ts + alpha_g*gs + alpha_d*ds (:363); order (score desc, key asc); top_k (:371-372).  fp64, the
 * reference's values bit for bit.  Outputs (host, length >= min(top_k, entries)): key, fused score and the three
 * score_*_norm values per kept hit; *out_n = hits written, the slots past it up to that length are overwritten with
 * key -1 and 0.0.  At most 4096 entries. */
int mrag_fuse_topk(int device, const int32_t* keys, const double* scores, int n_text, int n_graph, int n_dense,
                   double alpha_text, double alpha_graph, double alpha_dense, int top_k, int32_t* out_keys,
                   double* out_scores, double* out_text_norm, double* out_graph_norm, double* out_dense_norm,
                   int* out_n, void* stream);
/* The same fusion for a batch of questions in one launch: mrag_fuse_batch.h, included below. */

#ifdef __cplusplus
}
#endif

/* Additions to the ABI since its 64 entry points: each in a header of its own, part of this one. */
#include "mrag_bm25_batch.h"
#include "mrag_fuse_batch.h"
#include "mrag_rerank_batch.h"
#include "mrag_filter_batch.h"
#include "mrag_search_groups.h"
#include "mrag_search_collapsed.h"
#include "mrag_neighbors.h"

#endif /* MRAG_H_ */
