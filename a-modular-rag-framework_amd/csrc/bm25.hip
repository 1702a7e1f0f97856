// BM25 text channel on the device: the reference's BM25LiteIndex.search
// (app/modules/retrieval/text_index.py:59-97) over CSR postings resident in HBM, for MANY questions per call, each with
// its own expanded queries, optionally restricted to an allow-set of documents.  There is one search path:
// mrag_bm25_search_batch runs it for its questions, mrag_bm25_search is a batch of one question without an allow-set.
//
//   reference                                   here
//   tf: term -> {doc: tf}        (:27,45-47)    CSR: indptr[term], post_doc[], post_tf[] (docs ascending)
//   _idf(term)                   (:54-56)       computed by the HOST binding with the reference's own expression
//                                               (math.log) and passed per query token: bit-identical
//   _score_doc: for t in q_terms (:59-69)       one launch per token POSITION j: every query's j-th token scatters
//     score += idf*(f*(k1+1))/(f+K(doc))        its postings into that query's dense fp64 score row -- a document
//                                               receives its contributions in token order, exactly the reference's
//                                               left-to-right fp64 sum (same IEEE operations, no contraction)
//   merge over queries: max | sum (:90-91)      bm25_merge_kernel, a question's queries in order
//   keep s > 0, sort desc, [:top_k] (:92-96)    MSB-first radix select over (score bits, ~doc) + rank by counting:
//                                               (score desc, doc asc) -- the reference's tie order is the iteration
//                                               order of a set of ints; doc-ascending is this library's declared order
//
//   chunk      questions are taken in order while their expanded queries fit the score-row scratch (one fp64 row of n_docs
//              per expanded query; mrag_bm25_set_scratch_limit), at most 65 535 rows (a job is a grid row in y) and at
//              most BM25_CHUNK_QUESTIONS questions that have a query.  A question is never split: one with more rows than
//              the limit allows gets a chunk of its own.  A question without queries needs no row and no launch.
//   scatter    one launch per token position: y = the (row, position) jobs of the whole chunk, x covers the longest range
//   merge      y = question: max / sum over its rows in query order, s > 0 ? s : 0, 0 for a document outside the allow-set;
//              the merged row is written over the question's FIRST score row (a thread owns its document: in place is safe),
//              so the scratch is exactly one row per expanded query
//   select     y = question: MSB-first radix select over (score bits, ~doc) with per-question histograms and counters;
//              every workgroup rebuilds the selection state from the earlier passes' histograms with a 256-thread suffix
//              scan per pass (not a one-thread walk: with a grid of 1024 x questions workgroups the walk would cost more
//              than the documents), a question whose bucket is settled reads no document again
//   rank       y = question: rank by counting into the call's result buffer [n_questions][k]
// The selection kernels (bm25_hist_kernel, bm25_gather_kernel) launch at most 1024 workgroups of 256 threads in x: one sweep
// covers 1024 * 256 = 262 144 documents and a larger corpus is covered by their grid-stride loops, so a corpus above
// 262 144 documents is the first at which those loops take a second iteration (tests/test_gpu_text_channel.py, "stride").
// Launches per chunk: longest token list + 15 (merge, 12 histogram passes, gather, rank) and two memsets, whatever the
// number of questions.  The plan of every chunk (jobs, question descriptors) is built on the host and uploaded ONCE per
// call; the results of the whole call sit in one device buffer and come back after ONE stream synchronisation per call.
// HBM-bound integer/byte work.  Bytes per question with q expanded queries over N documents: 8 N q (row memset) + 8 + 16
// per posting (scatter) + 8 N q + 8 N (merge) + 8 N per histogram pass that still has a bucket to split + 8 N (gather).
#include "common.h"

#include <algorithm>
#include <vector>

namespace mrag {

constexpr int64_t BM25_DEFAULT_SCRATCH = 1ll << 30;   // score rows of one chunk (mrag_bm25_batch.h: not a measured optimum)
constexpr int BM25_MAX_K = 4096;
constexpr int BM25_MAX_QUERIES = 1024;       // expanded queries of one question
constexpr int BM25_PASSES = 12;              // 8 bytes of score bits + 4 bytes of ~doc
constexpr int BM25_CHUNK_QUESTIONS = 1024;   // questions with a query per chunk: bounds the selection state (12 KiB + 16 k bytes each)
constexpr unsigned BM25_GRID_YZ = 65535;     // HIP's limit of gridDim.y / gridDim.z

struct Bm25Index : Object {
  int64_t n_docs = 0, n_terms = 0, nnz = 0;
  double k1p1 = 2.5;
  DevArray<int64_t> indptr;      // [n_terms + 1]
  DevArray<int32_t> post_doc;    // [nnz]
  DevArray<int32_t> post_tf;     // [nnz]
  DevArray<double> doc_norm;     // [n_docs]  k1 * (1 - b + b * dl / avgdl)
  std::vector<int64_t> h_indptr; // host copy: posting counts size the launches
  int64_t scratch_limit = BM25_DEFAULT_SCRATCH;
  DevBuf scores, plan, hist, sel, out, allow;   // one call in flight per handle
};

struct Bm25Job { int64_t lo, hi; double idf; int32_t query; int32_t pad; };   // one (score row, token position) posting range
struct Bm25Group { int32_t row0, n_rows, question, pad; };   // one question of a chunk: its score rows, its index in the call

// digit p (0 = most significant) of the 96-bit key (score bits : ~doc); positive doubles order like their bit patterns
__device__ __forceinline__ uint32_t bm25_digit(uint64_t sb, uint32_t nd, int p) {
  return p < 8 ? (uint32_t)(sb >> (56 - 8 * p)) & 255u : (nd >> (24 - 8 * (p - 8))) & 255u;
}

// Selection state, derived by every workgroup from the histograms of the passes already run:
// prefix bytes pre[0..np), keys needed inside the prefix bucket, done = bucket wholly selected.
struct Bm25Pick { uint32_t pre[BM25_PASSES]; int np; int64_t need; bool done; };

__device__ __forceinline__ int bm25_cmp_prefix(uint64_t sb, uint32_t nd, const Bm25Pick& st) {
  // -1 below, 0 inside, +1 above the prefix bucket
  for (int p = 0; p < st.np; ++p) {
    const uint32_t dg = bm25_digit(sb, nd, p);
    if (dg != st.pre[p]) return dg > st.pre[p] ? 1 : -1;
  }
  return 0;
}

// one token position of a chunk: jobs[y] = a score row's posting range; x covers the longest range
__global__ __launch_bounds__(256) void bm25_scatter_kernel(const Bm25Job* __restrict__ jobs, const int32_t* __restrict__ post_doc,
                                                           const int32_t* __restrict__ post_tf, const double* __restrict__ doc_norm,
                                                           double k1p1, int64_t n_docs, double* __restrict__ scores) {
#pragma clang fp contract(off)
  const Bm25Job j = jobs[blockIdx.y];           // .query = the job's score row inside the chunk
  const int64_t i = j.lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= j.hi) return;
  const int32_t d = post_doc[i];
  const double f = (double)post_tf[i];
  const double denom = f + doc_norm[d];
  const double num = j.idf * (f * k1p1);
  double* s = scores + (size_t)j.query * n_docs + d;
  *s = *s + num / denom;      // one row per expanded query, docs unique inside a posting list: no two lanes share a word
}

// per question: max / sum over its rows in query order (text_index.py:90-91); s <= 0, untouched or not allowed -> 0
// (not a candidate, :92).  The allow-set only removes candidates: every score is computed as without it (idf and avgdl
// are the corpus's).
__global__ __launch_bounds__(256) void bm25_merge_kernel(double* __restrict__ scores, const Bm25Group* __restrict__ groups,
                                                         int64_t n_docs, int merge_sum, const uint32_t* __restrict__ allow) {
#pragma clang fp contract(off)
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n_docs) return;
  const Bm25Group g = groups[blockIdx.y];
  double* row = scores + (size_t)g.row0 * n_docs + d;
  double s = row[0];
  for (int q = 1; q < g.n_rows; ++q) {
    const double v = row[(size_t)q * n_docs];
    s = merge_sum ? s + v : (v > s ? v : s);
  }
  s = s > 0.0 ? s : 0.0;
  if (allow && !((allow[d >> 5] >> (d & 31)) & 1u)) s = 0.0;
  row[0] = s;
}

// The selection state after `passes` passes, by the whole workgroup (256 threads, one per bin): per pass a suffix sum over
// the bins; the bucket is the highest bin whose suffix sum reaches `need`.  Ends on a barrier.
__device__ inline void bm25_replay_block(const unsigned* __restrict__ hist, int passes, int64_t k, Bm25Pick& st, unsigned* suf) {
  const int t = threadIdx.x;
  if (t == 0) { st.np = 0; st.need = k; st.done = false; }
  __syncthreads();
  for (int p = 0; p < passes; ++p) {
    if (st.done) break;                       // uniform: st is only written between barriers
    const unsigned h = hist[p * 256 + t];
    suf[t] = h;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const unsigned v = t + off < 256 ? suf[t + off] : 0u;
      __syncthreads();
      suf[t] += v;
      __syncthreads();
    }
    const int64_t need = st.need;
    const int64_t at = suf[t], above = t < 255 ? suf[t + 1] : 0u, all = suf[0];    // keys in bins >= t, > t, in every bin
    __syncthreads();
    if (all < need) {
      if (t == 0) { st.done = true; st.need = 0; }   // fewer than `need` keys exist: everything is selected
    } else if (at >= need && above < need) {         // exactly one bin: the suffix sums fall with the bin
      st.pre[st.np++] = (uint32_t)t;
      st.need = need - above;
      if ((int64_t)h == need - above) st.done = true;
    }
    __syncthreads();
  }
}

// pass `pass` of every question of the chunk: histogram of digit `pass` over the keys inside the question's prefix bucket
__global__ __launch_bounds__(256) void bm25_hist_kernel(const double* __restrict__ scores, const Bm25Group* __restrict__ groups,
                                                        int64_t n_docs, int pass, int64_t k, unsigned* __restrict__ hist) {
  __shared__ unsigned lh[256], suf[256];
  __shared__ Bm25Pick st;
  unsigned* gh = hist + (size_t)blockIdx.y * (BM25_PASSES * 256);
  lh[threadIdx.x] = 0u;
  bm25_replay_block(gh, pass, k, st, suf);    // ends on a barrier
  if (st.done) return;
  const double* fin = scores + (size_t)groups[blockIdx.y].row0 * n_docs;
  for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n_docs; d += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t sb = (uint64_t)__double_as_longlong(fin[d]);
    if (sb == 0ull) continue;
    const uint32_t nd = 0xFFFFFFFFu - (uint32_t)d;
    if (bm25_cmp_prefix(sb, nd, st) == 0) atomicAdd(&lh[bm25_digit(sb, nd, pass)], 1u);
  }
  __syncthreads();
  if (lh[threadIdx.x]) atomicAdd(&gh[pass * 256 + threadIdx.x], lh[threadIdx.x]);
}

// the selected keys of every question (above its bucket, or inside a wholly selected bucket), unordered, k slots per question
__global__ __launch_bounds__(256) void bm25_gather_kernel(const double* __restrict__ scores, const Bm25Group* __restrict__ groups,
                                                          int64_t n_docs, int k, const unsigned* __restrict__ hist,
                                                          int* __restrict__ n_sel /*[question of the call]*/,
                                                          int64_t* __restrict__ sel_doc, double* __restrict__ sel_score) {
  __shared__ unsigned suf[256];
  __shared__ Bm25Pick st;
  const Bm25Group g = groups[blockIdx.y];
  bm25_replay_block(hist + (size_t)blockIdx.y * (BM25_PASSES * 256), BM25_PASSES, (int64_t)k, st, suf);
  const double* fin = scores + (size_t)g.row0 * n_docs;
  for (int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n_docs; d += (int64_t)gridDim.x * blockDim.x) {
    const double s = fin[d];
    const uint64_t sb = (uint64_t)__double_as_longlong(s);
    if (sb == 0ull) continue;
    if (bm25_cmp_prefix(sb, 0xFFFFFFFFu - (uint32_t)d, st) >= 0) {   // after all 12 passes the bucket is one key; an early stop takes it whole
      const int slot = atomicAdd(&n_sel[g.question], 1);
      if (slot < k) { sel_doc[(size_t)blockIdx.y * k + slot] = d; sel_score[(size_t)blockIdx.y * k + slot] = s; }
    }
  }
}

// one workgroup per question: order its <= k selected by (score desc, doc asc) into the call's result rows
__global__ __launch_bounds__(1024) void bm25_rank_kernel(const Bm25Group* __restrict__ groups, const int* __restrict__ n_sel,
                                                         const int64_t* __restrict__ sel_doc, const double* __restrict__ sel_score,
                                                         int k, int64_t* __restrict__ out_doc, double* __restrict__ out_score) {
  const int question = groups[blockIdx.x].question;
  const int n = min(n_sel[question], k);
  const int64_t* sd = sel_doc + (size_t)blockIdx.x * k;
  const double* ss = sel_score + (size_t)blockIdx.x * k;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double s = ss[i];
    const int64_t d = sd[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const double sj = ss[j];
      rank += (sj > s || (sj == s && sd[j] < d)) ? 1 : 0;
    }
    out_doc[(size_t)question * k + rank] = d;
    out_score[(size_t)question * k + rank] = s;
  }
}

namespace {

struct Bm25Chunk {
  int rows = 0, n_groups = 0, max_len = 0;
  size_t group0 = 0;      // first descriptor in the call's group list
  size_t pos0 = 0;        // pos_first[pos0 .. pos0 + max_len] (job indexes in the call's job list), pos_longest[pos0 ..)
};

int grid_ok(const dim3& g) {
  if (g.x == 0 || g.y == 0 || g.y > BM25_GRID_YZ || g.z > BM25_GRID_YZ)
    return fail(MRAG_ERR_HIP, "BM25 launch grid (%u, %u, %u) outside HIP's limits", g.x, g.y, g.z);
  return MRAG_OK;
}

// the token lists of queries [q_first, q_last): offsets from 0 upwards, term ids inside the vocabulary (< 0 = unknown term)
int check_queries(const Bm25Index* ix, int q_first, int q_last, const int32_t* q_ptr, const int32_t* q_terms, const double* q_idf) {
  if (q_first >= q_last) return MRAG_OK;
  if (q_ptr[q_first] < 0) return fail(MRAG_ERR_INVALID, "q_ptr starts below 0");
  for (int q = q_first; q < q_last; ++q)
    if (q_ptr[q + 1] < q_ptr[q]) return fail(MRAG_ERR_INVALID, "q_ptr not monotone");
  if (q_ptr[q_last] == q_ptr[q_first]) return MRAG_OK;
  if (!q_terms || !q_idf) return fail(MRAG_ERR_INVALID, "NULL buffer");
  for (int at = q_ptr[q_first]; at < q_ptr[q_last]; ++at)
    if (q_terms[at] >= ix->n_terms)
      return fail(MRAG_ERR_INVALID, "term id %d outside the vocabulary (%lld)", q_terms[at], (long long)ix->n_terms);
  return MRAG_OK;
}

// The search of n_questions >= 1 validated questions over a non-empty index, 1 <= k <= BM25_MAX_K: question g's answer in
// slots [g * k, g * k + out_n[g]) of out_docs / out_scores, (-1, 0.0) in the rest of its k slots.  A question without
// queries gets no launch and no output: its slots are the caller's to fill.
int search_questions(Bm25Index* ix, int n_questions, const int32_t* g_ptr, const int32_t* q_ptr, const int32_t* q_terms,
                     const double* q_idf, int merge_sum, int k, const uint32_t* allow_bits, int64_t* out_docs, double* out_scores,
                     int32_t* out_n, hipStream_t stream) {
  const int64_t N = ix->n_docs;
  const size_t n_out = (size_t)n_questions * k;

  // ---- the plan: chunks of whole questions, per chunk the jobs of every token position (unknown terms, id < 0, add nothing)
  const int64_t rows_cap = std::min<int64_t>(std::max<int64_t>(ix->scratch_limit / (N * 8), 1), BM25_GRID_YZ);
  std::vector<Bm25Chunk> chunks;
  std::vector<Bm25Group> groups;
  std::vector<Bm25Job> jobs;
  std::vector<size_t> pos_first;
  std::vector<int64_t> pos_longest;
  int max_rows = 0, max_groups = 0;
  for (int g = 0; g < n_questions;) {
    Bm25Chunk c;
    c.group0 = groups.size();
    int q0 = -1;                                 // the chunk's first query: its rows are the queries q0 .. q0 + rows - 1
    for (; g < n_questions; ++g) {
      const int nq = g_ptr[g + 1] - g_ptr[g];
      if (nq == 0) continue;
      if (c.n_groups && (c.rows + nq > rows_cap || c.n_groups == BM25_CHUNK_QUESTIONS)) break;
      if (q0 < 0) q0 = g_ptr[g];
      groups.push_back(Bm25Group{c.rows, nq, g, 0});
      c.rows += nq;
      ++c.n_groups;
    }
    if (!c.n_groups) break;
    for (int r = 0; r < c.rows; ++r) c.max_len = std::max(c.max_len, q_ptr[q0 + r + 1] - q_ptr[q0 + r]);
    c.pos0 = pos_first.size();
    for (int j = 0; j < c.max_len; ++j) {
      pos_first.push_back(jobs.size());
      int64_t longest = 0;
      for (int r = 0; r < c.rows; ++r) {
        const int at = q_ptr[q0 + r] + j;
        if (at >= q_ptr[q0 + r + 1]) continue;
        const int32_t t = q_terms[at];
        if (t < 0) continue;
        const int64_t lo = ix->h_indptr[t], hi = ix->h_indptr[t + 1];
        if (hi == lo) continue;
        jobs.push_back(Bm25Job{lo, hi, q_idf[at], r, 0});
        longest = std::max(longest, hi - lo);
      }
      pos_longest.push_back(longest);
    }
    pos_first.push_back(jobs.size());
    pos_longest.push_back(0);
    max_rows = std::max(max_rows, c.rows);
    max_groups = std::max(max_groups, c.n_groups);
    chunks.push_back(c);
  }
  if (chunks.empty()) return MRAG_OK;            // no question has a query

  MRAG_TRY(use_device(ix->device));
  const size_t jobs_bytes = jobs.size() * sizeof(Bm25Job), groups_bytes = groups.size() * sizeof(Bm25Group);
  const size_t hist_bytes = (size_t)BM25_PASSES * 256 * 4, words = (size_t)(N + 31) / 32;
  // every buffer before the first launch: growing one frees it
  MRAG_TRY(ix->scores.ensure((size_t)max_rows * N * 8));
  MRAG_TRY(ix->plan.ensure(jobs_bytes + groups_bytes));
  MRAG_TRY(ix->hist.ensure((size_t)max_groups * hist_bytes));
  MRAG_TRY(ix->sel.ensure((size_t)max_groups * k * 16));
  MRAG_TRY(ix->out.ensure(n_out * 16 + (size_t)n_questions * 4));
  if (allow_bits) MRAG_TRY(ix->allow.ensure(words * 4));
  const Bm25Job* d_jobs = (const Bm25Job*)ix->plan.p;
  const Bm25Group* d_groups = (const Bm25Group*)((char*)ix->plan.p + jobs_bytes);
  unsigned* d_hist = (unsigned*)ix->hist.p;
  int64_t* d_sel_doc = (int64_t*)ix->sel.p;
  double* d_sel_score = (double*)(d_sel_doc + (size_t)max_groups * k);
  int64_t* d_out_doc = (int64_t*)ix->out.p;
  double* d_out_score = (double*)(d_out_doc + n_out);
  int* d_n_sel = (int*)(d_out_score + n_out);
  double* d_scores = (double*)ix->scores.p;
  const uint32_t* d_allow = allow_bits ? (const uint32_t*)ix->allow.p : nullptr;

  auto enqueue = [&]() -> int {
    if (jobs_bytes) MRAG_HIP(hipMemcpyAsync(ix->plan.p, jobs.data(), jobs_bytes, hipMemcpyHostToDevice, stream));
    MRAG_HIP(hipMemcpyAsync((char*)ix->plan.p + jobs_bytes, groups.data(), groups_bytes, hipMemcpyHostToDevice, stream));
    if (allow_bits) MRAG_HIP(hipMemcpyAsync(ix->allow.p, allow_bits, words * 4, hipMemcpyHostToDevice, stream));
    MRAG_HIP(hipMemsetAsync(d_out_doc, 0xFF, n_out * 8, stream));                                   // (-1, 0.0) and out_n = 0
    MRAG_HIP(hipMemsetAsync(d_out_score, 0, n_out * 8 + (size_t)n_questions * 4, stream));
    const unsigned dgrid = (unsigned)((N + 255) / 256), sgrid = std::min<unsigned>(dgrid, 1024);
    for (const Bm25Chunk& c : chunks) {
      const Bm25Group* cg = d_groups + c.group0;
      MRAG_HIP(hipMemsetAsync(d_scores, 0, (size_t)c.rows * N * 8, stream));
      MRAG_HIP(hipMemsetAsync(d_hist, 0, (size_t)c.n_groups * hist_bytes, stream));
      for (int j = 0; j < c.max_len; ++j) {
        const size_t first = pos_first[c.pos0 + j], nj = pos_first[c.pos0 + j + 1] - first;
        if (!nj) continue;
        const dim3 grid((unsigned)((pos_longest[c.pos0 + j] + 255) / 256), (unsigned)nj);
        MRAG_TRY(grid_ok(grid));
        hipLaunchKernelGGL(bm25_scatter_kernel, grid, dim3(256), 0, stream, d_jobs + first, ix->post_doc, ix->post_tf,
                           ix->doc_norm, ix->k1p1, N, d_scores);
      }
      const dim3 mgrid(dgrid, (unsigned)c.n_groups), hgrid(sgrid, (unsigned)c.n_groups), rgrid((unsigned)c.n_groups);
      MRAG_TRY(grid_ok(mgrid));
      MRAG_TRY(grid_ok(hgrid));
      hipLaunchKernelGGL(bm25_merge_kernel, mgrid, dim3(256), 0, stream, d_scores, cg, N, merge_sum ? 1 : 0, d_allow);
      for (int p = 0; p < BM25_PASSES; ++p)
        hipLaunchKernelGGL(bm25_hist_kernel, hgrid, dim3(256), 0, stream, (const double*)d_scores, cg, N, p, (int64_t)k, d_hist);
      hipLaunchKernelGGL(bm25_gather_kernel, hgrid, dim3(256), 0, stream, (const double*)d_scores, cg, N, k,
                         (const unsigned*)d_hist, d_n_sel, d_sel_doc, d_sel_score);
      hipLaunchKernelGGL(bm25_rank_kernel, rgrid, dim3(1024), 0, stream, cg, (const int*)d_n_sel, (const int64_t*)d_sel_doc,
                         (const double*)d_sel_score, k, d_out_doc, d_out_score);
      MRAG_HIP(hipGetLastError());
    }
    MRAG_HIP(hipMemcpyAsync(out_n, d_n_sel, (size_t)n_questions * 4, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipMemcpyAsync(out_docs, d_out_doc, n_out * 8, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipMemcpyAsync(out_scores, d_out_score, n_out * 8, hipMemcpyDeviceToHost, stream));
    return MRAG_OK;
  };
  const int st = enqueue();
  const hipError_t e = hipStreamSynchronize(stream);   // the plan and the caller's buffers are in use until here, also after a failure
  if (st != MRAG_OK) { std::fill(out_n, out_n + n_questions, 0); return st; }
  MRAG_HIP(e);
  for (int g = 0; g < n_questions; ++g)
    if (out_n[g] > k) {
      const int n = out_n[g];
      std::fill(out_n, out_n + n_questions, 0);
      return fail(MRAG_ERR_HIP, "BM25 selection produced %d > k = %d entries for question %d", n, k, g);
    }
  return MRAG_OK;
}

}  // namespace

}  // namespace mrag

using namespace mrag;

extern "C" {

int mrag_bm25_create(int device, int64_t n_docs, int64_t n_terms, const int64_t* indptr, const int32_t* post_doc,
                     const int32_t* post_tf, const double* doc_norm, double k1_plus_1, mrag_handle* out) {
  if (!out) return fail(MRAG_ERR_INVALID, "out is NULL");
  if (n_docs < 0 || n_terms < 0 || n_docs > 0x7FFFFFFFll) return fail(MRAG_ERR_INVALID, "bad sizes");
  if (n_terms && (!indptr || indptr[0] != 0)) return fail(MRAG_ERR_INVALID, "indptr must start at 0");
  const int64_t nnz = n_terms ? indptr[n_terms] : 0;
  if (nnz && (!post_doc || !post_tf)) return fail(MRAG_ERR_INVALID, "NULL postings");
  if (n_docs && !doc_norm) return fail(MRAG_ERR_INVALID, "NULL doc_norm");
  for (int64_t t = 0; t < n_terms; ++t)
    if (indptr[t + 1] < indptr[t]) return fail(MRAG_ERR_INVALID, "indptr not monotone at term %lld", (long long)t);
  MRAG_TRY(use_device(device));
  Bm25Index* ix = new Bm25Index();
  ix->kind = KIND_BM25; ix->device = device;
  ix->n_docs = n_docs; ix->n_terms = n_terms; ix->nnz = nnz; ix->k1p1 = k1_plus_1;
  ix->h_indptr.assign(indptr, indptr + (n_terms ? n_terms + 1 : 0));
  auto up = [&](DevBuf& dst, const void* src, size_t bytes) -> int {
    if (!bytes) return MRAG_OK;
    MRAG_TRY(dst.alloc(bytes));
    MRAG_HIP(hipMemcpy(dst.p, src, bytes, hipMemcpyHostToDevice));
    return MRAG_OK;
  };
  int st = up(ix->indptr, indptr, (size_t)(n_terms ? n_terms + 1 : 0) * 8);
  if (st == MRAG_OK) st = up(ix->post_doc, post_doc, (size_t)nnz * 4);
  if (st == MRAG_OK) st = up(ix->post_tf, post_tf, (size_t)nnz * 4);
  if (st == MRAG_OK) st = up(ix->doc_norm, doc_norm, (size_t)n_docs * 8);
  if (st != MRAG_OK) { delete ix; return st; }
  *out = register_object(ix);
  return MRAG_OK;
}

int mrag_bm25_destroy(mrag_handle h) { return destroy_object(h, KIND_BM25); }

int mrag_bm25_set_scratch_limit(mrag_handle h, int64_t bytes) {
  Bm25Index* ix = (Bm25Index*)lookup(h, KIND_BM25);
  if (!ix) return MRAG_ERR_INVALID;
  ix->scratch_limit = bytes > 0 ? bytes : BM25_DEFAULT_SCRATCH;
  return MRAG_OK;
}

// One question: its n_queries expanded queries are the question's score rows, so the scratch limit never splits it.
// The k slots of out_docs / out_scores are the capacity mrag.h asks for; those past *out_n hold (-1, 0.0).
int mrag_bm25_search(mrag_handle h, int n_queries, const int32_t* q_ptr, const int32_t* q_terms, const double* q_idf,
                     int merge_sum, int k, int64_t* out_docs, double* out_scores, int* out_n, void* stream) {
  Bm25Index* ix = (Bm25Index*)lookup(h, KIND_BM25);
  if (!ix) return MRAG_ERR_INVALID;
  if (!out_n) return fail(MRAG_ERR_INVALID, "out_n is NULL");
  *out_n = 0;
  if (n_queries < 0 || k < 0) return fail(MRAG_ERR_INVALID, "bad n_queries / k");
  if (k > BM25_MAX_K) return fail(MRAG_ERR_UNSUPPORTED, "k = %d exceeds %d", k, BM25_MAX_K);
  if (n_queries == 0 || k == 0 || ix->n_docs == 0) return MRAG_OK;
  if (!q_ptr || !out_docs || !out_scores) return fail(MRAG_ERR_INVALID, "NULL buffer");
  if (n_queries > BM25_MAX_QUERIES) return fail(MRAG_ERR_UNSUPPORTED, "more than %d queries per call", BM25_MAX_QUERIES);
  MRAG_TRY(check_queries(ix, 0, n_queries, q_ptr, q_terms, q_idf));
  const int32_t g_ptr[2] = {0, n_queries};
  return search_questions(ix, 1, g_ptr, q_ptr, q_terms, q_idf, merge_sum, k, nullptr, out_docs, out_scores, out_n, (hipStream_t)stream);
}

int mrag_bm25_search_batch(mrag_handle h, int n_questions, const int32_t* g_ptr, const int32_t* q_ptr, const int32_t* q_terms,
                           const double* q_idf, int merge_sum, int k, const uint32_t* allow_bits, int64_t* out_docs,
                           double* out_scores, int32_t* out_n, void* stream) {
  Bm25Index* ix = (Bm25Index*)lookup(h, KIND_BM25);
  if (!ix) return MRAG_ERR_INVALID;
  if (n_questions < 0 || k < 0) return fail(MRAG_ERR_INVALID, "bad n_questions / k");
  if (n_questions == 0) return MRAG_OK;
  if (!out_n) return fail(MRAG_ERR_INVALID, "out_n is NULL");
  std::fill(out_n, out_n + n_questions, 0);
  if (k > BM25_MAX_K) return fail(MRAG_ERR_UNSUPPORTED, "k = %d exceeds %d", k, BM25_MAX_K);
  if (k == 0) return MRAG_OK;
  if (!g_ptr || !q_ptr || !out_docs || !out_scores) return fail(MRAG_ERR_INVALID, "NULL buffer");
  const size_t n_out = (size_t)n_questions * k;
  std::fill(out_docs, out_docs + n_out, (int64_t)-1);     // what a question without queries, or every question of an empty index, keeps
  std::fill(out_scores, out_scores + n_out, 0.0);
  if (ix->n_docs == 0) return MRAG_OK;
  // the whole batch is validated before anything is launched
  if (g_ptr[0] < 0) return fail(MRAG_ERR_INVALID, "g_ptr starts below 0");
  for (int g = 0; g < n_questions; ++g) {
    if (g_ptr[g + 1] < g_ptr[g]) return fail(MRAG_ERR_INVALID, "g_ptr not monotone at question %d", g);
    if (g_ptr[g + 1] - g_ptr[g] > BM25_MAX_QUERIES)
      return fail(MRAG_ERR_UNSUPPORTED, "question %d has more than %d queries", g, BM25_MAX_QUERIES);
  }
  MRAG_TRY(check_queries(ix, g_ptr[0], g_ptr[n_questions], q_ptr, q_terms, q_idf));
  return search_questions(ix, n_questions, g_ptr, q_ptr, q_terms, q_idf, merge_sum, k, allow_bits, out_docs, out_scores, out_n,
                          (hipStream_t)stream);
}

}  // extern "C"
