// What the BM25 sources (bm25.hip: one question per call; bm25_batch.hip: many questions per call) share: the index object,
// the posting-range job of the scatter launches and the selection state every selection workgroup derives from the
// histograms of the passes already run.  Kernels stay inside the source that owns them.  Internal to those two sources.
#pragma once
#include "common.h"

#include <vector>

namespace mrag {

constexpr int64_t BM25_DEFAULT_SCRATCH = 1ll << 30;   // score rows of one chunk of the batch search (mrag_bm25_batch.h: not a measured optimum)

struct Bm25Index : Object {
  int64_t n_docs = 0, n_terms = 0, nnz = 0;
  double k1p1 = 2.5;
  int64_t* indptr = nullptr;     // [n_terms + 1]
  int32_t* post_doc = nullptr;   // [nnz]
  int32_t* post_tf = nullptr;    // [nnz]
  double* doc_norm = nullptr;    // [n_docs]  k1 * (1 - b + b * dl / avgdl)
  std::vector<int64_t> h_indptr; // host copy: posting counts size the launches
  DevBuf scores, fin, hist, sel, qbuf;
  // batch search (bm25_batch.hip); `scores` is shared with the single search, one call in flight per handle
  int64_t scratch_limit = BM25_DEFAULT_SCRATCH;
  DevBuf b_plan, b_hist, b_sel, b_out, b_allow;
  ~Bm25Index() override {
    for (void* p : {(void*)indptr, (void*)post_doc, (void*)post_tf, (void*)doc_norm}) if (p) (void)hipFree(p);
    for (DevBuf* b : {&scores, &fin, &hist, &sel, &qbuf, &b_plan, &b_hist, &b_sel, &b_out, &b_allow}) b->release();
  }
};

constexpr int BM25_MAX_K = 4096;
constexpr int BM25_MAX_QUERIES = 1024;   // expanded queries of one question
constexpr int BM25_PASSES = 12;   // 8 bytes of score bits + 4 bytes of ~doc

struct Bm25Job { int64_t lo, hi; double idf; int32_t query; int32_t pad; };   // one (query, token position) posting range

#if defined(__HIPCC__)
// digit p (0 = most significant) of the 96-bit key (score bits : ~doc); positive doubles order like their bit patterns
__device__ __forceinline__ uint32_t bm25_digit(uint64_t sb, uint32_t nd, int p) {
  return p < 8 ? (uint32_t)(sb >> (56 - 8 * p)) & 255u : (nd >> (24 - 8 * (p - 8))) & 255u;
}

// Selection state, derived by every workgroup from the histograms of the passes already run:
// prefix bytes pre[0..np), keys needed inside the prefix bucket, done = bucket wholly selected.
struct Bm25Pick { uint32_t pre[BM25_PASSES]; int np; int64_t need; bool done; };

__device__ inline void bm25_replay(const unsigned* __restrict__ hist, int passes, int64_t k, Bm25Pick& st) {
  st.np = 0; st.need = k; st.done = false;
  for (int p = 0; p < passes && !st.done; ++p) {
    const unsigned* h = hist + p * 256;
    int64_t cum = 0;
    int b = 255;
    for (; b >= 0; --b) {
      if (cum + h[b] >= st.need) break;
      cum += h[b];
    }
    if (b < 0) { st.done = true; st.need = 0; break; }   // fewer than `need` keys exist: everything is selected
    st.pre[st.np++] = (uint32_t)b;
    st.need -= cum;
    if ((int64_t)h[b] == st.need) st.done = true;
  }
}

__device__ __forceinline__ int bm25_cmp_prefix(uint64_t sb, uint32_t nd, const Bm25Pick& st) {
  // -1 below, 0 inside, +1 above the prefix bucket
  for (int p = 0; p < st.np; ++p) {
    const uint32_t dg = bm25_digit(sb, nd, p);
    if (dg != st.pre[p]) return dg > st.pre[p] ? 1 : -1;
  }
  return 0;
}
#endif

}  // namespace mrag
