/*
 * mrag_bm25_batch.h -- the batched BM25 search of libmrag_hip.so: two entry points added to the C ABI of mrag.h.
 *
 * mrag.h includes this header, so a program that includes mrag.h has them; the conventions (status codes, handles, host
 * buffers, `stream`) are mrag.h's.  mrag.h itself keeps the 64 entry points it had: additions to the ABI come as
 * headers like this one, and MRAG_ABI_VERSION stays 1, as it did for every earlier addition.
 */
#ifndef MRAG_BM25_BATCH_H_
#define MRAG_BM25_BATCH_H_

#include "mrag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The same search for a BATCH of questions (text_index.py:71-97, applied per question): question g owns the expanded queries
 * g_ptr[g] .. g_ptr[g+1] (g_ptr[n_questions+1] indexes q_ptr; q_ptr / q_terms / q_idf as in mrag_bm25_search), and its answer is exactly what
 * mrag_bm25_search returns for those queries alone: the same documents, the same score bits, (score desc, doc asc), scores > 0
 * only.  out_docs / out_scores are [n_questions][k], out_n [n_questions]; the slots past out_n[g] hold (-1, 0.0).  A question
 * without queries, or with only empty or unknown-term queries, gets out_n = 0.  k <= 4096 and at most 1024 expanded queries per
 * question (MRAG_ERR_UNSUPPORTED beyond, as in mrag_bm25_search); n_questions is unbounded.  The whole batch is validated
 * before anything runs, with the status codes of mrag_bm25_search; after an error every out_n is 0.
 * allow_bits (text_index.py:92 keeps a document when s > 0; here also only when it is allowed -- the row filter the dense
 * channel applies to the same docs.jsonl rows): NULL = every document, else ceil(n_docs/32) host words, bit d%32 of word
 * d/32.  The set only decides which documents can be candidates; it changes no score (idf and avgdl stay the corpus's).  All
 * documents allowed is identical to NULL; no document allowed gives out_n = 0 everywhere.
 * All buffers are host buffers.  Questions are processed in chunks of whole questions whose fp64 score rows (n_docs * 8
 * bytes per expanded query; the merged row of a question reuses its first score row) fit the scratch limit; a question that
 * alone exceeds the limit is a chunk of its own.  The number of launches of a chunk does not depend on its number of
 * questions, and the call synchronises `stream` once, after the last chunk.
 * mrag_bm25_set_scratch_limit (text_index.py:71-97 has no counterpart: the reference scores candidates one by one): bytes of
 * score rows a chunk may use; <= 0 restores the default of 1 GiB -- a default nobody has measured an optimum for.  The
 * result does not depend on it. */
int mrag_bm25_search_batch(mrag_handle h, int n_questions, const int32_t* g_ptr, const int32_t* q_ptr, const int32_t* q_terms,
                           const double* q_idf, int merge_sum, int k, const uint32_t* allow_bits, int64_t* out_docs,
                           double* out_scores, int32_t* out_n, void* stream);
int mrag_bm25_set_scratch_limit(mrag_handle h, int64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* MRAG_BM25_BATCH_H_ */
