/*
 * mrag_rerank_batch.h -- the batched dense re-rank of libmrag_hip.so: one entry point added to the C ABI of mrag.h.
 *
 * mrag.h includes this header, so a program that includes mrag.h has it; the conventions (status codes, host buffers,
 * `stream`) are mrag.h's.  mrag.h itself keeps the 64 entry points it had, and MRAG_ABI_VERSION stays 1.
 */
#ifndef MRAG_RERANK_BATCH_H_
#define MRAG_RERANK_BATCH_H_

#include "mrag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The candidate lookup of mrag_index_score_rows for a BATCH of questions (DenseReranker.score per question of an
 * evaluation set, retrieval_backend.py:215-247, 332-334): queries is [n_questions][dim] in q_dtype, question g's
 * candidates are the stored rows row_ids[row_ptr[g] .. row_ptr[g+1]) (row_ptr: int64 [n_questions + 1], row_ptr[0] = 0,
 * non-decreasing), and out_scores has the layout of row_ids: out_scores[e] = <query g, stored row row_ids[e]>.
 * Question g's scores are bit for bit what mrag_index_score_rows returns for query g and g's ids alone, wherever g
 * stands in the batch and whatever the other questions hold: the query rows get the single call's preparation, and a
 * row's fp64 sum keeps the single kernel's assignment of columns to lanes, its per-lane order and its butterfly.
 * An id outside [0, size) scores 0.0; an id may occur any number of times, within a question and across questions; an
 * empty question costs nothing.  Sizes are int64 throughout: entries are limited by memory only (MRAG_ERR_OOM).
 * Refused before any device work, the message naming the question where there is one: n_questions < 0, row_ptr[0] != 0,
 * a decreasing row_ptr, a NULL required buffer when there is at least one entry, an unknown q_dtype, a dead handle --
 * MRAG_ERR_INVALID.  n_questions == 0 and a batch of empty questions are MRAG_OK without device work.
 * All buffers are host buffers.  The host cuts every question's list into descriptors of at most 64 rows, one
 * workgroup each, so no launch dimension depends on the longest list; the call makes one upload each of queries,
 * descriptors and ids, one row preparation, one score launch (one per 2^31 - 1 descriptors), one download, and
 * synchronises `stream` once, whatever the batch. */
int mrag_index_score_rows_batch(mrag_handle h, const void* queries, int q_dtype, int normalize, int64_t n_questions,
                                const int64_t* row_ptr, const int64_t* row_ids, float* out_scores, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MRAG_RERANK_BATCH_H_ */
