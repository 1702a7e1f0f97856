/*
 * mrag_filter_batch.h -- dense search with one allow-set of rows per question: two entry points added to the C ABI of
 * mrag.h.
 *
 * mrag.h includes this header, so a program that includes mrag.h has them; the conventions (status codes, handles, host
 * buffers, `stream`) are mrag.h's.  mrag.h itself keeps the 64 entry points it had, and MRAG_ABI_VERSION stays 1.
 */
#ifndef MRAG_FILTER_BATCH_H_
#define MRAG_FILTER_BATCH_H_

#include "mrag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mrag_index_search_filtered for a BATCH of questions that each search their own allow-set of rows (HotpotQA's
 * distractor setting: every question comes with its own ten paragraphs; a tenant or title filter: a few sets shared by
 * many questions).  queries is [nq][dim] in q_dtype and gets the plain search's preparation.  Set s is the local rows
 * set_rows[set_ptr[s] .. set_ptr[s+1]) (set_ptr: int64 [n_sets + 1], set_ptr[0] = 0, non-decreasing; the rows of a set
 * strictly ascending, inside [0, size), taken before id_base), and question q searches set set_of[q] (int32 [nq]).
 * Per question: the top-k of its set's rows in (score desc, row asc) order, ids = id_base + row, slots past the set's
 * size (-inf, -1), an empty set an all-(-inf, -1) row; out_scores / out_ids are [nq][k].
 *
 * Two routes, chosen per set by its size alone:
 *   scan    a set of at most 8 192 rows (the select kernel's register-path capacity): its rows are gathered straight from
 *           the corpus by the scan kernel and scored against the questions that use it, the scores leave as one fp32
 *           segment per question, and the segment's k best are selected.  A question's result does not depend on where it
 *           stands in the batch or on what the other questions hold.  Per call: one upload each of queries, plan and set
 *           rows, one row preparation, one scan launch and one select launch per scratch chunk, one download and ONE
 *           synchronisation of `stream`.  The score scratch is index-owned; a call whose segments exceed 1 GiB is cut
 *           into chunks of whole questions (no synchronisation between chunks).
 *   routed  a larger set becomes ONE mrag_index_search_filtered (MRAG_FILTER_AUTO, a host bitset built from its rows)
 *           over all of its questions together, written into those questions' output rows: a filter shared by 500
 *           questions costs one filtered search.  Where mrag_index_max_k(questions of the set) < k the questions are
 *           searched in groups that allow k; k is never clamped.
 *
 * 1 <= k <= 256 (= mrag_index_max_k for one query); k > 256 is MRAG_ERR_UNSUPPORTED.  Refused before any device work with
 * MRAG_ERR_INVALID, the message naming the set or the question, the output buffers untouched: nq < 0 or n_sets < 0,
 * set_ptr[0] != 0 or a decreasing set_ptr, a row outside [0, size), rows of a set that are not strictly ascending
 * (duplicates included), set_of[q] outside [0, n_sets), a NULL required buffer, an unknown q_dtype, a dead handle, k < 1.
 * nq == 0 is MRAG_OK without device work.  All buffers are host buffers. */
int mrag_index_search_sets(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int k,
                           int64_t n_sets, const int64_t* set_ptr, const int64_t* set_rows, const int32_t* set_of,
                           float* out_scores, int64_t* out_ids, void* stream);

/* What the LAST mrag_index_search_sets on this index did: questions that went through the scan (those of empty sets
 * included), questions that were routed to filtered searches, and descriptors (one chunk of <= 128 rows of a set x <= 128
 * of its questions) the scan launches walked.  Any output may be NULL.  MRAG_ERR_INVALID before the first completed call. */
int mrag_index_last_sets(mrag_handle h, int64_t* out_scanned_questions, int64_t* out_routed_questions,
                         int64_t* out_descriptors);

#ifdef __cplusplus
}
#endif
#endif /* MRAG_FILTER_BATCH_H_ */
