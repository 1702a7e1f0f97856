/*
 * mrag_search_groups.h -- dense search with several query vectors per question, max-merged on the device: two entry
 * points added to the C ABI of mrag.h.
 *
 * mrag.h includes this header, so a program that includes mrag.h has them; the conventions (status codes, handles, host
 * and device buffers, `stream`) are mrag.h's.  mrag.h itself keeps the 64 entry points it had, and MRAG_ABI_VERSION
 * stays 1.
 */
#ifndef MRAG_SEARCH_GROUPS_H_
#define MRAG_SEARCH_GROUPS_H_

#include "mrag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mrag_index_search for questions that each come as SEVERAL query vectors (the question and its expansions, the
 * reference's `queries = [req.query] + expanded`, retrieval_backend.py:307-310), merged per row with the maximum
 * (alpha_merge="max").  queries is [nq][dim] in q_dtype, host or device (queries_on_device), prepared as the plain
 * search prepares them; question g owns the queries group_ptr[g] .. group_ptr[g+1) (group_ptr: HOST int64
 * [n_groups + 1], group_ptr[0] = 0, non-decreasing, group_ptr[n_groups] = nq).
 *
 * Per question: the score of a row is the largest of its scores under the question's queries; the result is the top-k
 * of those scores in the index's declared order (score desc, id asc, ids = id_base + row), bit for bit what merging the
 * per-query top-k lists of mrag_index_search gives -- the union of those lists holds the merged top-k, ties included.
 * out_scores / out_ids / out_which are [n_groups][k], host or device (out_on_device); out_which (int32, may be NULL) is
 * the position inside the question of the query that gave the kept score, the lowest one among equal scores (+0.0 and
 * -0.0 are equal).  Slots past the number of distinct rows found are (-inf, -1, -1); a question without queries is such
 * a row.
 *
 * allow == NULL searches every row.  Otherwise allow / allow_n / allow_format are a HOST allow-set for the whole call,
 * as mrag_index_search_filtered takes it, and the underlying search is that call with MRAG_FILTER_AUTO.
 *
 * Per call: ONE search of all nq queries into index-owned device scratch, ONE merge launch (one workgroup per question),
 * and for host outputs one download and ONE synchronisation of `stream`; with device outputs the call does not wait.
 * A question's outputs do not depend on where it stands in the call or on what the other questions hold.
 *
 * 1 <= k <= 256 (= mrag_index_max_k for every nq, so the queries are never searched in parts and k is never clamped);
 * k > 256 is MRAG_ERR_UNSUPPORTED, and so is a question with queries x k > 4096 (the merge sorts a question in LDS).
 * Refused before any device work with MRAG_ERR_INVALID, the message naming the question where there is one, the output
 * buffers untouched: nq < 0 or n_groups < 0, group_ptr[0] != 0, a decreasing group_ptr, group_ptr[n_groups] != nq, a NULL
 * required buffer, an unknown q_dtype, a dead handle, k < 1, an allow-set that mrag_index_search_filtered would refuse.
 * n_groups == 0 (with nq == 0) is MRAG_OK without device work. */
int mrag_index_search_groups(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize,
                             int queries_on_device, int k, int64_t n_groups, const int64_t* group_ptr,
                             const void* allow, int64_t allow_n, int allow_format,
                             float* out_scores, int64_t* out_ids, int32_t* out_which, int out_on_device, void* stream);

/* What the LAST mrag_index_search_groups on this index did: query vectors searched, questions merged, and the entries
 * (queries x k) of its largest question, which sized the merge launch.  Any output may be NULL.  MRAG_ERR_INVALID before
 * the first completed call. */
int mrag_index_last_groups(mrag_handle h, int64_t* out_queries, int64_t* out_groups, int64_t* out_max_entries);

#ifdef __cplusplus
}
#endif
#endif /* MRAG_SEARCH_GROUPS_H_ */
