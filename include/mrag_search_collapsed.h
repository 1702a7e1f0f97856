/*
 * mrag_search_collapsed.h -- collapsed dense search, the top-k KEYS of a query with each key represented by its best row
 * (field collapsing, parent-document retrieval): three entry points added to the C ABI of mrag.h.
 *
 * mrag.h includes this header, so a program that includes mrag.h has them; the conventions (status codes, handles, host
 * and device buffers, `stream`) are mrag.h's.  mrag.h itself keeps the 64 entry points it had, and MRAG_ABI_VERSION
 * stays 1.
 */
#ifndef MRAG_SEARCH_COLLAPSED_H_
#define MRAG_SEARCH_COLLAPSED_H_

#include "mrag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One int32 key per stored row (a document, a title, a tenant), 0 <= key < 2^31; keys is [n], host or device
 * (keys_on_device), and n must equal the index size.  The keys are validated on the host (a negative key is
 * MRAG_ERR_INVALID and leaves the keys set before untouched); the number of distinct keys and the largest number of rows
 * that share a key are counted there too, so device keys are copied back once.  The index keeps its own device copy.
 * Rows added afterwards have no key: mrag_index_search_collapsed is refused until the keys are set again for all rows.
 * n == 0 with keys == NULL clears the keys, whatever the index holds.  The call waits for the device (it is a one-off,
 * like mrag_index_reserve). */
int mrag_index_set_row_keys(mrag_handle h, const int32_t* keys, int64_t n, int keys_on_device);

/* mrag_index_search with one hit per key.  For a query the score of a key is the best score of its rows, and the key's
 * representative is the first of its rows in the index's declared order (score desc, row asc).  The answer is the top-k
 * keys, ordered by their representatives in that same order; out_scores / out_ids / out_keys are [nq][k], host or device
 * (out_on_device), and hold the representative's score, its id (id_base + row) and the key (out_keys: int32, may be
 * NULL).  Slots past the number of distinct keys are (-inf, -1, -1); an empty index gives only such slots (and needs no
 * keys).  With all keys distinct the scores and ids are bit for bit those of mrag_index_search at k.
 *
 * The call is exact and made of rounds.  Round 0: ONE mrag_index_search of all nq queries at depth scan_k into
 * index-owned scratch and ONE collapse launch (one workgroup per query) that keeps the first entry of every key.  A query
 * is complete when that gave k keys, or when its list held fewer than scan_k rows (every row was seen): a key not met has
 * all its rows behind the scan_k-th entry, and k representatives stand before it.  Every incomplete query is then redone
 * alone, round after round: a mask launch (the rows whose key it has not found), one mrag_index_search_filtered with that
 * device allow-set and MRAG_FILTER_AUTO at scan_k, and the collapse launch appending behind what it has.  Every redo round
 * adds at least one key, so a query takes at most k of them.  mrag_index_last_collapsed tells how many there were;
 * mrag_index_last_filter afterwards reports the LAST redo round's filtered search (or what it reported before the call
 * when nothing was redone).
 *
 * scan_k == 0 picks min(256, rows, max(k, (k-1) * m + 1)), never below k, with m the largest number of rows that share
 * a key: a depth at which no redo can happen when it is below the 256 cap.  Any k <= scan_k <= 256 trades scan depth
 * against redo rounds.
 *
 * The call synchronises `stream` at least once -- it reads the per-query completeness words back after round 0 and after
 * every redo round -- ALSO with device outputs; a redo round's filtered search synchronises once more per query.
 * A query's outputs do not depend on where it stands in the call or on what the other queries hold.
 *
 * Refused before any device work, the message naming the cause, the output buffers untouched, with MRAG_ERR_INVALID:
 * a dead handle, nq < 0, k < 1, scan_k not 0 and outside [k, 256], no keys set on an index that holds rows, keys set
 * for another row count (rows were added since), a NULL required buffer, an unknown q_dtype; with MRAG_ERR_UNSUPPORTED:
 * k > 256.  nq == 0 is MRAG_OK without device work. */
int mrag_index_search_collapsed(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize,
                                int queries_on_device, int k, int scan_k, float* out_scores, int64_t* out_ids,
                                int32_t* out_keys, int out_on_device, void* stream);

/* What the LAST completed mrag_index_search_collapsed on this index did: the scan depth it used, the queries that were
 * incomplete after round 0, the filtered searches the redo rounds ran in all (one per incomplete query and round), and
 * of the keys it searched under the largest number of rows that share a key and the number of distinct keys.  Any output
 * may be NULL.  MRAG_ERR_INVALID before the first completed call. */
int mrag_index_last_collapsed(mrag_handle h, int* out_scan_k, int64_t* out_redone_queries, int64_t* out_redo_rounds,
                              int64_t* out_max_rows_per_key, int64_t* out_distinct_keys);

#ifdef __cplusplus
}
#endif
#endif /* MRAG_SEARCH_COLLAPSED_H_ */
