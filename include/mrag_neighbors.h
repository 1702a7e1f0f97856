/*
 * mrag_neighbors.h -- neighbour expansion of search hits, the graph channel of the hybrid retrieval on the device: two
 * entry points added to the C ABI of mrag.h.
 *
 * mrag.h includes this header, so a program that includes mrag.h has them; the conventions (status codes, handles, host
 * and device buffers, `stream`) are mrag.h's.  mrag.h itself keeps the 64 entry points it had, and MRAG_ABI_VERSION
 * stays 1.
 */
#ifndef MRAG_NEIGHBORS_H_
#define MRAG_NEIGHBORS_H_

#include "mrag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The rows around a question's seed rows, inside the seeds' own documents.  The index holds one int32 key per row
 * (mrag_index_set_row_keys); the RUN of a row is the maximal interval of consecutive rows that carry its key (equal keys
 * that are not contiguous are different runs) -- the sentences of one document, stored in a row, are one run, and the
 * neighbours of a row are the adjacent rows of its run.
 *
 * Per question q: seeds [nq][seed_stride] holds global ids (int64, host or device: seeds_on_device).  An id equal to -1
 * is skipped, and so is any id outside [id_base, id_base + n): nothing is read back and nothing is refused for them.
 * With local row r = id - id_base, the REACH of a seed is [max(run_lo, r - window), min(run_hi, r + window)].  For every
 * distinct row c inside some seed's reach
 *     dist(c)  = the minimum of |c - r| over the seeds whose reach holds c
 *     seed(c)  = the lowest seed POSITION (column of seeds[q]) that attains it (duplicate seeds: the lowest position)
 *     score(c) = decay[dist(c)]
 * and the distinct rows are ordered by (dist asc, seed position asc, row asc), a strict total order.  The first m are
 * written to out_scores (fp32), out_ids (int64, id_base + c), out_dist (int32) and out_seed (int32, the position), each
 * [nq][m]; out_dist and out_seed may be NULL.  The slots past the distinct rows hold (-inf, -1, -1, -1).  A question's
 * outputs depend on its own seed row alone, not on where it stands in the call.
 *
 * decay is float [window + 1], ALWAYS a host array (it travels by value in the kernel arguments); it must be finite and
 * must not increase, so that "by distance" is "by score, stable".  This is the multi-source breadth-first search of
 * graph_utils.expand_qmatch_neighbors along next_in_doc edges, as a mapping row -> (score, distance); the order among
 * equal scores is this library's own (the reference's is the iteration order of a set).
 *
 * Stream contract.  With device seeds and device outputs the call is ONE launch on `stream`: no synchronisation, no
 * read-back.  With a host buffer on either side it is one upload (host seeds), one launch, one download (host outputs)
 * and one synchronisation of `stream`, whatever nq.
 *
 * Refused before any device work, the outputs untouched, the message naming the cause.  MRAG_ERR_INVALID: a dead
 * handle; nq < 0, seed_stride < 0, m < 1 or window < 0; a NULL required buffer (seeds unless nq * seed_stride == 0,
 * decay, out_scores, out_ids); a decay entry that is NaN or infinite, or a decay table that increases; no keys set on
 * an index that holds rows, or keys set for another row count.  MRAG_ERR_UNSUPPORTED: window > 16; seed_stride > 256;
 * seed_stride * (2 * window + 1) > 4096; m > 4096.  nq == 0 is MRAG_OK without device work.  seed_stride == 0 gives
 * only padding slots, and so does an empty index, which needs no keys. */
int mrag_index_expand_neighbors(mrag_handle h, const int64_t* seeds, int64_t nq, int seed_stride, int seeds_on_device,
                                int window, const float* decay, int m, float* out_scores, int64_t* out_ids,
                                int32_t* out_dist, int32_t* out_seed, int out_on_device, void* stream);

/* What the LAST completed mrag_index_expand_neighbors on this index did: the questions it served, the entries of the
 * largest question (= seed_stride * (2 * window + 1)) and the window.  Any output may be NULL.  MRAG_ERR_INVALID before
 * the first completed call. */
int mrag_index_last_neighbors(mrag_handle h, int64_t* out_questions, int64_t* out_max_entries, int64_t* out_window);

#ifdef __cplusplus
}
#endif
#endif /* MRAG_NEIGHBORS_H_ */
