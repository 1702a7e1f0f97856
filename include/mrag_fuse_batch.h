/*
 * mrag_fuse_batch.h -- the batched channel fusion of libmrag_hip.so: one entry point added to the C ABI of mrag.h.
 *
 * mrag.h includes this header, so a program that includes mrag.h has it; the conventions (status codes, host buffers,
 * `stream`) are mrag.h's.  mrag.h itself keeps the 64 entry points it had, and MRAG_ABI_VERSION stays 1.
 */
#ifndef MRAG_FUSE_BATCH_H_
#define MRAG_FUSE_BATCH_H_

#include "mrag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The fusion of mrag_fuse_topk for a BATCH of questions (retrieval_backend.py:336-372, applied per question): question g's
 * text, graph and dense entries are the three consecutive ranges of keys / scores / payload that start at chan_ptr[3g]
 * (chan_ptr: int32 [3 * n_questions + 1], chan_ptr[0] = 0, non-decreasing).  Per question and channel: dedupe by key (a
 * strictly larger score wins, on equal scores the first entry met keeps the slot), min-max over the kept scores (an empty
 * channel or hi <= lo normalises to 0.0; among equal values the first one met is the min / max); fused score =
 * alpha_text*ts + alpha_graph*gs + alpha_dense*ds, left to right in fp64 without contraction; order (fused desc, key asc);
 * top_k[g] entries are kept.  Question g's outputs are bit for bit what mrag_fuse_topk returns for g's entries alone,
 * wherever g stands in the batch.  Keys are compared only inside a question; ascending key must mean ascending
 * normalised id.
 * payload (optional, NULL: none) is an opaque int32 per entry.  With it, out_payload [n_questions][out_stride][3] holds
 * for every survivor the payload of its kept entry in the text, graph and dense channel, -1 where that channel has none
 * for the key -- which text row and which dense row stand behind a survivor, without a second pass.
 * Outputs are [n_questions][out_stride]: key, fused score and the three norms; out_n [n_questions] = min(top_k[g],
 * distinct keys of g).  The slots past out_n[g] hold key -1, payload -1 and 0.0.
 * Refused before any device work, every out_n zeroed, the message naming the question: a negative size, a chan_ptr that
 * does not start at 0 or decreases, top_k[g] < 0 or > out_stride, a NULL required buffer, a NaN score (the message names
 * the entry too) -- MRAG_ERR_INVALID; a question of more than 4096 entries -- MRAG_ERR_UNSUPPORTED, the limit of
 * mrag_fuse_topk.  n_questions == 0 and a batch of empty questions are MRAG_OK.
 * All buffers are host buffers.  One workgroup per question sorts the question's entries in LDS, O(n log^2 n); the call
 * makes one device allocation, one upload, one launch, one download and synchronises `stream` once, whatever the batch. */
int mrag_fuse_topk_batch(int device, int n_questions, const int32_t* chan_ptr, const int32_t* keys, const double* scores,
                         const int32_t* payload, double alpha_text, double alpha_graph, double alpha_dense,
                         const int32_t* top_k, int out_stride, int32_t* out_keys, double* out_scores, double* out_text_norm,
                         double* out_graph_norm, double* out_dense_norm, int32_t* out_payload, int32_t* out_n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MRAG_FUSE_BATCH_H_ */
