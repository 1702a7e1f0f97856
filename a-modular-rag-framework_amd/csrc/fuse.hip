// Channel fusion on the device (a7): the arithmetic of HybridRetrievalBackend.run (retrieval_backend.py:336-372) over the
// three channels' (key, score) lists, for MANY questions per call -- key = the rank of the hit's NORMALISED id among the
// ids the host binding ranks, so ascending key == ascending id, the declared tie order:
//   per channel  dedupe by key, strictly larger score wins, the first one met among equals (:336-348)
//                min-max over the kept scores, all-equal / empty -> 0.0 (:296-301)
//   union        score = a_t*ts + a_g*gs + a_d*ds, left to right, no contraction (:363)
//   sort (score desc, key asc), keep top_k (:371-372)
// fp64, bit for bit the reference's values, wherever a question stands in the batch.  There is one fusion path:
// mrag_fuse_topk_batch runs it for its questions, mrag_fuse_topk is a batch of one question without payloads.
//
//   grid       one workgroup per question; blockDim = half the largest question's padded size, 64 .. 1024 threads
//   LDS        dynamic, sized by the largest question of the launch; a question of n entries works on P = the power of two
//              >= n (at least 2).  The entries are staged ONCE and stay there until the outputs are written:
//                head   64 B      lo[3], hi[3] of the channels
//                score  8 P       the entry's score, overwritten by its min-max norm once lo / hi are known
//                fused  8 P       fused score of the u-th distinct key
//                key    4 P
//                pay    4 P       the entry's payload (-1 without payloads)
//                scan   4 T       the block scan's partial counts (T = blockDim)
//                perm   2 P       sort 1: entry indexes; sort 2 (reused): distinct-key ordinals
//                ent    2 * 3 P   per channel and distinct key: its kept entry, 0xFFFF = the channel has none
//                kept   1 P       by entry: represents its key in its channel
//                flag   1 P       by sorted position: bit 0 kept entry, bit 1 first entry of its key
//              34 P + 4 T + 64 bytes: 17.7 KiB for a pool of 400 entries (P = 512: nine workgroups per CU), 140 KiB at
//              the limit of 4096 entries, inside the 160 KiB of a CU.
//   sort 1     bitonic over entry indexes by (key asc, channel asc, score desc, index asc).  Scores are compared as
//              doubles, never as bit patterns: -0.0 == +0.0 and the lower index -- the first one met -- stays in front.
//              The first entry of a (key, channel) run is the one the reference's dedupe keeps.
//   min-max    one wave per channel walks the channel's kept entries in index order, every lane keeping its first
//              strict minimum / maximum; the wave's reduction prefers the lower index among equal values, so lo and hi
//              are the FIRST min / max met (their sign matters when both zeros are present: score - lo).
//   union      a block scan over "first entry of its key" numbers the distinct keys in key order: u = 0 .. U-1; the kept
//              entries write themselves into ent[channel][u]
//   sort 2     bitonic over u by (fused desc, u asc); u ascending is key ascending
//   output     the first min(top_k, U) of sort 2; the slots up to out_stride hold (-1, 0.0)
// Work per question: O(P log^2 P) compare-exchanges in LDS; global memory is read once and written once.
#include "common.h"

#include <algorithm>
#include <vector>

namespace mrag {

constexpr int FUSE_MAX = 4096;               // entries of one question over its three channels
constexpr int FUSE_HEAD = 64;                // bytes
constexpr unsigned short FUSE_NONE = 0xFFFF;

__host__ __device__ inline int fuse_pow2(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}
static inline size_t fuse_lds_bytes(int P, int T) { return (size_t)FUSE_HEAD + (size_t)34 * P + (size_t)4 * T; }

// bitonic sort of perm[0 .. P) (P a power of two, distinct elements) under a strict total order; ends on a barrier
template <class Less>
__device__ inline void fuse_sort(unsigned short* perm, int P, Less less) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += blockDim.x) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
        const unsigned short a = perm[i], b = perm[l];
        if (less((int)b, (int)a) == ((i & k) == 0)) { perm[i] = b; perm[l] = a; }
      }
      __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void fuse_kernel(const int32_t* __restrict__ chan_ptr, const int32_t* __restrict__ keys,
                                                    const double* __restrict__ scores, const int32_t* __restrict__ payload,
                                                    const int32_t* __restrict__ top_k, double a_t, double a_g, double a_d,
                                                    int out_stride, int32_t* __restrict__ out_key, double* __restrict__ out_fused,
                                                    double* __restrict__ out_nt, double* __restrict__ out_ng,
                                                    double* __restrict__ out_nd, int32_t* __restrict__ out_payload,
                                                    int32_t* __restrict__ out_n) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char fuse_lds[];
  const int g = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int base = chan_ptr[3 * (size_t)g];
  const int c1 = chan_ptr[3 * (size_t)g + 1] - base, c2 = chan_ptr[3 * (size_t)g + 2] - base, n = chan_ptr[3 * (size_t)g + 3] - base;
  const int P = fuse_pow2(n);
  double* s_lo = (double*)fuse_lds;
  double* s_hi = s_lo + 3;
  double* s_score = (double*)(fuse_lds + FUSE_HEAD);
  double* s_fused = s_score + P;
  int32_t* s_key = (int32_t*)(s_fused + P);
  int32_t* s_pay = s_key + P;
  int* s_scan = s_pay + P;
  unsigned short* perm = (unsigned short*)(s_scan + T);
  unsigned short* ent = perm + P;                  // [3][P]
  unsigned char* kept = (unsigned char*)(ent + 3 * P);
  unsigned char* flag = kept + P;
  auto chan = [=](int i) { return i >= c2 ? 2 : (i >= c1 ? 1 : 0); };

  for (int i = tid; i < P; i += T) {
    if (i < n) {
      s_key[i] = keys[(size_t)base + i];
      s_score[i] = scores[(size_t)base + i];
      s_pay[i] = payload ? payload[(size_t)base + i] : -1;
    }
    perm[i] = (unsigned short)i;
    kept[i] = 0;
    flag[i] = 0;
    ent[i] = ent[P + i] = ent[2 * P + i] = FUSE_NONE;
  }
  __syncthreads();

  // 1) sort 1: real entries before the padding (index >= n), then (key, channel, score desc, index)
  fuse_sort(perm, P, [=](int a, int b) {
    if (b >= n) return a < n || a < b;
    if (a >= n) return false;
    const int ka = s_key[a], kb = s_key[b];
    if (ka != kb) return ka < kb;
    const int ca = chan(a), cb = chan(b);
    if (ca != cb) return ca < cb;
    const double sa = s_score[a], sb = s_score[b];
    if (sa > sb) return true;
    if (sa < sb) return false;
    return a < b;
  });

  // 2) run heads: the first entry of a (key, channel) run is kept, the first of a key run starts a distinct key
  for (int p = tid; p < n; p += T) {
    const int i = perm[p];
    bool run = true, kh = true;
    if (p > 0) {
      const int q = perm[p - 1];
      run = s_key[q] != s_key[i];
      kh = run || chan(q) != chan(i);
    }
    flag[p] = (unsigned char)((kh ? 1 : 0) | (run ? 2 : 0));
    kept[i] = kh ? 1 : 0;
  }
  __syncthreads();

  // 3) per channel the first minimum and the first maximum of the kept scores, in index order
  {
    const int lane = tid & 63, wave = tid >> 6, n_waves = T >> 6;
    for (int c = wave; c < 3; c += n_waves) {
      const int lo_i = c == 0 ? 0 : (c == 1 ? c1 : c2), hi_i = c == 0 ? c1 : (c == 1 ? c2 : n);
      double vmin = 0.0, vmax = 0.0;
      int imin = -1, imax = -1;                  // -1: this lane has met no kept entry
      for (int j = lo_i + lane; j < hi_i; j += 64) {
        if (!kept[j]) continue;
        const double v = s_score[j];
        if (imin < 0) { vmin = vmax = v; imin = imax = j; }
        else {
          if (v < vmin) { vmin = v; imin = j; }
          if (v > vmax) { vmax = v; imax = j; }
        }
      }
      for (int off = 32; off > 0; off >>= 1) {
        const double omin = __shfl_xor(vmin, off, 64), omax = __shfl_xor(vmax, off, 64);
        const int oimin = __shfl_xor(imin, off, 64), oimax = __shfl_xor(imax, off, 64);
        if (oimin >= 0 && (imin < 0 || omin < vmin || (omin == vmin && oimin < imin))) { vmin = omin; imin = oimin; }
        if (oimax >= 0 && (imax < 0 || omax > vmax || (omax == vmax && oimax < imax))) { vmax = omax; imax = oimax; }
      }
      if (lane == 0) { s_lo[c] = vmin; s_hi[c] = vmax; }
    }
  }
  __syncthreads();
  for (int i = tid; i < n; i += T) {
    if (!kept[i]) continue;
    const int c = chan(i);
    const double lo = s_lo[c], hi = s_hi[c];
    s_score[i] = hi > lo ? (s_score[i] - lo) / (hi - lo) : 0.0;
  }

  // 4) union: number the distinct keys in key order (block scan over the key-run heads of a thread's chunk of
  //    positions), every kept entry becomes its channel's entry of its key
  const int chunk = P >= T ? P / T : 1;
  const int p_lo = min(tid * chunk, n), p_hi = min(p_lo + chunk, n);
  int cnt = 0;
  for (int p = p_lo; p < p_hi; ++p) cnt += (flag[p] >> 1) & 1;
  s_scan[tid] = cnt;
  __syncthreads();
  for (int off = 1; off < T; off <<= 1) {
    const int v = tid >= off ? s_scan[tid - off] : 0;
    __syncthreads();
    s_scan[tid] += v;
    __syncthreads();
  }
  const int U = s_scan[T - 1];
  {
    int r = s_scan[tid] - cnt;                   // key-run heads before this chunk
    for (int p = p_lo; p < p_hi; ++p) {
      const int f = flag[p];
      r += (f >> 1) & 1;
      if (f & 1) {
        const int i = perm[p];
        ent[chan(i) * P + (r - 1)] = (unsigned short)i;    // position 0 is a head: r >= 1
      }
    }
  }
  __syncthreads();

  // 5) fused score of every distinct key, then sort 2 over the ordinals: (fused desc, ordinal asc) = (fused desc, key asc)
  for (int u = tid; u < P; u += T) {
    if (u < U) {
      const unsigned short e0 = ent[u], e1 = ent[P + u], e2 = ent[2 * P + u];
      const double ts = e0 != FUSE_NONE ? s_score[e0] : 0.0, gs = e1 != FUSE_NONE ? s_score[e1] : 0.0,
                   ds = e2 != FUSE_NONE ? s_score[e2] : 0.0;
      s_fused[u] = a_t * ts + a_g * gs + a_d * ds;
    }
    perm[u] = (unsigned short)u;
  }
  __syncthreads();
  fuse_sort(perm, fuse_pow2(U), [=](int a, int b) {
    if (b >= U) return a < U || a < b;
    if (a >= U) return false;
    const double fa = s_fused[a], fb = s_fused[b];
    if (fa > fb) return true;
    if (fa < fb) return false;
    return a < b;
  });

  // 6) the survivors, then (-1, 0.0) up to out_stride
  const int kk = min(top_k[g], U);
  for (int r = tid; r < out_stride; r += T) {
    const size_t o = (size_t)g * out_stride + r;
    int32_t key = -1, pay[3] = {-1, -1, -1};
    double f = 0.0, nm[3] = {0.0, 0.0, 0.0};
    if (r < kk) {
      const int u = perm[r];
      f = s_fused[u];
      for (int c = 2; c >= 0; --c) {
        const unsigned short e = ent[c * P + u];
        if (e == FUSE_NONE) continue;
        key = s_key[e];
        nm[c] = s_score[e];
        pay[c] = s_pay[e];
      }
    }
    out_key[o] = key;
    out_fused[o] = f;
    out_nt[o] = nm[0];
    out_ng[o] = nm[1];
    out_nd[o] = nm[2];
    if (out_payload) { out_payload[3 * o] = pay[0]; out_payload[3 * o + 1] = pay[1]; out_payload[3 * o + 2] = pay[2]; }
  }
  if (tid == 0) out_n[g] = kk;
}

namespace {

// The fusion of n_questions >= 1 validated questions that hold at least one entry, out_stride >= 1: question g's
// out_stride slots of every output and its out_n[g].
int fuse_questions(int device, int n_questions, const int32_t* chan_ptr, const int32_t* keys, const double* scores,
                   const int32_t* payload, double alpha_text, double alpha_graph, double alpha_dense, const int32_t* top_k,
                   int out_stride, int32_t* out_keys, double* out_scores, double* out_text_norm, double* out_graph_norm,
                   double* out_dense_norm, int32_t* out_payload, int32_t* out_n, hipStream_t stream) {
  const size_t n_out = (size_t)n_questions * out_stride, E = (size_t)chan_ptr[3 * (size_t)n_questions];
  int n_max = 0;
  for (int g = 0; g < n_questions; ++g) n_max = std::max(n_max, chan_ptr[3 * (size_t)g + 3] - chan_ptr[3 * (size_t)g]);
  // one block of device memory: inputs | outputs, the 8-byte items first in each part
  auto r8 = [](size_t b) { return (b + 7) & ~(size_t)7; };
  const size_t n_ptr = 3 * (size_t)n_questions + 1;
  const size_t i_scores = 0, i_ptr = i_scores + E * 8, i_topk = i_ptr + r8(n_ptr * 4), i_keys = i_topk + r8((size_t)n_questions * 4),
               i_pay = i_keys + r8(E * 4), in_bytes = i_pay + (payload ? r8(E * 4) : 0);
  const size_t o_fused = 0, o_nt = o_fused + n_out * 8, o_ng = o_nt + n_out * 8, o_nd = o_ng + n_out * 8, o_key = o_nd + n_out * 8,
               o_pay = o_key + r8(n_out * 4), o_n = o_pay + (payload ? r8(3 * n_out * 4) : 0), out_bytes = o_n + r8((size_t)n_questions * 4);
  std::vector<char> h_in(in_bytes), h_out(out_bytes);
  memcpy(h_in.data() + i_scores, scores, E * 8);
  memcpy(h_in.data() + i_ptr, chan_ptr, n_ptr * 4);
  memcpy(h_in.data() + i_topk, top_k, (size_t)n_questions * 4);
  memcpy(h_in.data() + i_keys, keys, E * 4);
  if (payload) memcpy(h_in.data() + i_pay, payload, E * 4);

  MRAG_TRY(use_device(device));
  const int P = fuse_pow2(n_max), T = std::min(1024, std::max(64, P / 2));
  const size_t lds = fuse_lds_bytes(P, T);
  if (lds > 65536)    // above HIP's default limit of dynamic LDS the kernel's own limit is raised (a process-wide, idempotent setting)
    MRAG_HIP(hipFuncSetAttribute((const void*)fuse_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)fuse_lds_bytes(FUSE_MAX, 1024)));
  DevBuf block;
  MRAG_TRY(block.alloc(in_bytes + out_bytes));
  char *d = (char*)block.p, *d_out = d + in_bytes;
  // (run_synced: the staging vectors are in use until the stream has settled, also after a failure)
  MRAG_TRY(run_synced(stream, [&]() -> int {
    MRAG_HIP(hipMemcpyAsync(d, h_in.data(), in_bytes, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(fuse_kernel, dim3((unsigned)n_questions), dim3((unsigned)T), lds, stream, (const int32_t*)(d + i_ptr),
                       (const int32_t*)(d + i_keys), (const double*)(d + i_scores), payload ? (const int32_t*)(d + i_pay) : nullptr,
                       (const int32_t*)(d + i_topk), alpha_text, alpha_graph, alpha_dense, out_stride, (int32_t*)(d_out + o_key),
                       (double*)(d_out + o_fused), (double*)(d_out + o_nt), (double*)(d_out + o_ng), (double*)(d_out + o_nd),
                       payload ? (int32_t*)(d_out + o_pay) : nullptr, (int32_t*)(d_out + o_n));
    MRAG_HIP(hipGetLastError());
    MRAG_HIP(hipMemcpyAsync(h_out.data(), d_out, out_bytes, hipMemcpyDeviceToHost, stream));
    return MRAG_OK;
  }));
  memcpy(out_scores, h_out.data() + o_fused, n_out * 8);
  memcpy(out_text_norm, h_out.data() + o_nt, n_out * 8);
  memcpy(out_graph_norm, h_out.data() + o_ng, n_out * 8);
  memcpy(out_dense_norm, h_out.data() + o_nd, n_out * 8);
  memcpy(out_keys, h_out.data() + o_key, n_out * 4);
  if (payload) memcpy(out_payload, h_out.data() + o_pay, 3 * n_out * 4);
  memcpy(out_n, h_out.data() + o_n, (size_t)n_questions * 4);
  return MRAG_OK;
}

}  // namespace

}  // namespace mrag

using namespace mrag;

extern "C" {

// One question.  The caller's buffers hold min(top_k, entries) slots (mrag.h) and that is the stride of the one output
// row, so they take the row as it is; slots past *out_n hold (-1, 0.0).
int mrag_fuse_topk(int device, const int32_t* keys, const double* scores, int n_text, int n_graph, int n_dense,
                   double alpha_text, double alpha_graph, double alpha_dense, int top_k, int32_t* out_keys,
                   double* out_scores, double* out_text_norm, double* out_graph_norm, double* out_dense_norm,
                   int* out_n, void* stream) {
  if (!out_n) return fail(MRAG_ERR_INVALID, "out_n is NULL");
  *out_n = 0;
  if (n_text < 0 || n_graph < 0 || n_dense < 0 || top_k < 0) return fail(MRAG_ERR_INVALID, "negative size");
  const int n = n_text + n_graph + n_dense;
  if (n > FUSE_MAX) return fail(MRAG_ERR_UNSUPPORTED, "%d fusion entries exceed %d", n, FUSE_MAX);
  if (n == 0 || top_k == 0) return MRAG_OK;
  if (!keys || !scores || !out_keys || !out_scores || !out_text_norm || !out_graph_norm || !out_dense_norm)
    return fail(MRAG_ERR_INVALID, "NULL buffer");
  for (int i = 0; i < n; ++i)
    if (!(scores[i] == scores[i])) return fail(MRAG_ERR_INVALID, "NaN score at fusion entry %d", i);
  const int32_t chan_ptr[4] = {0, n_text, n_text + n_graph, n}, kk = std::min(top_k, n);
  return fuse_questions(device, 1, chan_ptr, keys, scores, nullptr, alpha_text, alpha_graph, alpha_dense, &kk, kk, out_keys,
                        out_scores, out_text_norm, out_graph_norm, out_dense_norm, nullptr, out_n, (hipStream_t)stream);
}

int mrag_fuse_topk_batch(int device, int n_questions, const int32_t* chan_ptr, const int32_t* keys, const double* scores,
                         const int32_t* payload, double alpha_text, double alpha_graph, double alpha_dense,
                         const int32_t* top_k, int out_stride, int32_t* out_keys, double* out_scores,
                         double* out_text_norm, double* out_graph_norm, double* out_dense_norm, int32_t* out_payload,
                         int32_t* out_n, void* stream) {
  if (n_questions < 0 || out_stride < 0) return fail(MRAG_ERR_INVALID, "negative n_questions / out_stride");
  if (n_questions == 0) return MRAG_OK;
  if (!out_n) return fail(MRAG_ERR_INVALID, "out_n is NULL");
  std::fill(out_n, out_n + n_questions, 0);
  if (!chan_ptr || !top_k) return fail(MRAG_ERR_INVALID, "NULL chan_ptr / top_k");
  const size_t n_out = (size_t)n_questions * out_stride;
  if (n_out && (!out_keys || !out_scores || !out_text_norm || !out_graph_norm || !out_dense_norm || (payload && !out_payload)))
    return fail(MRAG_ERR_INVALID, "NULL output buffer");

  // ---- the whole batch is validated before any device work
  if (chan_ptr[0] != 0) return fail(MRAG_ERR_INVALID, "chan_ptr must start at 0");
  for (int g = 0; g < n_questions; ++g) {
    const int32_t* p = chan_ptr + 3 * (size_t)g;
    if (p[1] < p[0] || p[2] < p[1] || p[3] < p[2]) return fail(MRAG_ERR_INVALID, "chan_ptr decreases inside question %d", g);
    if ((int64_t)p[3] - p[0] > FUSE_MAX)
      return fail(MRAG_ERR_UNSUPPORTED, "question %d has %lld fusion entries, more than %d", g, (long long)p[3] - p[0], FUSE_MAX);
    if (top_k[g] < 0 || top_k[g] > out_stride)
      return fail(MRAG_ERR_INVALID, "top_k = %d of question %d outside [0, out_stride = %d]", top_k[g], g, out_stride);
  }
  const size_t E = (size_t)chan_ptr[3 * (size_t)n_questions];
  if (E && (!keys || !scores)) return fail(MRAG_ERR_INVALID, "NULL keys / scores");
  for (int g = 0; g < n_questions; ++g)
    for (int i = chan_ptr[3 * (size_t)g]; i < chan_ptr[3 * (size_t)g + 3]; ++i)
      if (!(scores[i] == scores[i]))
        return fail(MRAG_ERR_INVALID, "NaN score at fusion entry %d of question %d", i - chan_ptr[3 * (size_t)g], g);

  if (n_out == 0) return MRAG_OK;                        // every top_k is 0
  if (E == 0) {                                          // only empty questions
    std::fill(out_keys, out_keys + n_out, (int32_t)-1);
    for (double* o : {out_scores, out_text_norm, out_graph_norm, out_dense_norm}) std::fill(o, o + n_out, 0.0);
    if (payload) std::fill(out_payload, out_payload + 3 * n_out, (int32_t)-1);
    return MRAG_OK;
  }
  return fuse_questions(device, n_questions, chan_ptr, keys, scores, payload, alpha_text, alpha_graph, alpha_dense, top_k, out_stride,
                        out_keys, out_scores, out_text_norm, out_graph_norm, out_dense_norm, out_payload, out_n, (hipStream_t)stream);
}

}  // extern "C"
