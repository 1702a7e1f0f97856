// Filtered search (mrag_index_search_filtered): top-k over an allow-set of corpus rows.
//   path M (mask):    the FILT instances of K2 / K2s score every row and drop the disallowed ones in the epilogue.
//   path C (compact): the allowed rows are gathered into a scratch corpus (ascending, so the row-ascending tie-break
//                     carries over), the unchanged search runs over them, and the ids are mapped back.
// The allow-set lives on the device as a bitset (bit r%32 of word r/32) padded with zero words to whole 256-row tiles.
// This file: the allow-set kernels, the gather and the id remap of path C, and the host side shared by
// mrag_index_search_filtered and the exact path of mrag_ivf_search_filtered (declared in common.h).
#include "bf_kernels.h"

namespace mrag {

constexpr int FW_PER_THREAD = 4;                    // bitset words per thread of the count / emit kernels
constexpr int FW_BLOCK = 256 * FW_PER_THREAD;       // words per block

// byte mask (nonzero = allowed) -> bitset, one ballot per 64 rows; the grid covers every padded word
__global__ void allow_pack_bytes_kernel(const uint8_t* __restrict__ bytes, int64_t n, uint32_t* __restrict__ bits) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const unsigned long long b = __ballot(r < n && bytes[r] != 0);
  const int lane = threadIdx.x & 63;
  if (lane == 0) bits[r >> 5] = (uint32_t)b;
  if (lane == 32) bits[r >> 5] = (uint32_t)(b >> 32);
}

// word w of the bitset with the bits of rows >= n cleared
__device__ __forceinline__ uint32_t allow_word(const uint32_t* __restrict__ bits, int64_t w, int64_t n) {
  const int64_t rem = n - w * 32;
  if (rem <= 0) return 0u;
  const uint32_t x = bits[w];
  return rem < 32 ? (x & ((1u << rem) - 1u)) : x;
}

// block-wide exclusive scan of one int per thread (256 threads); returns the block total through *total
__device__ __forceinline__ int block_excl_scan256(int v, int* ws, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off);
    if (lane >= off) incl += o;
  }
  if (lane == 63) ws[wv] = incl;
  __syncthreads();
  int before = 0;
  for (int i = 0; i < wv; ++i) before += ws[i];
  *total = ws[0] + ws[1] + ws[2] + ws[3];
  __syncthreads();
  return before + incl - v;
}

// allowed rows per block of FW_BLOCK words
__global__ void allow_count_kernel(const uint32_t* __restrict__ bits, int64_t n, int64_t nwords, int* __restrict__ blk) {
  __shared__ int ws[4];
  const int64_t w0 = (int64_t)blockIdx.x * FW_BLOCK + threadIdx.x * FW_PER_THREAD;
  int c = 0;
#pragma unroll
  for (int u = 0; u < FW_PER_THREAD; ++u)
    if (w0 + u < nwords) c += __popc(allow_word(bits, w0 + u, n));
  int tot;
  (void)block_excl_scan256(c, ws, &tot);
  if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

// one block: blk[] -> exclusive prefix, *total = allowed rows
__global__ void allow_scan_kernel(int* __restrict__ blk, int nblk, int* __restrict__ total) {
  __shared__ int ws[4];
  int carry = 0;
  for (int b0 = 0; b0 < nblk; b0 += 256) {
    const int i = b0 + threadIdx.x;
    const int v = i < nblk ? blk[i] : 0;
    int tot;
    const int ex = block_excl_scan256(v, ws, &tot);
    if (i < nblk) blk[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *total = carry;
}

// ascending list of the allowed rows: thread t of block b owns words b*FW_BLOCK + t*FW_PER_THREAD .. + FW_PER_THREAD-1
__global__ void allow_emit_kernel(const uint32_t* __restrict__ bits, int64_t n, int64_t nwords, const int* __restrict__ blk_excl,
                                  int* __restrict__ rows) {
  __shared__ int ws[4];
  const int64_t w0 = (int64_t)blockIdx.x * FW_BLOCK + threadIdx.x * FW_PER_THREAD;
  uint32_t x[FW_PER_THREAD];
  int c = 0;
#pragma unroll
  for (int u = 0; u < FW_PER_THREAD; ++u) {
    x[u] = w0 + u < nwords ? allow_word(bits, w0 + u, n) : 0u;
    c += __popc(x[u]);
  }
  int tot;
  int o = blk_excl[blockIdx.x] + block_excl_scan256(c, ws, &tot);
#pragma unroll
  for (int u = 0; u < FW_PER_THREAD; ++u)
    for (uint32_t b = x[u]; b; b &= b - 1u) rows[o++] = (int)((w0 + u) * 32 + __builtin_ctz(b));
}

// compacted corpus: row i = stored row rows[i] for i < m, zeros up to m_pad (one wave per row, 16 B per lane)
__global__ void gather_rows_kernel(const uint16_t* __restrict__ src, int ld, const int* __restrict__ rows, int64_t m,
                                   int64_t m_pad, uint16_t* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= m_pad) return;
  const int lane = threadIdx.x & 63, nv = ld / 8;
  uint4* d = (uint4*)(dst + (size_t)i * ld);
  if (i < m) {
    const uint4* s = (const uint4*)(src + (size_t)rows[i] * ld);
    for (int c = lane; c < nv; c += 64) d[c] = s[c];
  } else {
    for (int c = lane; c < nv; c += 64) d[c] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// compacted position -> id_base + stored row; empty slots stay -1
__global__ void remap_ids_kernel(int64_t* __restrict__ ids, int64_t tot, const int* __restrict__ rows, int64_t id_base) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < tot) {
    const int64_t v = ids[i];
    ids[i] = v < 0 ? -1 : (int64_t)rows[v] + id_base;
  }
}

// ---- filtered search: AUTO's choice between path M and path C ------------------------------------------------------
// Path C pays a gather of the m allowed rows (read + write of m x ld x 2 B) and searches m rows; path M searches all n.
// In the streaming regime (a handful of queries, HBM-bound) a search costs ~ its corpus bytes, so C costs ~ 3m against n;
// the batch regime is MFMA-bound and C's gather is small next to the search.  Fractions from tools/perf_filter.py
// (DESIGN.md "Filtered search").
constexpr double FILTER_STREAM_FRAC = 0.25;     // streaming regime: C when m <= FILTER_STREAM_FRAC * n
constexpr double FILTER_BATCH_FRAC = 0.80;      // batch regime: C when m <= FILTER_BATCH_FRAC * n
constexpr double FILTER_SCRATCH_MB = 4096.0;    // C only when the compacted corpus fits this many MiB
int filter_choose_path(int64_t nq, int k, int64_t n, int64_t m, int ld) {
  if ((double)round_up(m, TM) * ld * 2 > FILTER_SCRATCH_MB * 1048576.0) return MRAG_FILTER_MASK;
  // the regime bf_launch runs for the unfiltered search over n rows
  const BfRegime regime = bf_regime(nq, k, n, false);
  // k > 64 over fewer than 64 compacted tiles leaves the wide-batch path for the streaming kernel, 8 queries per launch:
  // 1 000 queries x 1M x 768 at k = 200 and 1 % of the rows measured 6.0 ms compacted against 2.4 ms masked
  if (regime == BF_WIDE_BATCH && bf_regime(nq, k, m, false) != BF_WIDE_BATCH) return MRAG_FILTER_MASK;
  return (double)m <= (regime == BF_STREAM ? FILTER_STREAM_FRAC : FILTER_BATCH_FRAC) * (double)n ? MRAG_FILTER_COMPACT : MRAG_FILTER_MASK;
}

// ---- filtered search over prepared operands (mrag_index_search_filtered, and the exact path of mrag_ivf_search_filtered)
// layout of FilterWork::fwork: allowed count (word 0) | per-block counts at byte 256 | ascending allowed rows
static int64_t filter_nwords(int64_t n) { return round_up(std::max<int64_t>(n, 1), TM) / 32; }   // bitset padded to whole tiles (the kernels read 8 words per tile)
static int filter_nblk(int64_t n) { return (int)((filter_nwords(n) + FW_BLOCK - 1) / FW_BLOCK); }
static size_t filter_off_rows(int64_t n) { return (size_t)round_up(256 + (int64_t)filter_nblk(n) * 4, 256); }

static int filter_count_on_device(FilterWork& w, int64_t n, hipStream_t stream) {
  const int64_t nwords = filter_nwords(n);
  const int nblk = filter_nblk(n);
  int* d_blk = (int*)((char*)w.fwork.p + 256);
  hipLaunchKernelGGL(allow_count_kernel, dim3((unsigned)nblk), dim3(256), 0, stream, (const uint32_t*)w.fbits.p, n, nwords, d_blk);
  hipLaunchKernelGGL(allow_scan_kernel, dim3(1), dim3(256), 0, stream, d_blk, nblk, (int*)w.fwork.p);
  MRAG_HIP(hipGetLastError());
  w.counted = true;
  return MRAG_OK;
}

int filter_upload(FilterWork& w, const void* allow, int64_t n, int allow_format, int allow_is_device, bool want_count, int64_t* m_out,
                  hipEvent_t ev_begin, hipStream_t stream) {
  const int64_t nwords = filter_nwords(n);
  const int64_t in_words = (n + 31) / 32;
  MRAG_TRY(w.fbits.ensure((size_t)nwords * 4));
  MRAG_TRY(w.fwork.ensure(filter_off_rows(n) + (size_t)std::max<int64_t>(n, 1) * 4));
  uint32_t* bits = (uint32_t*)w.fbits.p;
  w.counted = false;                  // d_blk / the allowed count hold this call's counts
  int64_t m = -1;
  if (n == 0 || allow_is_device) MRAG_HIP(hipEventRecord(ev_begin, stream));
  if (n == 0) {
    m = 0;
  } else if (!allow_is_device) {
    // host allow-set: packed and counted here, no read-back
    if (!w.ev_fbits) MRAG_TRY(w.ev_fbits.create(false));
    else MRAG_HIP(hipEventSynchronize(w.ev_fbits));       // the previous copy out of the staging buffer is done
    MRAG_TRY(w.h_fbits.ensure((size_t)nwords * 4));
    uint32_t* hb = (uint32_t*)w.h_fbits.p;
    memset(hb, 0, (size_t)nwords * 4);
    if (allow_format == MRAG_ALLOW_BITS32) {
      memcpy(hb, allow, (size_t)in_words * 4);
    } else {
      const uint8_t* b = (const uint8_t*)allow;
      for (int64_t r = 0; r < n; ++r) if (b[r]) hb[r >> 5] |= 1u << (r & 31);
    }
    if (n & 31) hb[in_words - 1] &= (1u << (n & 31)) - 1u;
    m = 0;
    for (int64_t i = 0; i < in_words; ++i) m += __builtin_popcount(hb[i]);
    MRAG_HIP(hipEventRecord(ev_begin, stream));
    MRAG_HIP(hipMemcpyAsync(bits, hb, (size_t)nwords * 4, hipMemcpyHostToDevice, stream));
    MRAG_HIP(hipEventRecord(w.ev_fbits, stream));
  } else {
    if (allow_format == MRAG_ALLOW_BITS32) {
      MRAG_HIP(hipMemsetAsync(bits, 0, (size_t)nwords * 4, stream));
      MRAG_HIP(hipMemcpyAsync(bits, allow, (size_t)in_words * 4, hipMemcpyDeviceToDevice, stream));
    } else {
      hipLaunchKernelGGL(allow_pack_bytes_kernel, dim3((unsigned)(nwords * 32 / 256)), dim3(256), 0, stream, (const uint8_t*)allow, n, bits);
      MRAG_HIP(hipGetLastError());
    }
    MRAG_TRY(filter_count_on_device(w, n, stream));
    if (want_count) {                 // the caller needs the count on the host: one read-back
      int hm = 0;
      MRAG_HIP(hipMemcpyAsync(&hm, w.fwork.p, sizeof(int), hipMemcpyDeviceToHost, stream));
      MRAG_HIP(hipStreamSynchronize(stream));
      m = hm;
    }
  }
  *m_out = m;
  return MRAG_OK;
}

int filter_search(FilterWork& w, BfLaunch a, int path, int64_t m, hipStream_t stream) {
  const int64_t n = a.n_rows;
  if (path == MRAG_FILTER_MASK) {
    a.allow = (const uint32_t*)w.fbits.p;
    return bf_launch(a);
  }
  // path C: ascending allowed rows -> compacted corpus (zero padded to a whole tile) -> the unchanged search -> ids
  if (!w.counted) MRAG_TRY(filter_count_on_device(w, n, stream));
  const int nblk = filter_nblk(n);
  const int* d_blk = (const int*)((char*)w.fwork.p + 256);
  int* d_rows = (int*)((char*)w.fwork.p + filter_off_rows(n));
  hipLaunchKernelGGL(allow_emit_kernel, dim3((unsigned)nblk), dim3(256), 0, stream, (const uint32_t*)w.fbits.p, n, filter_nwords(n),
                     d_blk, d_rows);
  const int64_t m_pad = round_up(m, TM);
  MRAG_TRY(w.fcomp.ensure((size_t)m_pad * a.ld * 2));
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((m_pad + 3) / 4)), dim3(256), 0, stream, a.corpus, a.ld, (const int*)d_rows,
                     m, m_pad, (uint16_t*)w.fcomp.p);
  MRAG_HIP(hipGetLastError());
  const int64_t id_base = a.id_base;
  a.corpus = (const uint16_t*)w.fcomp.p;
  a.n_rows = m;
  a.id_base = 0;
  MRAG_TRY(bf_launch(a));
  const int64_t tot = a.nq * a.k;
  hipLaunchKernelGGL(remap_ids_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream, a.out_ids, tot, (const int*)d_rows,
                     id_base);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

// the allow-set arguments of a filtered search over n rows: one row each, a known format, a known path (`kind` names the
// path enum in the message: the dense and the IVF enums both run 0..2 with AUTO = 0)
int check_allow_args(int64_t allow_rows, int64_t n, int allow_format, int path, const char* kind) {
  static_assert((int)MRAG_IVF_FILTER_AUTO == (int)MRAG_FILTER_AUTO && (int)MRAG_IVF_FILTER_PROBE == (int)MRAG_FILTER_MASK &&
                (int)MRAG_IVF_FILTER_EXACT == (int)MRAG_FILTER_COMPACT, "one range check serves both path enums");
  if (allow_rows != n) return fail(MRAG_ERR_INVALID, "allow-set covers %lld rows, the index holds %lld", (long long)allow_rows, (long long)n);
  if (allow_format != MRAG_ALLOW_BITS32 && allow_format != MRAG_ALLOW_BYTES) return fail(MRAG_ERR_INVALID, "unknown allow format %d", allow_format);
  if (path != MRAG_FILTER_AUTO && path != MRAG_FILTER_MASK && path != MRAG_FILTER_COMPACT) return fail(MRAG_ERR_INVALID, "unknown %s path %d", kind, path);
  return MRAG_OK;
}

}  // namespace mrag
