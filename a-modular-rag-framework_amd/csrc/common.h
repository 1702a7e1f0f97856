// Internal helpers shared by the libmrag_hip translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <mutex>
#include <utility>
#include <unordered_map>
#include <string>
#include <vector>

#include "../../include/mrag.h"

namespace mrag {

void set_error(const char* fmt, ...);
int fail(int code, const char* fmt, ...);

#define MRAG_HIP(expr)                                                                          \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess) {                                                                     \
      return ::mrag::fail(_e == hipErrorOutOfMemory ? MRAG_ERR_OOM : MRAG_ERR_HIP,              \
                          "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,      \
                          __LINE__);                                                            \
    }                                                                                           \
  } while (0)

#define MRAG_TRY(expr)            \
  do {                            \
    int _s = (expr);              \
    if (_s != MRAG_OK) return _s; \
  } while (0)

// verifies a usable device and makes it current
int use_device(int device);

enum HandleKind : uint32_t { KIND_BF_INDEX = 1, KIND_IVF = 2, KIND_ENCODER = 3, KIND_BM25 = 4 };

struct Object {
  HandleKind kind;
  int device;
  virtual ~Object() {}
};

mrag_handle register_object(Object* o);
Object* lookup(mrag_handle h, HandleKind kind);  // nullptr + error set when invalid
// removes the handle from the registry and deletes its object behind the device's queued work: the owners' destructors
// must not free what a kernel still reads
int destroy_object(mrag_handle h, HandleKind kind);

// ---- owners of device resources --------------------------------------------------------------------------------------
// Each frees what it holds in its destructor, moves and does not copy.  They are members of handles and locals of entry
// points, never parameters (launch structs keep plain DevBuf* and raw views), and never static or at namespace scope: a
// destructor that runs after the HIP runtime has shut down can crash.  hipFree waits for the device, so a local buffer
// that dies on an early return behind queued work is safe; host memory that an async copy reads is not owned here and
// still needs its synchronisation.
#define MRAG_MOVE_ONLY(T)                          \
  T() = default;                                   \
  T(const T&) = delete;                            \
  T& operator=(const T&) = delete;                 \
  T(T&& o) noexcept { swap(o); }                   \
  T& operator=(T&& o) noexcept { swap(o); return *this; }

// device buffer
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  MRAG_MOVE_ONLY(DevBuf)
  ~DevBuf();
  void swap(DevBuf& o) { std::swap(p, o.p); std::swap(bytes, o.bytes); }
  int ensure(size_t need);   // grows with 25 % head-room, the exact size if that fails (contents NOT preserved)
  // storage that is sized once: exactly n bytes, replacing what was held; `what` names it in the refusal ("hipMalloc(n) for <what> failed")
  int alloc(size_t n, const char* what = nullptr);
};
// an exact-size DevBuf that reads as its T*
template <typename T>
struct DevArray : DevBuf {
  operator T*() const { return (T*)p; }
};

struct Event {
  hipEvent_t e = nullptr;
  MRAG_MOVE_ONLY(Event)
  ~Event();
  void swap(Event& o) { std::swap(e, o.e); }
  int create(bool timing);   // once: a no-op on an event that exists
  operator hipEvent_t() const { return e; }
};

// pinned host staging
struct PinnedBuf {
  void* p = nullptr;
  size_t bytes = 0;
  MRAG_MOVE_ONLY(PinnedBuf)
  ~PinnedBuf();
  void swap(PinnedBuf& o) { std::swap(p, o.p); std::swap(bytes, o.bytes); }
  int ensure(size_t need);   // grows to exactly `need` (contents NOT preserved)
};

static inline size_t dtype_size(int dt) {
  switch (dt) { case MRAG_F32: return 4; case MRAG_F16: case MRAG_BF16: return 2; case MRAG_F64: return 8; default: return 0; }
}

// Runs `enqueue` and synchronises the stream whatever it returns: asynchronous copies that read host vectors or the
// caller's host buffers have finished before those go out of scope.  Returns the first failure.
template <class F>
static inline int run_synced(hipStream_t stream, F&& enqueue) {
  const int status = enqueue();
  if (status != MRAG_OK) {
    (void)hipStreamSynchronize(stream);
    return status;
  }
  MRAG_HIP(hipStreamSynchronize(stream));
  return MRAG_OK;
}

static inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// rows of any supported dtype -> normalised/rounded storage rows (fp16/bf16), zero padded to `ld`
// src/dst are device pointers.  dst row r lives at dst + r*ld (16-bit elements).
int launch_prep_rows(const void* src, int src_dtype, int64_t n, int dim, void* dst, int ld,
                     int storage_dtype, int normalize, hipStream_t stream);


// Internal operand type of the fp8 scan copy (mrag_index_search_fp8): OCP e4m3fn bytes.  Not an ABI dtype: a BfLaunch
// with this dtype carries `ld` in 16-bit units (bytes per row / 2), so every stage and tile offset stays as it is.
constexpr int MRAG_DT_FP8 = 16;

#if defined(__HIPCC__)
// The block-scaled 16x16x128 MFMA (2x the fp16 MFMA rate; the unscaled _fp8_fp8 forms run at the fp16 rate) with e4m3 A
// and B (format 0) and neutral E8M0 scales (127 = 2^0), shared by the fp8 instances of the dense kernels (bf_batch.hip, bf_stream.hip) and
// of the IVF list scan (ivf_scan.hip).  A 128-element K step is the 128 bytes per row a 16-bit K step stages, so the stage
// layout and the two 16-byte fragment reads (k halves ph0 / ph1) stay; the two reads form one 32-byte operand.  Which k a
// register byte stands for does not matter as long as A and B read alike.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
struct MfmaFp8 {
  typedef i32x4 frag;
  static __device__ __forceinline__ f32x4 run2(frag a0, frag a1, frag b0, frag b1, f32x4 c) {
    const i32x8 a = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
    const i32x8 b = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 127, 0, 127);
  }
};
#endif

// The fp8 quantisers and the exact re-rank (bf_fp8.hip), shared by mrag_index_search_fp8 and mrag_ivf_search_fp8; all
// pointers are device pointers.
constexpr int FP8_K = 128;            // elements per fp8 K step (the 128 bytes per row a 16-bit K step stages)
constexpr int FP8_MAX_REFINE = 64;    // candidates per query: the batch kernel's list limit
// rows [0, n) of a 16-bit matrix (pitch ld) -> e4m3fn(clamp(256 x, +-448)) at pitch ld8 bytes, columns >= ld zero
int launch_quant_rows_fp8(const uint16_t* src, int ld, int is_bf16, int64_t n, uint8_t* dst, int ld8, hipStream_t stream);
// prepared query rows [0, n) -> e4m3fn(q * 2^e), max |q * 2^e| in [128, 256) per row; a zero row stays zero
int launch_quant_queries_fp8(const uint16_t* src, int ld, int is_bf16, int64_t n, uint8_t* dst, int ld8, hipStream_t stream);
// per query the fp32 dot products of its 16-bit row with the stored 16-bit rows cand[q][0 .. refine) (-1: none) -> the k
// best, (score desc, row asc), ids = row + id_base, slots past the candidates (-inf, -1)
int launch_fp8_rerank(const uint16_t* rows, const uint16_t* queries, int ld, int is_bf16, const int64_t* cand, int64_t nq, int refine,
                      int k, int64_t id_base, float* out_sc, int64_t* out_id, hipStream_t stream);

// One fused similarity + top-k pass (K2) and the candidate merge (K4) over PREPARED operands
// (storage dtype, padded to `ld`, query buffer padded to a multiple of 256 rows); bf_launch is in bf_index.hip.
struct BfLaunch {
  const uint16_t* corpus = nullptr;   // [rows padded to 256][ld]
  const uint16_t* queries = nullptr;  // dense: [ceil(nq/256)*256][ld]; descriptor mode: gathered [n_wg*256][ld]
  int ld = 0, dtype = MRAG_F16, k = 0;
  int64_t nq = 0;                     // queries reported (rows of out_scores / out_ids)
  int64_t n_rows = 0;                 // dense mode: valid corpus rows
  // descriptor mode (IVF list scan)
  const int* wg_desc = nullptr;       // device int[n_wg][8]
  int n_wg = 0;
  const void* pair_loc = nullptr;     // device int2[nq][nprobe]
  int nprobe = 0;
  const int64_t* row_ids = nullptr;   // device: stored position -> original row
  int64_t id_base = 0;
  float* out_scores = nullptr;        // device [nq][k]
  int64_t* out_ids = nullptr;         // device [nq][k]
  DevBuf* lists = nullptr;            // workspace (grown as needed)
  DevBuf* counts = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev_k2_begin = nullptr, ev_k2_end = nullptr;   // optional
  long long* clock = nullptr;         // optional device long long[4]: batch kernel workgroup 0's clock stamps
  const uint32_t* allow = nullptr;    // dense mode, optional: allow-set bitset over the corpus rows (bit r%32 of word r/32),
                                      // padded with zero words to whole 256-row tiles; runs the filtered (FILT) instances
  bool force_stream = false;          // dense mode, k <= 64: the streaming kernel whatever nq and the corpus size are
  // range search (dense mode, 16-bit operands): the RANGE instances list only rows scoring >= `floor` and count them
  bool range = false;
  float floor = 0.f;                  // finite
  int64_t* out_counts = nullptr;      // device [nq]: rows >= floor per query (NULL: lists only -- the wide-batch redo)
  DevBuf* rslots = nullptr;           // workspace: one count slot per (workgroup, query)
};
int bf_launch(const BfLaunch& a);

// Filtered dense search over prepared operands (bf_filter.hip), shared by mrag_index_search_filtered and the exact path
// of mrag_ivf_search_filtered.
struct FilterWork {
  DevBuf fbits;                       // allow-set bitset over the corpus rows, padded with zero words to whole 256-row tiles
  DevBuf fwork;                       // allowed count (int, word 0) | per-block counts | ascending allowed rows
  DevBuf fcomp;                       // path C: the compacted corpus
  PinnedBuf h_fbits;                  // pinned staging of a host allow-set (pageable copies cost ~25 us per 1M rows)
  Event ev_fbits;                     // recorded after the last copy out of h_fbits (it is rewritten only after it)
  bool counted = false;               // fwork holds the counts of the current allow-set
};
// the allow-set arguments of a filtered search over n rows: allow_rows == n, a known format, a known path of the
// MRAG_FILTER_* / MRAG_IVF_FILTER_* enum (`kind` names it in the message: "filter" / "IVF filter")
int check_allow_args(int64_t allow_rows, int64_t n, int allow_format, int path, const char* kind);
// allow-set (host or device, MRAG_ALLOW_BITS32 / _BYTES) over n rows -> w.fbits.  *m_out = allowed rows when known on
// the host (host allow-set; device allow-set with want_count: one read-back), else -1 (the count is in fwork word 0).
// ev_begin is recorded where the device work of the search starts.
int filter_upload(FilterWork& w, const void* allow, int64_t n, int allow_format, int allow_is_device, bool want_count, int64_t* m_out,
                  hipEvent_t ev_begin, hipStream_t stream);
// AUTO's choice between MRAG_FILTER_MASK and MRAG_FILTER_COMPACT for m allowed rows of n (m >= 0)
int filter_choose_path(int64_t nq, int k, int64_t n, int64_t m, int ld);
// the search restricted to the uploaded allow-set: `a` is the unfiltered dense launch over a.n_rows rows (m > 0 for path C)
int filter_search(FilterWork& w, BfLaunch a, int path, int64_t m, hipStream_t stream);
int bf_max_k();
int bf_max_k_wide();
int64_t bf_round_rows(int64_t n);     // rows rounded up to the kernel's tile (256)
int64_t bf_query_rows(int64_t nq);    // rows of a prepared query buffer: whole 256-query tiles + 16 zero rows
// every slot of sc / ids (n each) -> (-inf, -1): the result of a search with nothing to search
int launch_fill_empty(float* sc, int64_t* ids, int64_t n, hipStream_t stream);

// "Score segments + select" regime of the IVF search (ivf_scan.hip).  One scan workgroup = one descriptor:
//   [0] gq base: slot s of the workgroup scores query row gq[base + s] (< 0: none); or -1 - first for the
//       identity map (queries first .. first + 127)          [1] queries (<= 128)
//   [2] first corpus row            [3] rows to score          [4] index of the first row inside the segment
//   [5],[6] float offset of the workgroup's score block S[slot][pitch] (low, high)        [7] pitch (floats, % 32 == 0)
constexpr int IVFS_DESC_WORDS = 8;
constexpr int IVFS_QUERIES = 128;       // queries per scan workgroup
constexpr int IVFS_CHUNK_ROWS = 128;    // rows of a list one scan descriptor covers = one tile of the scan kernel (longer lists are cut: no single-workgroup tails)
constexpr int IVFS_PITCH_ALIGN = 32;    // floats: every query's score segment starts on a 128-byte line
static inline int64_t ivfs_pitch(int64_t rows) { return (rows + IVFS_PITCH_ALIGN - 1) / IVFS_PITCH_ALIGN * IVFS_PITCH_ALIGN; }
constexpr int IVFS_DENSE_ROWS = 128;    // corpus rows per descriptor of the dense (probe selection) case: one tile, so that the persistent grid balances
// (n_desc_dev != nullptr: the descriptor count lives on the device and n_desc is its host-side upper bound = the grid)
int ivfs_scan(const uint16_t* corpus, const uint16_t* queries, int ld, int dtype, int64_t zero_row, const int* desc, int n_desc,
              const int* n_desc_dev, const int64_t* gq, float* S, hipStream_t stream);
// pinfo: int4 per (query, probe) = (float offset of the pair's score segment: low, high; its rows; its first stored row)
// stored_bits != nullptr: filtered selection, a stored position whose bit is clear is never selected
// range != nullptr: range selection -- only entries scoring >= floor, the entry at stored position excl_pos[q] (-1 or a
// NULL array: none) left out, counts[q] = the entries that remain (all device pointers; not combined with stored_bits)
struct IvfsRange {
  float floor;
  const int64_t* excl_pos;
  int64_t* counts;
};
int ivfs_select_lists(const float* S, const void* pinfo, int nprobe, int64_t nq, int k, const int64_t* row_ids,
                      int64_t id_base, float* out_scores, int64_t* out_ids, hipStream_t stream, const uint32_t* stored_bits = nullptr,
                      const IvfsRange* range = nullptr);
int ivfs_dense_n_desc(int64_t nq, int n_rows);
// count_out != nullptr: every selected row r with row_weight[r] > 0 also bumps count_out[r] (the IVF search's
// "queries per list" histogram, otherwise a kernel of its own)
int ivfs_dense_topk(const uint16_t* corpus, int n_rows, const uint16_t* queries, int64_t nq, int ld, int dtype, int k, int* desc,
                    float* S, float* out_scores, int64_t* out_ids, hipStream_t stream, int* count_out = nullptr,
                    const int* row_weight = nullptr, const uint32_t* row_bits = nullptr);
// (row_bits != nullptr: only rows whose bit is set are selected; missing slots are (-inf, -1))

}  // namespace mrag
