// Dense search with one allow-set of rows per question (mrag_index_search_sets): the gathered-set scan.
//
// A "set" is what an IVF list is to ivfs_scan_kernel (ivf_scan.hip): a group of rows scored against the few questions
// that point at it.  The difference is where the rows are: a list is contiguous, the rows of a set are scattered over
// the corpus.  So this kernel is the list scan with BOTH operands fetched by per-lane source addresses:
//
//   sets_scan_kernel   one workgroup walks descriptors; one descriptor = one chunk of <= 128 rows of one set x <= 128 of
//                      the questions that use the set, as one 128 x 128 x 64 MFMA tile per K step, fed by LDS-DMA into
//                      two 32-KiB stages.  Corpus row r of the chunk comes from corpus[set_rows[pos0 + r]], question
//                      slot s from queries[qlist[q0 + s]] (qlist = the questions sorted by set); rows and slots past the
//                      end of the chunk read a zero row.  No gathered copy of either operand is written to HBM.
//                      Scores leave as fp32 segments, one per question, of pitch ivfs_pitch(m_set) floats: every segment
//                      starts on a 128-byte line and is written with 16-byte stores (4 consecutive rows of one question
//                      per lane).
//
// The corpus is the MFMA A operand, Mfma<DT> is the instruction of K2 and of the list scan (SMfma there), and a score is
// accumulated over K ascending from a zero accumulator: one (row, question) score does not depend on which other rows or
// questions share its tile, and equals what those kernels compute for the pair.
// Selection is ivfs_select_lists with nprobe = 1 (sets_scan_route below).  Behind the kernel: the host plan of the scan
// route, the two routes and the entry points.
#include "bf_index.h"

namespace mrag {

// One descriptor = one chunk of <= SETS_CHUNK rows of one set x <= SETS_CHUNK of the questions that use it:
//   [0] first slot in qlist (the questions sorted by set)     [1] questions (<= 128)
//   [2] first position in set_rows                            [3] rows (<= 128)      [4] index of the first row inside the set
//   [5],[6] float offset of the first question's score segment (low, high)           [7] segment pitch (floats, % 32 == 0)
// Slot s of the descriptor writes S[offset + s * pitch + [4] ...]: the questions of a set hold consecutive segments.
constexpr int SETS_DESC_WORDS = 8;
constexpr int SETS_CHUNK = 128;

constexpr int FT = 128, FK = 64, FTHR = 256;
constexpr int F_A_BYTES = FT * FK * 2;          // 16 KiB: corpus rows of a stage
constexpr int F_STAGE = 2 * F_A_BYTES;          // 32 KiB
static_assert(FT == SETS_CHUNK, "one descriptor is one tile");

template <int DT>
__global__ __launch_bounds__(FTHR) void sets_scan_kernel(const uint16_t* __restrict__ corpus, const uint16_t* __restrict__ queries,
                                                         const uint16_t* __restrict__ zero, int ld, const int* __restrict__ desc,
                                                         int n_desc, const int64_t* __restrict__ set_rows,
                                                         const int* __restrict__ qlist, float* __restrict__ S) {
  typedef typename Mfma<DT>::frag frag;
  __shared__ __attribute__((aligned(16))) char sm[2 * F_STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1;
  // blocks go to XCDs round-robin: each XCD gets a contiguous run of descriptors (the chunks of one set and the question
  // groups of one chunk are neighbours, so a set's rows are fetched into ONE L2)
  const int per = (n_desc + 7) >> 3;
  const int nk = ld / FK;
  for (int it = (int)(blockIdx.x >> 3); it < per; it += (int)(gridDim.x >> 3)) {
    const int lin = (int)(blockIdx.x & 7) * per + it;
    if (lin >= n_desc) break;
    __syncthreads();                                         // every wave is done with the previous descriptor's LDS stages
    const int* d = desc + (size_t)lin * SETS_DESC_WORDS;
    const int q0 = d[0], nq_local = d[1], pos0 = d[2], n_rows = d[3], r_off = d[4], pitch = d[7];
    const int64_t soff = (int64_t)(uint32_t)d[5] | ((int64_t)d[6] << 32);

    // per-lane LDS-DMA sources: wave w fills 1-KiB chunks 4w..4w+3 of each operand (8 rows x 128 B per chunk), the 16-byte
    // piece a lane fetches is XOR-swizzled by its row so that the fragment reads are conflict-free
    int64_t rid[4];
    int qid[4];                                              // all eight index loads in flight together
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (4 * w + i) * 8 + (lane >> 3);
      rid[i] = r < n_rows ? set_rows[(size_t)pos0 + r] : -1;
      qid[i] = r < nq_local ? qlist[(size_t)q0 + r] : -1;
    }
    const uint16_t* a_src[4];
    const uint16_t* b_src[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = (4 * w + i) * 8 + (lane >> 3);
      const int kc = (lane & 7) ^ ((r >> 1) & 7);
      a_src[i] = (rid[i] >= 0 ? corpus + (size_t)rid[i] * ld : zero) + kc * 8;
      b_src[i] = (qid[i] >= 0 ? queries + (size_t)qid[i] * ld : zero) + kc * 8;
    }
    // the loads of K step kk: only the 1-KiB chunks (8 rows) that hold rows of the set / questions of the group (the rest of
    // the stage keeps whatever it held: those rows' scores are never stored)
    auto stage = [&](int kk, int buf) {
      char* la = sm + buf * F_STAGE + (4 * w) * 1024;
      char* lb = la + F_A_BYTES;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if ((4 * w + i) * 8 < n_rows)
          __builtin_amdgcn_global_load_lds((glb_vptr)(a_src[i] + kk * FK), (lds_vptr)(la + i * 1024), 16, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if ((4 * w + i) * 8 < nq_local)
          __builtin_amdgcn_global_load_lds((glb_vptr)(b_src[i] + kk * FK), (lds_vptr)(lb + i * 1024), 16, 0, 0);
    };
    const int frow = lane & 15, fsw = frow >> 1;
    const int a_rd = (wm * 64 + frow) * 128, b_rd = F_A_BYTES + (wn * 64 + frow) * 128;
    const int ph0 = ((lane >> 4) ^ fsw) * 16;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // this wave's 64 x 64 piece: only the 16-row / 16-question fragments that hold real rows / questions (wave-uniform)
    const int ni = min(4, (n_rows - wm * 64 + 15) >> 4);
    const int nj = min(4, (nq_local - wn * 64 + 15) >> 4);
    stage(0, 0);
    for (int kk = 0; kk < nk; ++kk) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of stage kk have landed
      __builtin_amdgcn_s_barrier();                      // everyone's pieces are in LDS; everyone is done with the buffer restaged below
      asm volatile("" ::: "memory");
      if (kk + 1 < nk) stage(kk + 1, (kk + 1) & 1);
      const char* sb = sm + (kk & 1) * F_STAGE;
      if (ni > 0 && nj > 0) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const int ph = ks ? (ph0 ^ 64) : ph0;
          frag af[4], bf[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) if (i < ni) af[i] = *(const frag*)(sb + a_rd + i * 2048 + ph);
#pragma unroll
          for (int j = 0; j < 4; ++j) if (j < nj) bf[j] = *(const frag*)(sb + b_rd + j * 2048 + ph);
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (i < ni && j < nj) acc[i][j] = Mfma<DT>::run(af[i], bf[j], acc[i][j]);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's fragment reads are done before it reaches the next barrier
    }
    // scores: a lane holds rows r0..r0+3 (consecutive) of question slot q per accumulator.  Rows up to the next multiple of
    // 4 are written (zero-row scores); the segment's pitch covers them.
    float* Sb = S + soff;
    const int rl = wm * 64 + (lane >> 4) * 4;
    const int rows4 = (n_rows + 3) & ~3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int q = wn * 64 + j * 16 + (lane & 15);
      if (q >= nq_local) continue;
      float* sq = Sb + (size_t)q * pitch + r_off;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r0 = rl + i * 16;
        if (r0 < rows4) *(f32x4*)(sq + r0) = acc[i][j];
      }
    }
  }
}

// scores of every descriptor's (row, question) pairs -> S; all pointers are device pointers, `zero` is a row of ld zeros
static int launch_sets_scan(const uint16_t* corpus, const uint16_t* queries, const uint16_t* zero, int ld, int dtype, const int* desc,
                     int n_desc, const int64_t* set_rows, const int* qlist, float* S, hipStream_t stream) {
  if (n_desc <= 0) return MRAG_OK;
  if (ld % FK) return fail(MRAG_ERR_INVALID, "sets scan: ld %d is not a multiple of %d", ld, FK);
  if (dtype != MRAG_F16 && dtype != MRAG_BF16) return fail(MRAG_ERR_UNSUPPORTED, "sets scan: storage dtype %d", dtype);
  static int cus = 0;
  if (!cus) { hipDeviceProp_t pr; int dev = 0; cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256; }
  // persistent grid: two workgroups per CU (whole XCD rounds), never more than the descriptors need
  const unsigned grid = (unsigned)std::max<int64_t>(8, std::min<int64_t>((int64_t)(n_desc + 7) / 8 * 8, (int64_t)cus * 2 / 8 * 8));
  if (dtype == MRAG_F16) hipLaunchKernelGGL((sets_scan_kernel<MRAG_F16>), dim3(grid), dim3(FTHR), 0, stream, corpus, queries, zero, ld, desc, n_desc, set_rows, qlist, S);
  else hipLaunchKernelGGL((sets_scan_kernel<MRAG_BF16>), dim3(grid), dim3(FTHR), 0, stream, corpus, queries, zero, ld, desc, n_desc, set_rows, qlist, S);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

// ---- mrag_index_search_sets: the host plan of the scan route ----
// Score scratch of one scan + select pair.  A call whose segments need more is cut into chunks of whole questions.
// Nobody has measured this limit: 1 GiB holds 32 768 segments of the largest scanned set and keeps the scratch a small
// part of the device's memory; a smaller scratch that stays in L2 between the scan and the select may well be faster.
constexpr int64_t SETS_SCRATCH_FLOATS = (int64_t)1 << 28;

struct SetsChunk {
  int64_t q0, nq;          // sorted scan questions [q0, q0 + nq)
  int64_t d0, nd;          // its descriptors
};
struct SetsPlan {
  std::vector<int> qlist;               // scan questions, sorted by set (stable): original question index
  std::vector<int> desc;                // SETS_DESC_WORDS ints per descriptor, chunk after chunk
  std::vector<int> pinfo;               // int4 per sorted scan question: segment offset (low, high), rows, first position
  std::vector<SetsChunk> chunks;
  std::vector<int64_t> rows;            // the scanned sets' rows when some set is routed (else the caller's set_rows serve)
  std::vector<int64_t> routed;          // sets above SETS_SCAN_MAX_ROWS that some question uses
  std::vector<int64_t> order, qstart;   // all questions sorted by set (stable); set s owns order[qstart[s] .. qstart[s+1])
  int64_t n_rows = 0, max_floats = 0;   // positions the scan may read; floats of the largest chunk
};

// (arguments validated by the caller)
static int sets_plan(int64_t nq, int64_t n_sets, const int64_t* set_ptr, const int64_t* set_rows, const int32_t* set_of, SetsPlan& p) {
  p.qstart.assign((size_t)n_sets + 1, 0);
  for (int64_t q = 0; q < nq; ++q) ++p.qstart[(size_t)set_of[q] + 1];
  for (int64_t s = 0; s < n_sets; ++s) p.qstart[(size_t)s + 1] += p.qstart[(size_t)s];
  p.order.resize((size_t)nq);
  {
    std::vector<int64_t> at(p.qstart.begin(), p.qstart.end() - 1);
    for (int64_t q = 0; q < nq; ++q) p.order[(size_t)at[(size_t)set_of[q]]++] = q;
  }
  for (int64_t s = 0; s < n_sets; ++s)
    if (p.qstart[(size_t)s + 1] > p.qstart[(size_t)s] && set_ptr[s + 1] - set_ptr[s] > SETS_SCAN_MAX_ROWS) p.routed.push_back(s);
  const bool compact = !p.routed.empty();
  int64_t floats = 0;                     // of the open chunk
  SetsChunk c{0, 0, 0, 0};
  const auto close = [&]() {
    if (c.nq) { p.chunks.push_back(c); p.max_floats = std::max(p.max_floats, floats); }
    c = SetsChunk{c.q0 + c.nq, 0, c.d0 + c.nd, 0};
    floats = 0;
  };
  for (int64_t s = 0; s < n_sets; ++s) {
    const int64_t m = set_ptr[s + 1] - set_ptr[s];
    int64_t g0 = p.qstart[(size_t)s];
    const int64_t g1 = p.qstart[(size_t)s + 1];
    if (g1 == g0 || m > SETS_SCAN_MAX_ROWS) continue;
    int64_t pos = set_ptr[s];
    if (compact) {
      pos = (int64_t)p.rows.size();
      p.rows.insert(p.rows.end(), set_rows + set_ptr[s], set_rows + set_ptr[s + 1]);
    }
    if (pos + m > 0x7FFFFFFFll) return fail(MRAG_ERR_UNSUPPORTED, "set %lld ends at position %lld of set_rows: one call scans at most 2^31 - 1 positions", (long long)s, (long long)(pos + m));
    p.n_rows = std::max(p.n_rows, pos + m);
    const int64_t pitch = ivfs_pitch(m);
    while (g0 < g1) {
      // the questions of the set that still fit the open chunk (an empty set's questions take no scratch)
      int64_t fit = pitch ? (SETS_SCRATCH_FLOATS - floats) / pitch : g1 - g0;
      if (fit <= 0) { close(); continue; }
      fit = std::min(fit, g1 - g0);
      for (int64_t r0 = 0; r0 < m; r0 += SETS_CHUNK)
        for (int64_t q0 = 0; q0 < fit; q0 += SETS_CHUNK) {
          const int64_t soff = floats + q0 * pitch;
          const int d[SETS_DESC_WORDS] = {(int)(c.q0 + c.nq + q0), (int)std::min<int64_t>(SETS_CHUNK, fit - q0), (int)(pos + r0),
                                          (int)std::min<int64_t>(SETS_CHUNK, m - r0), (int)r0, (int)(uint32_t)(soff & 0xFFFFFFFFll),
                                          (int)(soff >> 32), (int)pitch};
          p.desc.insert(p.desc.end(), d, d + SETS_DESC_WORDS);
          ++c.nd;
        }
      for (int64_t g = 0; g < fit; ++g) {
        const int64_t soff = floats + g * pitch;
        const int pi[4] = {(int)(uint32_t)(soff & 0xFFFFFFFFll), (int)(soff >> 32), (int)m, (int)pos};
        p.pinfo.insert(p.pinfo.end(), pi, pi + 4);
        p.qlist.push_back((int)p.order[(size_t)(g0 + g)]);
      }
      floats += fit * pitch;
      c.nq += fit;
      g0 += fit;
    }
  }
  close();
  return MRAG_OK;
}

// the arguments of a call over nq > 0 questions, behind nq, k and n_sets
static int sets_check_args(const BfIndex* ix, const void* queries, int64_t nq, int q_dtype, int64_t n_sets, const int64_t* set_ptr,
                           const int64_t* set_rows, const int32_t* set_of, const float* out_scores, const int64_t* out_ids, size_t* esz) {
  MRAG_TRY(check_query_args(!queries || !set_ptr || !set_of || !out_scores || !out_ids, q_dtype, nq, "questions", esz));
  if (n_sets > 0) MRAG_TRY(check_csr(set_ptr, n_sets, "set_ptr", "set"));
  if (n_sets > 0 && set_ptr[n_sets] > 0 && !set_rows) return fail(MRAG_ERR_INVALID, "NULL buffer (set_rows)");
  for (int64_t s = 0; s < n_sets; ++s)
    for (int64_t i = set_ptr[s]; i < set_ptr[s + 1]; ++i) {
      const int64_t r = set_rows[i];
      if (r < 0 || r >= ix->n)
        return fail(MRAG_ERR_INVALID, "set %lld: row %lld outside [0, %lld)", (long long)s, (long long)r, (long long)ix->n);
      if (i > set_ptr[s] && r <= set_rows[i - 1])
        return fail(MRAG_ERR_INVALID, "set %lld: rows are not strictly ascending (%lld after %lld)", (long long)s, (long long)r,
                    (long long)set_rows[i - 1]);
    }
  for (int64_t q = 0; q < nq; ++q)
    if (set_of[q] < 0 || set_of[q] >= n_sets)
      return fail(MRAG_ERR_INVALID, "question %lld: set %d outside [0, %lld)", (long long)q, (int)set_of[q], (long long)n_sets);
  return MRAG_OK;
}

// The questions one sets search serves, as both routes see them (host buffers)
struct SetsCall {
  const void* queries;
  int64_t nq;
  int q_dtype, normalize, k;
  size_t row_bytes;          // of one question's vector
  float* out_scores;         // [nq][k]
  int64_t* out_ids;
  hipStream_t stream;
};

// ---- scan route: every question of a set of <= SETS_SCAN_MAX_ROWS rows
static int sets_scan_route(BfIndex* ix, const SetsCall& c, const SetsPlan& p, const int64_t* set_rows) {
  SetsState& w = ix->sets;
  const int64_t nq = c.nq, n_scan = (int64_t)p.qlist.size();
  const int ld = ix->ld, k = c.k;
  hipStream_t stream = c.stream;
  ix->timed = false;                                       // (the events of the last plain search bracket none of this)
  const int64_t* rows_src = p.routed.empty() ? set_rows : p.rows.data();
  // plan: [descriptors | question list | segment table], one upload
  const size_t db = (size_t)round_up((int64_t)(p.desc.size() * 4), 256), lb = (size_t)round_up(n_scan * 4, 256), pb = (size_t)n_scan * 16;
  std::vector<char> plan(db + lb + pb);
  if (!p.desc.empty()) memcpy(plan.data(), p.desc.data(), p.desc.size() * 4);
  memcpy(plan.data() + db, p.qlist.data(), (size_t)n_scan * 4);
  memcpy(plan.data() + db + lb, p.pinfo.data(), pb);
  std::vector<float> h_sc((size_t)n_scan * k);
  std::vector<int64_t> h_id((size_t)n_scan * k);
  MRAG_TRY(ix->stage_in.ensure((size_t)nq * c.row_bytes));
  MRAG_TRY(w.q.ensure((size_t)(nq + 1) * ld * 2));
  MRAG_TRY(w.plan.ensure(plan.size()));
  MRAG_TRY(w.rows.ensure((size_t)std::max<int64_t>(p.n_rows, 1) * 8));
  MRAG_TRY(w.S.ensure((size_t)std::max<int64_t>(p.max_floats, 32) * 4));
  MRAG_TRY(ix->out_sc.ensure((size_t)n_scan * k * 4));
  MRAG_TRY(ix->out_id.ensure((size_t)n_scan * k * 8));
  uint16_t* d_q = (uint16_t*)w.q.p;
  const uint16_t* d_zero = d_q + (size_t)nq * ld;
  const char* d_plan = (const char*)w.plan.p;
  float* d_sc = (float*)ix->out_sc.p;
  int64_t* d_id = (int64_t*)ix->out_id.p;
  // (the uploads read `plan`, `p` and the caller's buffers asynchronously)
  MRAG_TRY(run_synced(stream, [&]() -> int {
    MRAG_HIP(hipMemcpyAsync(ix->stage_in.p, c.queries, (size_t)nq * c.row_bytes, hipMemcpyHostToDevice, stream));
    MRAG_HIP(hipMemcpyAsync(w.plan.p, plan.data(), plan.size(), hipMemcpyHostToDevice, stream));
    if (p.n_rows) MRAG_HIP(hipMemcpyAsync(w.rows.p, rows_src, (size_t)p.n_rows * 8, hipMemcpyHostToDevice, stream));
    MRAG_HIP(hipMemsetAsync((void*)d_zero, 0, (size_t)ld * 2, stream));
    MRAG_TRY(launch_prep_rows(ix->stage_in.p, c.q_dtype, nq, ix->dim, d_q, ld, ix->dtype, c.normalize && ix->metric == MRAG_METRIC_COSINE, stream));
    for (const SetsChunk& ch : p.chunks) {
      MRAG_TRY(launch_sets_scan(ix->rows, d_q, d_zero, ld, ix->dtype, (const int*)d_plan + (size_t)ch.d0 * SETS_DESC_WORDS, (int)ch.nd,
                                (const int64_t*)w.rows.p, (const int*)(d_plan + db), (float*)w.S.p, stream));
      MRAG_TRY(ivfs_select_lists((const float*)w.S.p, d_plan + db + lb + (size_t)ch.q0 * 16, 1, ch.nq, k, (const int64_t*)w.rows.p,
                                 ix->id_base, d_sc + (size_t)ch.q0 * k, d_id + (size_t)ch.q0 * k, stream));
    }
    MRAG_HIP(hipMemcpyAsync(h_sc.data(), d_sc, h_sc.size() * 4, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipMemcpyAsync(h_id.data(), d_id, h_id.size() * 8, hipMemcpyDeviceToHost, stream));
    return MRAG_OK;
  }));
  scatter_rows(p.qlist.data(), n_scan, k, h_sc.data(), h_id.data(), c.out_scores, c.out_ids);
  return MRAG_OK;
}

// ---- routed: a larger set is ONE filtered search over all of its questions (in groups where the batch limits k)
static int sets_routed_route(BfIndex* ix, const SetsCall& c, const SetsPlan& p, const int64_t* set_ptr, const int64_t* set_rows,
                             int64_t* n_routed) {
  const int k = c.k;
  for (const int64_t s : p.routed) {
    const int64_t g0 = p.qstart[(size_t)s], n_q = p.qstart[(size_t)s + 1] - g0;
    std::vector<uint32_t> bits((size_t)((ix->n + 31) / 32), 0u);
    for (int64_t i = set_ptr[s]; i < set_ptr[s + 1]; ++i) bits[(size_t)(set_rows[i] >> 5)] |= 1u << (set_rows[i] & 31);
    int64_t group = n_q;
    for (;;) {
      int kmax = 0;
      MRAG_TRY(mrag_index_max_k(group, &kmax));
      if (kmax >= k || group == 1) break;
      group = (group + 1) / 2;
    }
    std::vector<char> hq((size_t)group * c.row_bytes);
    std::vector<float> h_sc((size_t)group * k);
    std::vector<int64_t> h_id((size_t)group * k);
    for (int64_t j0 = 0; j0 < n_q; j0 += group) {
      const int64_t n_g = std::min(group, n_q - j0);
      const int64_t* order = p.order.data() + g0 + j0;
      for (int64_t j = 0; j < n_g; ++j)
        memcpy(hq.data() + (size_t)j * c.row_bytes, (const char*)c.queries + (size_t)order[j] * c.row_bytes, c.row_bytes);
      MRAG_TRY(search_allowed(ix, hq.data(), n_g, c.q_dtype, c.normalize, 0, k, nullptr, bits.data(), ix->n, MRAG_ALLOW_BITS32, 0,
                              MRAG_FILTER_AUTO, h_sc.data(), h_id.data(), nullptr, 0, c.stream));
      scatter_rows(order, n_g, k, h_sc.data(), h_id.data(), c.out_scores, c.out_ids);
    }
    *n_routed += n_q;
  }
  return MRAG_OK;
}

}  // namespace mrag

using namespace mrag;

extern "C" {

int mrag_index_search_sets(mrag_handle h, const void* queries, int64_t nq, int q_dtype, int normalize, int k, int64_t n_sets,
                           const int64_t* set_ptr, const int64_t* set_rows, const int32_t* set_of, float* out_scores,
                           int64_t* out_ids, void* stream_) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  MRAG_TRY(check_nq_k(nq, k));
  if (n_sets < 0) return fail(MRAG_ERR_INVALID, "n_sets < 0");
  if (nq == 0) return MRAG_OK;
  size_t esz = 0;
  MRAG_TRY(sets_check_args(ix, queries, nq, q_dtype, n_sets, set_ptr, set_rows, set_of, out_scores, out_ids, &esz));
  SetsPlan p;
  MRAG_TRY(sets_plan(nq, n_sets, set_ptr, set_rows, set_of, p));
  MRAG_TRY(use_device(ix->device));
  ix->sets.last.open();
  const SetsCall c{queries, nq, q_dtype, normalize, k, (size_t)ix->dim * esz, out_scores, out_ids, (hipStream_t)stream_};
  const int64_t n_scan = (int64_t)p.qlist.size();
  int64_t n_routed = 0;
  if (n_scan) MRAG_TRY(sets_scan_route(ix, c, p, set_rows));
  MRAG_TRY(sets_routed_route(ix, c, p, set_ptr, set_rows, &n_routed));
  ix->sets.last.close(n_scan, n_routed, (int64_t)(p.desc.size() / SETS_DESC_WORDS));
  return MRAG_OK;
}

int mrag_index_last_sets(mrag_handle h, int64_t* out_scanned_questions, int64_t* out_routed_questions, int64_t* out_descriptors) {
  BfIndex* ix = (BfIndex*)lookup(h, KIND_BF_INDEX);
  if (!ix) return MRAG_ERR_INVALID;
  return ix->sets.last.read("search over per-question sets", out_scanned_questions, out_routed_questions, out_descriptors);
}

}  // extern "C"
