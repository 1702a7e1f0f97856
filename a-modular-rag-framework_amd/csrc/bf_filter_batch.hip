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
// Selection is ivfs_select_lists with nprobe = 1 (the caller, bf_index.hip).
#include "bf_kernels.h"

namespace mrag {

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

int launch_sets_scan(const uint16_t* corpus, const uint16_t* queries, const uint16_t* zero, int ld, int dtype, const int* desc,
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

}  // namespace mrag
