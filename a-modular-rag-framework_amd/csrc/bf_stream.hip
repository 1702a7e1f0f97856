// K2s: the online regime (<= 16 queries per call, e.g. the reference's one question at a time).
// HBM-bound: every corpus byte is read once and the query block rides along, so the structure is
// a pure stream -- 256-row corpus tiles through a 3-stage LDS ring (2 stages = 68 KiB per CU in
// flight behind counted vmcnt), scored on MFMA against the 16 queries, and filtered per query by
// ONE wave per query pair (no atomics): a wave appends the scores that beat the query's running
// k-th best to a 128-entry LDS list, 64 rows at a time, and compacts the list (rank by counting)
// when it passes 64.  Algorithmic bytes per launch = N*D*2 (+ 16*D*2).
//
// Cache policy of the corpus-stream LDS-DMA loads (written into their asm string), measured on one box: every corpus byte
// is read ONCE per launch by ONE workgroup -- nt: 0.270 -> 0.257 ms (5.69 -> 5.98 TB/s at 1 x 1M x 768).  (The batch
// kernel's workgroups share their corpus streams through L2 and keep the default policy: bf_batch.hip.)
#include "bf_kernels.h"

namespace mrag {

constexpr int S_NST = 3;
constexpr int S_STAGE = A_BYTES + SQ * BK * 2;       // 32 KiB corpus + 2 KiB queries
constexpr int S_OFF_SC = S_NST * S_STAGE;            // float [16][260] score tile
constexpr int S_SC_LD = 260;
constexpr int S_OFF_LIST = S_OFF_SC + SQ * S_SC_LD * 4;   // uint2 [queries][LCAP]
// Two instances: QPW = 2 queries per wave (16 per block) with 128-entry lists serves k <= 64;
// QPW = 1 (8 per block) with 512-entry lists serves k <= KMAX_WIDE = 256.
template <int QPW, int LCAP> struct StreamLds {
  static constexpr int NQB = 8 * QPW;                                  // queries per block
  static constexpr int OFF_CNT = S_OFF_LIST + NQB * LCAP * 8;          // int [16]
  static constexpr int OFF_TAU = OFF_CNT + 64;                         // float [16]
  static constexpr int TOTAL = OFF_TAU + 64;
};

// one wave: cut query q's LDS list (<= 64*R entries) to its k best (sorted), raise tau
template <int R>
__device__ __forceinline__ void stream_compact(uint2* __restrict__ lst, int* __restrict__ cnt, float* __restrict__ tau, int q, int k, int lane) {
  const int c = cnt[q];
  uint2 e[R];
  uint64_t key[R];
  int rank[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = r * 64 + lane;
    e[r] = i < c ? lst[i] : make_uint2(0u, 0u);
    key[r] = i < c ? make_key(e[r].x, e[r].y) : 0ull;
    rank[r] = 0;
  }
  for (int j = 0; j < c; ++j) {
    const uint2 o = lst[j];                       // broadcast read
    const uint64_t kj = make_key(o.x, o.y);
#pragma unroll
    for (int r = 0; r < R; ++r) rank[r] += kj > key[r] ? 1 : 0;
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = r * 64 + lane;
    if (i < c && rank[r] < k) {
      lst[rank[r]] = e[r];
      if (rank[r] == k - 1) tau[q] = __uint_as_float(e[r].x);
    }
  }
  if (lane == 0) cnt[q] = min(c, k);
}

// RANGE: tau starts at next_below(p.floor) (only rows >= floor are listed) and the wave filter counts the rows >= floor.
template <int DT, int QPW, int LCAP, bool FILT = false, bool RANGE = false>
__global__ __launch_bounds__(NTHR, 2) void bf_stream_topk_kernel(StreamParams p) {
  typedef typename Mfma<DT>::frag frag;
  typedef StreamLds<QPW, LCAP> L;
  static_assert(LCAP % 64 == 0 && LCAP >= 128, "list capacity: whole 64-entry appends + compaction head room");
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wg = blockIdx.x;
  const int tile_lo = (int)(((long long)wg * p.n_ctiles) / p.S);
  const int tile_hi = (int)(((long long)(wg + 1) * p.n_ctiles) / p.S);
  const int ksteps = p.ksteps, n_tiles = tile_hi - tile_lo;
  float* sc = (float*)(smem + S_OFF_SC);
  uint2* lists = (uint2*)(smem + S_OFF_LIST);
  int* cnt = (int*)(smem + L::OFF_CNT);
  float* tau = (float*)(smem + L::OFF_TAU);
  const float fnb = RANGE ? next_below(p.floor) : -INFINITY;
  if (tid < SQ) { cnt[tid] = 0; tau[tid] = fnb; }
  int rc[QPW];   // RANGE: rows >= floor of this wave's queries (wave-uniform)
#pragma unroll
  for (int qq = 0; qq < QPW; ++qq) rc[qq] = 0;

  const uint32_t row_b = (uint32_t)p.ld * 2u;
  const uint32_t voff_e = (uint32_t)(lane >> 3) * row_b + (uint32_t)(((lane & 7) ^ (lane >> 4)) * 16);
  const uint32_t voff_o = (uint32_t)(lane >> 3) * row_b + (uint32_t)(((lane & 7) ^ (4 + (lane >> 4))) * 16);
  const uint32_t chunk_b = 8u * row_b;
  const size_t tile_bytes = (size_t)TM * p.ld * 2;
  const char* q_ptr = (const char*)p.queries + (size_t)(w & 1) * chunk_b;     // every wave (re)loads query chunk w&1
  const uint32_t voff_q = (w & 1) ? voff_o : voff_e;
  auto stage = [&](const char* a, const char* b, int slot) {
    const uint32_t la = (uint32_t)(slot * S_STAGE + (4 * w) * 1024);
    const uint32_t lb = (uint32_t)(slot * S_STAGE + A_BYTES + (w & 1) * 1024);
    const char *a1 = a + chunk_b, *a2 = a1 + chunk_b, *a3 = a2 + chunk_b;
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %9\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %4 nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %5 nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %6 nt\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %7 nt\n\t"
        "s_mov_b32 m0, %10\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %8\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff_e), "v"(voff_o), "v"(voff_q), "s"(a), "s"(a1), "s"(a2), "s"(a3), "s"(b), "s"(la), "s"(lb)
        : "memory", "scc");
  };
  const int frow = lane & 15, fsw = frow >> 1;
  const int a_rd = (w * 32 + frow) * 128;
  const int b_rd = A_BYTES + frow * 128;
  const int ph0 = ((lane >> 4) ^ fsw) * 16;
  f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};

  const char* a_tile = (const char*)p.corpus + (size_t)tile_lo * tile_bytes + (size_t)(4 * w) * 8 * row_b;
  int pf_kk = 0, pf_left = n_tiles * ksteps, pf_slot = 0, slot = 0;
#pragma unroll 1
  for (int i = 0; i < S_NST - 1; ++i)
    if (pf_left > 0) {
      stage(a_tile + pf_kk * (BK * 2), q_ptr + pf_kk * (BK * 2), pf_slot);
      --pf_left;
      pf_slot = pf_slot == S_NST - 1 ? 0 : pf_slot + 1;
      if (++pf_kk == ksteps) { pf_kk = 0; a_tile += tile_bytes; }
    }
  __syncthreads();
  const int total = n_tiles * ksteps;
  int step = 0;
  for (int ti = 0; ti < n_tiles; ++ti) {
    // FILT: the wave stages rows w*32 .. w*32+31 of the tile = allow-set word tile*8 + w (one scalar load, ahead of the K loop)
    uint32_t allow_w = ~0u;
    if constexpr (FILT) allow_w = *(const __attribute__((address_space(4))) uint32_t*)(p.allow + (size_t)(tile_lo + ti) * (TM / 32) + w);
    for (int kk = 0; kk < ksteps; ++kk, ++step) {
      if (step + 1 < total) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");   // the next stage may stay in flight
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (pf_left > 0) {
        stage(a_tile + pf_kk * (BK * 2), q_ptr + pf_kk * (BK * 2), pf_slot);
        --pf_left;
        pf_slot = pf_slot == S_NST - 1 ? 0 : pf_slot + 1;
        if (++pf_kk == ksteps) { pf_kk = 0; a_tile += tile_bytes; }
      }
      const char* sb = smem + slot * S_STAGE;
      if constexpr (DT == MRAG_DT_FP8) {   // one 16x16x128 MFMA per row block: the two k halves are one 32-byte operand
        const int ph1 = ph0 ^ 64;
        const frag b0 = *(const frag*)(sb + b_rd + ph0), b1 = *(const frag*)(sb + b_rd + ph1);
        const frag a00 = *(const frag*)(sb + a_rd + ph0), a01 = *(const frag*)(sb + a_rd + ph1);
        const frag a10 = *(const frag*)(sb + a_rd + 2048 + ph0), a11 = *(const frag*)(sb + a_rd + 2048 + ph1);
        acc[0] = Mfma<DT>::run2(a00, a01, b0, b1, acc[0]);
        acc[1] = Mfma<DT>::run2(a10, a11, b0, b1, acc[1]);
      } else {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const int ph = ks ? (ph0 ^ 64) : ph0;
          const frag b = *(const frag*)(sb + b_rd + ph);
          const frag a0 = *(const frag*)(sb + a_rd + ph);
          const frag a1 = *(const frag*)(sb + a_rd + 2048 + ph);
          acc[0] = Mfma<DT>::run(a0, b, acc[0]);
          acc[1] = Mfma<DT>::run(a1, b, acc[1]);
        }
      }
      slot = slot == S_NST - 1 ? 0 : slot + 1;
    }
    // ---- tile done: scores -> LDS [query][row], then one wave per query pair filters them -------
    const int tile = tile_lo + ti;
    const int q = lane & 15;
#pragma unroll
    for (int mf = 0; mf < 2; ++mf)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = w * 32 + mf * 16 + (lane >> 4) * 4 + j;
        bool keep = tile * TM + r < p.n_rows;
        if constexpr (FILT) keep = keep && ((allow_w >> (r & 31)) & 1u);
        sc[q * S_SC_LD + r] = keep ? acc[mf][j] : -INFINITY;
      }
    acc[0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    __syncthreads();
#pragma unroll 1
    for (int qq = 0; qq < QPW; ++qq) {
      const int qi = QPW * w + qq;
      if (qi >= p.nq) continue;
      uint2* lst = lists + qi * LCAP;
#pragma unroll 1
      for (int c0 = 0; c0 < TM; c0 += 64) {
        const float v = sc[qi * S_SC_LD + c0 + lane];
        if constexpr (RANGE) {
          const int hits = __popcll(__ballot(v > fnb));
          if (QPW == 1 || qq == 0) rc[0] += hits;
          else rc[QPW - 1] += hits;
        }
        const bool pass = v > tau[qi];                 // strict: a later tie loses to the rows already listed
        const unsigned long long bal = __ballot(pass);
        if (bal) {
          const int base = cnt[qi];
          if (pass) lst[base + __popcll(bal & ((1ull << lane) - 1ull))] = make_uint2(__float_as_uint(v), (uint32_t)(tile * TM + c0 + lane));
          __builtin_amdgcn_wave_barrier();
          if (lane == 0) cnt[qi] = base + __popcll(bal);
          __builtin_amdgcn_wave_barrier();
          if (base + __popcll(bal) > LCAP - 64) stream_compact<LCAP / 64>(lst, cnt, tau, qi, p.k, lane);
        }
      }
    }
    __syncthreads();   // score tile free again
  }
  // ---- end of the split: k best per query (sorted) into the K4 layout ------------------------
  for (int qq = 0; qq < QPW; ++qq) {
    const int qi = QPW * w + qq;
    if constexpr (RANGE) if (lane == 0 && qi < SQ) p.rcounts[(size_t)wg * TQ + qi] = qi < p.nq ? (qq == 0 ? rc[0] : rc[QPW - 1]) : 0;
    if (qi >= p.nq) { if (lane == 0 && qi < SQ) p.counts[(size_t)wg * TQ + qi] = 0; continue; }
    uint2* lst = lists + qi * LCAP;
    stream_compact<LCAP / 64>(lst, cnt, tau, qi, p.k, lane);
    __builtin_amdgcn_wave_barrier();
    const int c = cnt[qi];
    uint2* out = p.list + ((size_t)wg * TQ + qi) * QCAP;
    for (int i = lane; i < c; i += 64) out[i] = lst[i];
    if (lane == 0) p.counts[(size_t)wg * TQ + qi] = c;
  }
}

// K2s instances: [dtype slot][filtered (path M)][range][512-entry lists (k > 32)]; the fp8 row serves the plain search only.
// The 512-entry-list instance also wins for 32 < k <= 64: with 128-entry lists a list of k = 64 is compacted after every
// 64-row chunk (1 x 1M x 768: 0.431 ms at k = 64 against 0.332 ms at k = 100 on the wide instance)
int launch_k2s(int dtype, bool filt, bool range, bool wide, hipStream_t stream, const StreamParams& p) {
  typedef void (*K2sFn)(StreamParams);
  static const K2sFn fns[3][2][2][2] = {
      {{{bf_stream_topk_kernel<MRAG_F16, 2, 128>, bf_stream_topk_kernel<MRAG_F16, 1, 512>},
        {bf_stream_topk_kernel<MRAG_F16, 2, 128, false, true>, bf_stream_topk_kernel<MRAG_F16, 1, 512, false, true>}},
       {{bf_stream_topk_kernel<MRAG_F16, 2, 128, true>, bf_stream_topk_kernel<MRAG_F16, 1, 512, true>},
        {bf_stream_topk_kernel<MRAG_F16, 2, 128, true, true>, bf_stream_topk_kernel<MRAG_F16, 1, 512, true, true>}}},
      {{{bf_stream_topk_kernel<MRAG_BF16, 2, 128>, bf_stream_topk_kernel<MRAG_BF16, 1, 512>},
        {bf_stream_topk_kernel<MRAG_BF16, 2, 128, false, true>, bf_stream_topk_kernel<MRAG_BF16, 1, 512, false, true>}},
       {{bf_stream_topk_kernel<MRAG_BF16, 2, 128, true>, bf_stream_topk_kernel<MRAG_BF16, 1, 512, true>},
        {bf_stream_topk_kernel<MRAG_BF16, 2, 128, true, true>, bf_stream_topk_kernel<MRAG_BF16, 1, 512, true, true>}}},
      {{{bf_stream_topk_kernel<MRAG_DT_FP8, 2, 128>, bf_stream_topk_kernel<MRAG_DT_FP8, 1, 512>}, {nullptr, nullptr}},
       {{nullptr, nullptr}, {nullptr, nullptr}}}};
  static const int slds[2] = {StreamLds<2, 128>::TOTAL, StreamLds<1, 512>::TOTAL};
  const int di = dtype == MRAG_F16 ? 0 : (dtype == MRAG_BF16 ? 1 : 2);
  if (range && di > 1) return fail(MRAG_ERR_UNSUPPORTED, "range search serves the dense 16-bit index only");
  const K2sFn fn = fns[di][filt][range][wide];
  if (!fn) return fail(MRAG_ERR_UNSUPPORTED, "the fp8 scan serves the plain dense search only");
  MRAG_TRY(set_max_lds((const void*)fn, slds[wide]));
  hipLaunchKernelGGL(fn, dim3((unsigned)p.S), dim3(NTHR), slds[wide], stream, p);
  MRAG_HIP(hipGetLastError());
  return MRAG_OK;
}

}  // namespace mrag
