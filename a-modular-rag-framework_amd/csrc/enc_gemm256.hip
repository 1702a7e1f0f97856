// K6, the encoder's large-batch GEMM: enc_gemm256_kernel<DT, EPI, LNF>, persistent 256 x 256 x 64 tiles (the K2 main loop),
// epilogue bias | bias + erf-GELU | bias + residual, optionally with a LayerNorm folded in on either side (LNF, LnArgs in
// enc_kernels.h).  launch_gemm256 is its only launcher: it picks among the fourteen instances the two flows of encoder.hip
// use, sets the kernel's dynamic-LDS limit the first time an instance runs and sizes the persistent grid.
#include "enc_kernels.h"

namespace mrag {

// ------------------------------------------------------------------ 256 x 256 persistent GEMM (the K2 main loop)
// Used when N_pad % 256 == 0 and M_pad % 256 == 0.  Same structure as the similarity kernel of
// bf_batch.hip: 8 waves (2 x 4), 256 x 256 x 64 stages through LDS-DMA issued from inline asm (scalar
// base + 32-bit voffset, XOR swizzle on the source address), two fragment register sets so that the
// MFMA pipe never waits on a read it has just issued, zero C operand on the first K step of a tile,
// one barrier per K step.  Workgroups are persistent: each walks tiles lin = first, first + stride, ...
// and prefetches the first stage of its next tile during the last K step of the current one.
// The WEIGHT rows are the MFMA A operand and the token rows the B operand, so a lane's four accumulator
// values are four consecutive OUTPUT columns of one token: bias / GELU / residual apply to 8-byte
// groups and the stores are 8 bytes per lane (the 128 x 128 kernel above stores 2 bytes at a time).
constexpr int G2_THR = 512;
constexpr int G2_A_BYTES = G2_T * GK * 2;            // 32 KiB: weight rows of a stage
constexpr int G2_STAGE = 2 * G2_A_BYTES;             // 64 KiB
constexpr int G2_PAD = 4096;                          // between the two stage buffers: either buffer + the pad holds the
constexpr int G2_BUF1 = G2_STAGE + G2_PAD;            // epilogue's 128 x 528-byte output slab
constexpr int G2_VEC = 2048;                          // behind the stage buffers: bias / gamma of the tile's 256 columns (LNR epilogue)
constexpr int G2_CPITCH = 528;                        // output row pitch in LDS: 256 columns x 2 B + 16 (bank shift per row)
// Wave roles: waves 0-3 (one per SIMD) issue every LDS-DMA of the K loop, waves 4-7 every global store of the epilogue.
// vmcnt counts a wave's loads and stores in issue order, so a wave that does both sits out its output stores (128 KiB per
// CU, all CUs at once: the HBM write rate) at the next stage wait; with the roles split the loading waves never have a
// store outstanding and the storing waves never wait on vmcnt inside the K loop.
constexpr int G2_CPW = 8;                             // 1-KiB chunks of each operand stage a loading wave fills
constexpr int G2_PS = 2048;                           // the loading waves' LayerNorm partial sums pass through LDS to the storing waves
constexpr int G2_LDS = 2 * G2_STAGE + G2_PAD + G2_VEC + G2_PS;   // 134 KiB

template <int DT, int EPI, int LNF>
__global__ __launch_bounds__(G2_THR, 2) void enc_gemm256_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ W,
                                                                const float* __restrict__ bias, const uint16_t* __restrict__ R,
                                                                uint16_t* __restrict__ C, int N, int K, int tiles_m, int tiles_n,
                                                                LnArgs ln) {
  typedef typename EMfma<DT>::frag frag;
  typedef typename EMfma<DT>::elem elem;
  typedef elem e4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) char sm2[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 2, wn = w & 3;     // wave tile: 128 weight rows (output columns) x 64 tokens
  const int ksteps = K / GK;
  const int n_tiles = tiles_m * tiles_n;
  // XCD-aware start: the workgroups of one XCD (blockIdx % 8) take consecutive tiles, which walk N first
  // and share the token panel in that XCD's L2
  const int nwg = gridDim.x;
  const int first = (nwg % 8 == 0) ? (int)(blockIdx.x & 7) * (nwg / 8) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  const uint32_t row_b = (uint32_t)K * 2u;
  const uint32_t voff_e = (uint32_t)(lane >> 3) * row_b + (uint32_t)(((lane & 7) ^ (lane >> 4)) * 16);
  const uint32_t voff_o = (uint32_t)(lane >> 3) * row_b + (uint32_t)(((lane & 7) ^ (4 + (lane >> 4))) * 16);
  const uint32_t chunk_b = 8u * row_b;
  const bool loader = w < 4;                             // (wave-uniform)
  const bool storer = w >= 4;
  const size_t wave_off = (size_t)(G2_CPW * (w & 3)) * chunk_b;     // loading wave w fills 1-KiB chunks 8w..8w+7 of each operand
  auto tile_ptrs = [&](int lin, const char*& a, const char*& b) {
    const int tm = lin / tiles_n, tn = lin - tm * tiles_n;
    a = (const char*)(W + (size_t)tn * G2_T * K) + wave_off;
    b = (const char*)(X + (size_t)tm * G2_T * K) + wave_off;
  };
  auto stage = [&](const char* a, const char* b, int buf) {
    if (!loader) return;
#pragma unroll
    for (int op = 0; op < 2; ++op) {
      const char* base = op ? b : a;
#pragma unroll
      for (int i = 0; i < G2_CPW; i += 2) {
        const uint32_t la = (uint32_t)(buf * G2_BUF1 + op * G2_A_BYTES + (G2_CPW * (w & 3) + i) * 1024);
        const char* c0 = base + (size_t)i * chunk_b;
        const char* c1 = c0 + chunk_b;
        uint32_t keep;
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\t"
            "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %4\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(voff_e), "v"(voff_o), "s"(c0), "s"(c1), "s"(la)
            : "memory", "scc");
      }
    }
  };
  const int frow = lane & 15, fsw = frow >> 1;
  const int a_rd = (wm * 128 + frow) * 128;
  const int b_rd = G2_A_BYTES + (wn * 64 + frow) * 128;
  const int ph0 = ((lane >> 4) ^ fsw) * 16;
  f32x4 acc[8][4];
  frag f1a[8], f1b[4];

  // prefetch cursor over the flattened (tile, k step) sequence of this workgroup
  int pf_lin = first, pf_kk = 0;
  const char *pf_a = nullptr, *pf_b = nullptr;
  if (pf_lin < n_tiles) tile_ptrs(pf_lin, pf_a, pf_b);
  int buf = 0;
  auto prefetch = [&](int into) {
    if (pf_lin >= n_tiles) return;
    stage(pf_a + pf_kk * (GK * 2), pf_b + pf_kk * (GK * 2), into);
    if (++pf_kk == ksteps) {
      pf_kk = 0;
      pf_lin += nwg;
      if (pf_lin < n_tiles) tile_ptrs(pf_lin, pf_a, pf_b);
    }
  };
  prefetch(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  auto kstep = [&](auto pending_tag) {
    constexpr bool PENDING = decltype(pending_tag)::value;
    prefetch(buf ^ 1);
    const char* sb = sm2 + buf * G2_BUF1;
    buf ^= 1;
    const int ph1 = ph0 ^ 64;
    frag f0a[8], f0b[4];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) f0b[nf] = *(const frag*)(sb + b_rd + nf * 2048 + ph0);
#pragma unroll
    for (int mf = 0; mf < 8; ++mf) f0a[mf] = *(const frag*)(sb + a_rd + mf * 2048 + ph0);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (PENDING) {
#pragma unroll
      for (int mf = 0; mf < 8; ++mf)
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) acc[mf][nf] = EMfma<DT>::run(f1a[mf], f1b[nf], acc[mf][nf]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) f1b[nf] = *(const frag*)(sb + b_rd + nf * 2048 + ph1);
#pragma unroll
    for (int mf = 0; mf < 8; ++mf) f1a[mf] = *(const frag*)(sb + a_rd + mf * 2048 + ph1);
#pragma unroll
    for (int mf = 0; mf < 8; ++mf)
#pragma unroll
      for (int nf = 0; nf < 4; ++nf)
        acc[mf][nf] = EMfma<DT>::run(f0a[mf], f0b[nf], PENDING ? acc[mf][nf] : (f32x4){0.f, 0.f, 0.f, 0.f});
#define MRAG_SGB(n_rd) __builtin_amdgcn_sched_group_barrier(0x008, 4, 0); __builtin_amdgcn_sched_group_barrier(0x100, n_rd, 0);
    MRAG_SGB(2) MRAG_SGB(1) MRAG_SGB(2) MRAG_SGB(1) MRAG_SGB(2) MRAG_SGB(1) MRAG_SGB(2) MRAG_SGB(1)
#undef MRAG_SGB
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  auto kstep_sync = [&]() {
    if (loader) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the storing waves' output stores stay in flight
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  for (int lin = first; lin < n_tiles; lin += nwg) {
    kstep(std::false_type{});
    for (int kk = 1; kk < ksteps; ++kk) {
      kstep_sync();
      kstep(std::true_type{});
    }
#pragma unroll
    for (int mf = 0; mf < 8; ++mf)
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) acc[mf][nf] = EMfma<DT>::run(f1a[mf], f1b[nf], acc[mf][nf]);
    // the next tile's first stage is in flight: make sure it has landed BEFORE this tile's stores are
    // issued (vmcnt counts in order), so that the barrier below does not wait for the stores
    if (loader) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // ---- epilogue: n = tn*256 + wm*128 + mf*16 + (lane>>4)*4 + r, token = tm*256 + wn*64 + nf*16 + (lane&15).
    // The tile goes out through LDS in two passes of 128 tokens (nf = 2p, 2p+1): every lane writes its
    // 8-byte groups into a [token][column] slab (the stage buffer just consumed + the pad), then all 512
    // threads store the slab as 16-byte pieces of whole 512-byte rows.  Storing the 8-byte groups
    // straight from the accumulator layout touches 16 cache lines per instruction (QKV GEMM 1.15 -> 1.01 ms).
    const int tm = lin / tiles_n, tn = lin - tm * tiles_n;
    char* slab = sm2 + ((buf ^ 1) ? G2_STAGE : 0);          // free buffer: buffer 0 + pad, or pad + buffer 1
    const int n_l = wm * 128 + (lane >> 4) * 4;             // + mf*16: column inside the tile
    const int n_b = tn * G2_T + n_l;
    const int t_b = tm * G2_T + wn * 64 + (lane & 15);
    // Every global load of the epilogue is issued HERE, back to back, and waited for once: written inside the
    // passes, hipcc puts an s_waitcnt vmcnt(0) behind each of them (8 bias + 32 residual loads = up to 40 serial
    // L2 round trips per tile), and in pass 1 that wait also sits out pass 0's stores (vmcnt counts in order).
    constexpr bool VEC_LDS = (LNF & 2) != 0;     // LNR: bias and gamma of the tile's columns live in LDS (the register budget:
                                                 // 128 accumulators + the 64 residual registers leave no room for two more vectors)
    float* vec = (float*)(sm2 + 2 * G2_STAGE + G2_PAD);
    if (VEC_LDS && tid < 128) {
      const int n0 = tn * G2_T + (tid & 63) * 4;
      float4 t4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n0 < N) t4 = *(const float4*)((tid < 64 ? bias : ln.r_gamma) + n0);
      *(float4*)(vec + (tid >> 6) * 256 + (tid & 63) * 4) = t4;     // (visible after the barrier below)
    }
    float4 bv[VEC_LDS ? 1 : 8];
    float4 xv[((LNF & 3) && !VEC_LDS) ? 8 : 1];  // LNA: s_n (LNR: gamma_n, in LDS)
    e4 rr[8][4];
    float2 tst[(LNF & 3) ? 4 : 1];              // (mu, rstd) of this lane's four tokens
    float ps1[(LNF & 4) ? 4 : 1], ps2[(LNF & 4) ? 4 : 1];
    if (LNF & 3) {
      const float2* st = (const float2*)((LNF & 1) ? ln.a_stats : ln.r_stats);
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) tst[nf] = st[t_b + nf * 16];
    }
    if (LNF & 4) {
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) { ps1[nf] = 0.f; ps2[nf] = 0.f; }
    }
#pragma unroll
    for (int mf = 0; mf < 8; ++mf) {
      const int n0 = n_b + mf * 16;
      if (!VEC_LDS) {
        bv[mf] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n0 < N) bv[mf] = *(const float4*)(bias + n0);
      }
      if ((LNF & 3) && !VEC_LDS) {
        xv[mf] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n0 < N) xv[mf] = *(const float4*)(ln.s_vec + n0);
      }
      if (EPI == EPI_RESID) {
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
          rr[mf][nf] = (e4){(elem)0.f, (elem)0.f, (elem)0.f, (elem)0.f};
          if (n0 < N) rr[mf][nf] = *(const e4*)(R + (size_t)(t_b + nf * 16) * N + n0);
        }
      }
    }
    if (VEC_LDS) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the bias / gamma vectors are in LDS before anyone passes the barrier
    __builtin_amdgcn_s_barrier();   // every wave has read its last fragments out of the buffer the slab reuses (lgkmcnt(0) in kstep)
    asm volatile("" ::: "memory");
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
      for (int mf = 0; mf < 8; ++mf) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int nf = pass * 2 + h;
          const float4 b4 = VEC_LDS ? *(const float4*)(vec + n_l + mf * 16) : bv[VEC_LDS ? 0 : mf];
          const float bq[4] = {b4.x, b4.y, b4.z, b4.w};
          float v[4];
          if (LNF & 1) {
            const float xq[4] = {xv[mf].x, xv[mf].y, xv[mf].z, xv[mf].w};
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = tst[nf].y * (acc[mf][nf][r] - tst[nf].x * xq[r]) + bq[r];
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[mf][nf][r] + bq[r];
          }
          if (EPI == EPI_GELU) {
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = gelu_erf(v[r]);
          }
          if (EPI == EPI_RESID) {
            if (LNF & 2) {
              const float4 g4 = *(const float4*)(vec + 256 + n_l + mf * 16);
              const float xq[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
              for (int r = 0; r < 4; ++r) v[r] += ((float)rr[mf][nf][r] - tst[nf].x) * tst[nf].y * xq[r];
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r) v[r] += (float)rr[mf][nf][r];
            }
          }
          e4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = (elem)v[r];
          if ((LNF & 4) && n_b + mf * 16 < N) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float f = (float)o[r]; ps1[nf] += f; ps2[nf] += f * f; }
          }
          const int tl = wn * 32 + h * 16 + (lane & 15);    // token row inside the pass
          *(e4*)(slab + tl * G2_CPITCH + (n_l + mf * 16) * 2) = o;
        }
      }
      // raw barriers behind LDS-only waits: the global stores below stay in flight across them (a
      // __syncthreads() here drains them: a full HBM write round trip per pass with every CU storing at once)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      // roles: the 256 threads of waves 4-7 store the slab, 16 pieces each.  Thread -> (row r0 + 8 i, piece): the piece and r0
      // are fixed per thread, so every store is lane offset + a wave-uniform base (no per-store address registers: the
      // hoisted 64-bit addresses of a plain store loop spill).  The stores are asm so that hipcc neither counts them nor waits.
      if (storer) {
        const int r0 = (tid - 256) >> 5, piece = tid & 31;
        const int n0 = tn * G2_T + piece * 8;
        const uint32_t lane_off = ((uint32_t)r0 * (uint32_t)N + (uint32_t)(piece * 8)) * 2u;
        const char* srow = slab + r0 * G2_CPITCH + piece * 16;
        if (n0 < N) {
#pragma unroll
          for (int g = 0; g < 16; g += 4) {          // four slab reads in flight, then their four stores
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            u32x4 vv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const uint4 val = *(const uint4*)(srow + (g + j) * 8 * G2_CPITCH);
              vv[j] = (u32x4){val.x, val.y, val.z, val.w};
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int i = g + j;
              const int tok0 = tm * G2_T + (i >> 2) * 64 + pass * 32 + 8 * (i & 3);      // + r0: in lane_off
              const char* base = (const char*)(C + (size_t)tok0 * N + (size_t)tn * G2_T);
              // non-temporal: the output is streamed once, it must not evict the operand panels from L2
              asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 nt\n\ts_nop 1" ::"v"(lane_off), "v"(vv[j]), "s"(base) : "memory");
            }
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // slab reads done (pass 1 rewrites it; after pass 1 the next stage lands in it)
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
    if (LNF & 4) {
      // the four lane groups (lane >> 4) of a wave hold different columns of the SAME tokens: add them up, then one lane per
      // token writes the wave's partial -- slot 2 tn + wm of the token (finalised by enc_ln_stats_kernel in slot order)
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) {
        ps1[nf] += __shfl_xor(ps1[nf], 16); ps1[nf] += __shfl_xor(ps1[nf], 32);
        ps2[nf] += __shfl_xor(ps2[nf], 16); ps2[nf] += __shfl_xor(ps2[nf], 32);
      }
      // waves w and w + 4 hold the two column halves (wm = 0 / 1) of the same 64 tokens: the loading wave hands its sums
      // over through LDS and the storing wave writes both slots (the loading waves issue no global store at all)
      float2* psl = (float2*)(sm2 + 2 * G2_STAGE + G2_PAD + G2_VEC);
      if (!storer && lane < 16) {
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) psl[wn * 64 + nf * 16 + lane] = make_float2(ps1[nf], ps2[nf]);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (storer && lane < 16) {
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
          float2* dst = (float2*)ln.partials + (size_t)(t_b + nf * 16) * ln.np + 2 * tn;
          dst[0] = psl[wn * 64 + nf * 16 + lane];
          dst[1] = make_float2(ps1[nf], ps2[nf]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------ launcher
int enc_device_cus() {
  static int n = 0;
  if (!n) { hipDeviceProp_t pr; int dev = 0; n = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256; }
  return n;
}

typedef void (*Gemm256Fn)(const uint16_t*, const uint16_t*, const float*, const uint16_t*, uint16_t*, int, int, int, int, LnArgs);
struct Gemm256Instance {
  int epi, lnf;
  Gemm256Fn fn;
  bool lds_set;   // hipFuncAttributeMaxDynamicSharedMemorySize raised to G2_LDS: once per process and kernel
};

// The (EPI, LNF) pairs in use: the plain flow's three epilogues, and the fused-LayerNorm flow's LNA consumers (QKV, FFN up),
// STATS producer (layer 0's attention output) and LNR + STATS producers (every other residual GEMM).
template <int DT>
static Gemm256Instance* gemm256_instance(int epi, int lnf) {
  static Gemm256Instance table[] = {
      {EPI_BIAS, 0, enc_gemm256_kernel<DT, EPI_BIAS, 0>, false}, {EPI_GELU, 0, enc_gemm256_kernel<DT, EPI_GELU, 0>, false},
      {EPI_RESID, 0, enc_gemm256_kernel<DT, EPI_RESID, 0>, false}, {EPI_BIAS, 1, enc_gemm256_kernel<DT, EPI_BIAS, 1>, false},
      {EPI_GELU, 1, enc_gemm256_kernel<DT, EPI_GELU, 1>, false}, {EPI_RESID, 4, enc_gemm256_kernel<DT, EPI_RESID, 4>, false},
      {EPI_RESID, 6, enc_gemm256_kernel<DT, EPI_RESID, 6>, false}};
  for (Gemm256Instance& t : table)
    if (t.epi == epi && t.lnf == lnf) return &t;
  return nullptr;
}

int launch_gemm256(int dt, int epi, int lnf, const uint16_t* A, const uint16_t* W, const float* bias, const uint16_t* R, uint16_t* C, int M_pad,
                   int N, int K, const LnArgs& ln, hipStream_t stream) {
  Gemm256Instance* inst = dt == MRAG_F16 ? gemm256_instance<MRAG_F16>(epi, lnf) : gemm256_instance<MRAG_BF16>(epi, lnf);
  if (!inst) return fail(MRAG_ERR_UNSUPPORTED, "no 256 x 256 GEMM instance for epilogue %d with LayerNorm flags %d", epi, lnf);
  if (!inst->lds_set) {
    MRAG_HIP(hipFuncSetAttribute((const void*)inst->fn, hipFuncAttributeMaxDynamicSharedMemorySize, G2_LDS));
    inst->lds_set = true;
  }
  const int tiles_m = M_pad / G2_T, tiles_n = (int)(round_up(N, G2_T) / G2_T);
  const int nwg = std::min(tiles_m * tiles_n, enc_device_cus());   // persistent: a workgroup per CU at the most
  // (starting the XCDs an eighth of a tile apart did not shorten the store phase -- 960 -> 970 -> 984 us for the QKV GEMM
  // at 0 / 4500 / 12000 cycles per XCD; non-temporal stores did, see the epilogue)
  hipLaunchKernelGGL(inst->fn, dim3((unsigned)nwg), dim3(G2_THR), G2_LDS, stream, A, W, bias, R, C, N, K, tiles_m, tiles_n, ln);
  return launched();
}

}  // namespace mrag
