// K6, self-attention of the sentence encoder on MFMA, fp32 softmax.  QKV [M_pad][3H] (q | k | v per token) -> ctx [M_pad][H].
//   enc_attention_s128_kernel<DT, DH, SP, NW>  S <= 256: one workgroup per (batch, head), K / V staged once with the keys padded
//                                              to SP = 64 / 128 / 256, P^T and V through gfx950's transposing LDS read
//   enc_attention_kernel<DT, DH, NW>           longer S: per (batch, head, 16 NW = 128 query rows), flash-style loop over 64-key
//                                              blocks, online softmax in the accumulator layout (row = (lane>>4)*4+j, reduced
//                                              over the 16 lanes of a row by shuffles), P staged through LDS as the next MFMA's
//                                              A operand, V transposed on store
// launch_attention at the end of the file picks the instance from (dtype, head dim, S).
#include "enc_kernels.h"

namespace mrag {

// ------------------------------------------------------------------ attention
constexpr float ENC_NO_KEY = -3.0e38f;   // score bias of a key slot beyond the sequence (finite: exp(ENC_NO_KEY - max) == 0 for any max >= -1e30)
// QKV [M_pad][3H] (q | k | v per token), mask [B][S] (1 = token), out [M_pad][H].
// NW waves = 16 NW query rows per workgroup: grid = B * heads * ceil(S / (16 NW)), 64 NW threads, wave w owns query rows
// 16w .. 16w+15 of the block.  The launcher uses NW = 8 (128 query rows, 512 threads), so that 128 queries stage their
// K / V blocks once instead of once per 64-row half (attention 0.59 -> see DESIGN).
template <int DT, int DH, int NW>
__global__ __launch_bounds__(64 * NW) void enc_attention_kernel(const uint16_t* __restrict__ qkv, const int32_t* __restrict__ mask,
                                                                uint16_t* __restrict__ out, int B, int S, int H, int heads, float scale) {
  constexpr int QB = 16 * NW, NT_ = 64 * NW;
  typedef typename EMfma<DT>::frag frag;
  typedef typename EMfma<DT>::elem elem;
  constexpr int KB = 64;                       // keys per block
  constexpr int NK = DH / 32;                  // k-steps of the QK^T contraction
  constexpr int ND = DH / 16;                  // 16-column groups of the output
  __shared__ __attribute__((aligned(16))) elem sK[KB][DH + 8];       // [key][dh]   (+8: 16-B pad against bank conflicts)
  __shared__ __attribute__((aligned(16))) elem sVt[DH][KB + 8];      // [dh][key]
  __shared__ __attribute__((aligned(16))) elem sP[NW][16][KB + 8];   // per wave [q row][key]
  __shared__ float sBias[KB];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nqb = (S + QB - 1) / QB;
  const int qb = blockIdx.x % nqb;
  const int hh = (blockIdx.x / nqb) % heads;
  const int bb = blockIdx.x / (nqb * heads);
  const size_t ld = (size_t)3 * H;
  const uint16_t* base = qkv + (size_t)bb * S * ld;
  const int q_row = qb * QB + w * 16 + (lane & 15);           // A operand row of this lane
  // Q fragments: lane holds Q[q_row][k = 32*ks + 8*(lane>>4) + j]
  frag qf[NK];
#pragma unroll
  for (int ks = 0; ks < NK; ++ks) {
    frag z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (elem)0.f;
    if (q_row < S) z = *(const frag*)(base + (size_t)q_row * ld + hh * DH + ks * 32 + (lane >> 4) * 8);
    qf[ks] = z;
  }
  f32x4 o[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) o[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m_run[4], l_run[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_run[r] = -1e30f; l_run[r] = 0.f; }

  for (int k0 = 0; k0 < S; k0 += KB) {
    __syncthreads();
    // stage K (row-major) and V (transposed) of this key block; 256 threads x 16 B = one 64 x 32 slab per pass
    for (int e = tid; e < KB * (DH / 8); e += NT_) {
      const int key = e / (DH / 8), c = e % (DH / 8);
      frag kv, vv;
#pragma unroll
      for (int j = 0; j < 8; ++j) { kv[j] = (elem)0.f; vv[j] = (elem)0.f; }
      if (k0 + key < S) {
        kv = *(const frag*)(base + (size_t)(k0 + key) * ld + H + hh * DH + c * 8);
        vv = *(const frag*)(base + (size_t)(k0 + key) * ld + 2 * H + hh * DH + c * 8);
      }
      *(frag*)&sK[key][c * 8] = kv;
#pragma unroll
      for (int j = 0; j < 8; ++j) sVt[c * 8 + j][key] = vv[j];
    }
    // masked keys get -1e30 (a row with no valid key attends all S of them evenly, as the oracle does); slots beyond S get
    // ENC_NO_KEY, far enough below that to vanish from that row's softmax as well
    if (tid < KB) sBias[tid] = k0 + tid >= S ? ENC_NO_KEY : mask[(size_t)bb * S + k0 + tid] != 0 ? 0.f : -1e30f;
    __syncthreads();
    // S = Q K^T  (16 q rows x 64 keys per wave): B operand lane holds K[key = 16*nf + (lane&15)][k chunk]
    f32x4 sc[4];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      sc[nf] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NK; ++ks) {
        const frag kf = *(const frag*)&sK[nf * 16 + (lane & 15)][ks * 32 + (lane >> 4) * 8];
        sc[nf] = EMfma<DT>::run(qf[ks], kf, sc[nf]);
      }
    }
    // online softmax: this lane's rows are (lane>>4)*4 + r, its columns 16*nf + (lane&15)
    float p[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = -1e30f;
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) {
        const float v = sc[nf][r] * scale + sBias[nf * 16 + (lane & 15)];
        p[nf][r] = v;
        mx = fmaxf(mx, v);
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
      const float m_new = fmaxf(m_run[r], mx);
      const float alpha = __expf(m_run[r] - m_new);
      float rs = 0.f;
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) {
        const float e = __expf(p[nf][r] - m_new);
        p[nf][r] = e;
        rs += e;
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) rs += __shfl_xor(rs, off);
      l_run[r] = l_run[r] * alpha + rs;
      m_run[r] = m_new;
#pragma unroll
      for (int d = 0; d < ND; ++d) o[d][r] *= alpha;
    }
    // P -> LDS (this wave's 16 x 64 slab), then O += P V
#pragma unroll
    for (int nf = 0; nf < 4; ++nf)
#pragma unroll
      for (int r = 0; r < 4; ++r) sP[w][(lane >> 4) * 4 + r][nf * 16 + (lane & 15)] = (elem)p[nf][r];
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's own LDS writes are visible to its reads
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ks = 0; ks < KB / 32; ++ks) {
      const frag pf = *(const frag*)&sP[w][lane & 15][ks * 32 + (lane >> 4) * 8];
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const frag vf = *(const frag*)&sVt[d * 16 + (lane & 15)][ks * 32 + (lane >> 4) * 8];
        o[d] = EMfma<DT>::run(pf, vf, o[d]);
      }
    }
  }
  // out[row][hh*DH + 16*d + (lane&15)], row = qb*QB + w*16 + (lane>>4)*4 + r.  The wave's 16 x DH block goes
  // through its (now idle) P slab so that it leaves as 16-byte pieces of whole DH-wide rows instead of
  // sixteen 2-byte stores per lane.
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float inv = 1.0f / l_run[r];
#pragma unroll
    for (int d = 0; d < ND; ++d) sP[w][(lane >> 4) * 4 + r][d * 16 + (lane & 15)] = (elem)(o[d][r] * inv);
  }
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_wave_barrier();
  constexpr int PIECES = DH / 8;                 // 16-byte pieces per row
  for (int e = lane; e < 16 * PIECES; e += 64) {
    const int rr = e / PIECES, pc = e % PIECES;
    const int row = qb * QB + w * 16 + rr;
    if (row < S) *(frag*)&out[((size_t)bb * S + row) * H + hh * DH + pc * 8] = *(const frag*)&sP[w][rr][pc * 8];
  }
}

// ------------------------------------------------------------------ attention, sequences of <= 256 tokens
// One workgroup (4 waves) per (batch, head): K and V of the head are staged ONCE, row-major, with all global loads in flight
// together; every wave then owns 32 query rows (two 16-row MFMA groups) against all 128 (padded) keys -- no key-block loop, no
// online-softmax rescaling, no per-block barriers.  The two operands whose contraction index runs along LDS ROWS come from
// gfx950's transposing LDS read (ds_read_b64_tr_b16, cdna_hip_programming.md T10):
//   V  [key][dh]  -> B operand of P V   (lane n = dh column, 8 consecutive keys): two reads of a 4-key x 16-column block
//   P^T[key][row] -> A operand of P V   (lane m = query row, 8 consecutive keys): the accumulator layout of Q K^T already holds
//                    4 consecutive rows of one key per lane, so P goes to LDS as ONE 8-byte store per accumulator (the
//                    generic kernel above writes sixteen 2-byte stores per lane and block, and eight per V chunk).
// Row reductions of the softmax stay inside a 16-lane DPP row (row_ror), no LDS permutes.
typedef short tr_s4 __attribute__((ext_vector_type(4)));
template <typename F>
__device__ __forceinline__ F tr_read_pair(const void* lo_ptr, const void* hi_ptr) {
  typedef __attribute__((address_space(3))) tr_s4* lp;
  union { tr_s4 h[2]; F f; } u;
  u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)lo_ptr);
  u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)hi_ptr);
  return u.f;
}
template <int N>
__device__ __forceinline__ float dpp_ror16(float x) {   // value of the lane N places further round its 16-lane row
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x120 + N, 0xF, 0xF, false));
}
__device__ __forceinline__ float row16_max(float x) {
  x = fmaxf(x, dpp_ror16<8>(x)); x = fmaxf(x, dpp_ror16<4>(x)); x = fmaxf(x, dpp_ror16<2>(x)); return fmaxf(x, dpp_ror16<1>(x));
}
__device__ __forceinline__ float row16_sum(float x) {
  x += dpp_ror16<8>(x); x += dpp_ror16<4>(x); x += dpp_ror16<2>(x); return x + dpp_ror16<1>(x);
}

// SP = padded key count (64 / 128 / 256), NW waves; every wave owns SP / NW query rows (groups of 16).
template <int DT, int DH, int SP, int NW>
__global__ __launch_bounds__(64 * NW) void enc_attention_s128_kernel(const uint16_t* __restrict__ qkv, const int32_t* __restrict__ mask,
                                                                     uint16_t* __restrict__ out, int B, int S, int H, int heads, float scale) {
  typedef typename EMfma<DT>::frag frag;
  typedef typename EMfma<DT>::elem elem;
  typedef elem e4 __attribute__((ext_vector_type(4)));
  constexpr int NT_ = 64 * NW;
  constexpr int NK = DH / 32;                  // k steps of Q K^T
  constexpr int ND = DH / 16;                  // 16-column groups of the output
  constexpr int NFK = SP / 16;                 // 16-key groups
  constexpr int KS = SP / 32;                  // k steps of P V
  constexpr int GROUPS = SP / (NW * 16);       // 16-row groups per wave
  constexpr bool HOIST = KS * ND <= 16;        // V fragments kept in registers across the wave's row groups (<= 64 VGPRs)
  constexpr int KP = DH + 8;                   // row pitch of the K / V images (elements): 16-byte pad
  constexpr int PIECES = DH / 8;               // 16-byte pieces per row
  constexpr int LOADS = SP * PIECES / NT_;
  __shared__ __attribute__((aligned(16))) elem sK[SP][KP];
  __shared__ __attribute__((aligned(16))) elem sV[SP][KP];
  __shared__ __attribute__((aligned(16))) elem sPt[NW][SP][16];    // per wave: P^T [key][query row]; afterwards its [16][DH] output slab
  __shared__ float sBias[SP];
  constexpr int SLP = SP >= KP ? KP : DH;      // row pitch of the output slab inside the wave's P^T area (SP x 16 elements)
  static_assert(SP * 16 >= 16 * SLP, "output slab must fit the wave's P^T area");
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int hh = blockIdx.x % heads, bb = blockIdx.x / heads;
  const size_t ld = (size_t)3 * H;
  const uint16_t* base = qkv + (size_t)bb * S * ld;
  {
    frag kv[LOADS], vv[LOADS];
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      const int e = tid + i * NT_, key = e / PIECES, c = e % PIECES;
#pragma unroll
      for (int j = 0; j < 8; ++j) { kv[i][j] = (elem)0.f; vv[i][j] = (elem)0.f; }
      if (key < S) {
        kv[i] = *(const frag*)(base + (size_t)key * ld + H + hh * DH + c * 8);
        vv[i] = *(const frag*)(base + (size_t)key * ld + 2 * H + hh * DH + c * 8);
      }
    }
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
      const int e = tid + i * NT_, key = e / PIECES, c = e % PIECES;
      *(frag*)&sK[key][c * 8] = kv[i];
      *(frag*)&sV[key][c * 8] = vv[i];
    }
  }
  for (int i = tid; i < SP; i += NT_) sBias[i] = i >= S ? ENC_NO_KEY : mask[(size_t)bb * S + i] != 0 ? 0.f : -1e30f;   // (as above)
  __syncthreads();
  const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 2, tp = i16 & 3;   // tr read: lane 4q+p of a 16-lane group addresses row q, columns 4p..4p+3
  auto v_frag = [&](int ks, int d) -> frag {     // V[keys 32 ks + 8 g .. +7][dh 16 d + i16]
    return tr_read_pair<frag>(&sV[ks * 32 + 8 * g + tq][d * 16 + 4 * tp], &sV[ks * 32 + 8 * g + 4 + tq][d * 16 + 4 * tp]);
  };
  frag vf[HOIST ? KS : 1][ND];
  if (HOIST) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int d = 0; d < ND; ++d) vf[ks][d] = v_frag(ks, d);
  }
  float bias[NFK];
#pragma unroll
  for (int nf = 0; nf < NFK; ++nf) bias[nf] = sBias[nf * 16 + i16];
#pragma unroll 1
  for (int rg = 0; rg < GROUPS; ++rg) {
    const int row0 = (w * GROUPS + rg) * 16;
    if (row0 >= S) break;                                                  // (wave-uniform)
    const int q_row = row0 + i16;
    frag qf[NK];
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      frag z;
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = (elem)0.f;
      if (q_row < S) z = *(const frag*)(base + (size_t)q_row * ld + hh * DH + ks * 32 + g * 8);
      qf[ks] = z;
    }
    // scores: lane holds rows 4 g + r, key 16 nf + i16
    f32x4 sc[NFK];
#pragma unroll
    for (int nf = 0; nf < NFK; ++nf) {
      sc[nf] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NK; ++ks) {
        const frag kf = *(const frag*)&sK[nf * 16 + i16][ks * 32 + g * 8];
        sc[nf] = EMfma<DT>::run(qf[ks], kf, sc[nf]);
      }
    }
    float inv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = -1e30f;
#pragma unroll
      for (int nf = 0; nf < NFK; ++nf) { sc[nf][r] = sc[nf][r] * scale + bias[nf]; mx = fmaxf(mx, sc[nf][r]); }
      mx = row16_max(mx);
      float rs = 0.f;
#pragma unroll
      for (int nf = 0; nf < NFK; ++nf) { const float e = __expf(sc[nf][r] - mx); sc[nf][r] = e; rs += e; }
      inv[r] = 1.0f / row16_sum(rs);
    }
    // P^T -> LDS: one 8-byte store per accumulator (4 consecutive query rows of one key)
#pragma unroll
    for (int nf = 0; nf < NFK; ++nf) {
      e4 pk;
#pragma unroll
      for (int r = 0; r < 4; ++r) pk[r] = (elem)sc[nf][r];
      *(e4*)&sPt[w][nf * 16 + i16][4 * g] = pk;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave's own LDS writes are visible to its reads
    __builtin_amdgcn_wave_barrier();
    f32x4 o[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) o[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const frag pf = tr_read_pair<frag>(&sPt[w][ks * 32 + 8 * g + tq][4 * tp], &sPt[w][ks * 32 + 8 * g + 4 + tq][4 * tp]);
#pragma unroll
      for (int d = 0; d < ND; ++d) o[d] = EMfma<DT>::run(pf, HOIST ? vf[HOIST ? ks : 0][d] : v_frag(ks, d), o[d]);
    }
    // out[row][hh*DH + 16 d + i16], row = row0 + 4 g + r: through the wave's (now idle) P^T area as a [16][DH] slab, so that it
    // leaves as 16-byte pieces of whole rows
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    elem* slab = &sPt[w][0][0];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int d = 0; d < ND; ++d) slab[(4 * g + r) * SLP + d * 16 + i16] = (elem)(o[d][r] * inv[r]);
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    for (int e = lane; e < 16 * PIECES; e += 64) {
      const int rr = e / PIECES, pc = e % PIECES;
      const int row = row0 + rr;
      if (row < S) *(frag*)&out[((size_t)bb * S + row) * H + hh * DH + pc * 8] = *(const frag*)&slab[rr * SLP + pc * 8];
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------------------ launcher: (dtype, head dim, S) -> instance
template <int DT, int DH>
static void launch_attention_as(const uint16_t* qkv, const int32_t* mask, uint16_t* ctx, int B, int S, int H, int heads, float scale,
                                hipStream_t stream) {
  const dim3 whole((unsigned)(B * heads));   // whole-sequence kernel: one workgroup per (batch, head)
  if (S <= 64) hipLaunchKernelGGL((enc_attention_s128_kernel<DT, DH, 64, 4>), whole, dim3(256), 0, stream, qkv, mask, ctx, B, S, H, heads, scale);
  else if (S <= 128) hipLaunchKernelGGL((enc_attention_s128_kernel<DT, DH, 128, 4>), whole, dim3(256), 0, stream, qkv, mask, ctx, B, S, H, heads, scale);
  else if (S <= 256) hipLaunchKernelGGL((enc_attention_s128_kernel<DT, DH, 256, 8>), whole, dim3(512), 0, stream, qkv, mask, ctx, B, S, H, heads, scale);
  else   // longer sequences: 128 query rows per workgroup (NW = 8, 512 threads), keys in blocks of 64 with an online softmax
    hipLaunchKernelGGL((enc_attention_kernel<DT, DH, 8>), dim3((unsigned)(B * heads * ((S + 127) / 128))), dim3(512), 0, stream, qkv, mask, ctx, B, S,
                       H, heads, scale);
}

int launch_attention(int dt, int dh, const uint16_t* qkv, const int32_t* mask, uint16_t* ctx, int B, int S, int H, int heads, hipStream_t stream) {
  if (dh != 32 && dh != 64) return fail(MRAG_ERR_UNSUPPORTED, "head dim %d not supported (32 or 64)", dh);
  const float scale = 1.0f / sqrtf((float)dh);
  if (dt == MRAG_F16) {
    if (dh == 32) launch_attention_as<MRAG_F16, 32>(qkv, mask, ctx, B, S, H, heads, scale, stream);
    else launch_attention_as<MRAG_F16, 64>(qkv, mask, ctx, B, S, H, heads, scale, stream);
  } else {
    if (dh == 32) launch_attention_as<MRAG_BF16, 32>(qkv, mask, ctx, B, S, H, heads, scale, stream);
    else launch_attention_as<MRAG_BF16, 64>(qkv, mask, ctx, B, S, H, heads, scale, stream);
  }
  return launched();
}

}  // namespace mrag
