// K6: BERT-family sentence-encoder forward (MiniLM-L6 / bge-base shapes) -- fills the
// LLMProvider.embed slot of the reference (app/core/providers/base.py:6, called from
// app/core/llm_router.py:115).  The reference itself contains no encoder; the architecture
// follows HF BertModel (embeddings + LN, L x {MHA, erf-GELU FFN, post-LN residuals}), pooling
// (mean over the mask, or CLS) and L2 normalisation as in sentence-transformers.
//
// This file is the host side: the parameter table, the forward driver with its two per-layer flows and the C entry
// points.  The kernels (fp16 or bf16 activations / weights, fp32 accumulation and fp32 LN / softmax / GELU math) live
// with their launchers in the sources enc_kernels.h declares:
//   enc_rowwise.hip     enc_embed_ln_kernel, enc_ln_kernel, enc_ln_vec_kernel, enc_pool_kernel and the fused-LayerNorm
//                       flow's helpers enc_ln_stats_kernel, enc_fold_ln_kernel, enc_add_vec_kernel
//   enc_gemm.hip        enc_gemm_kernel (128 x 128 tiles), enc_gemm_skinny_kernel (<= 64 tokens, K split over the waves)
//   enc_gemm256.hip     enc_gemm256_kernel (persistent 256 x 256 tiles, optional LayerNorm folding)
//   enc_attention.hip   enc_attention_s128_kernel (S <= 256, per (batch, head)), enc_attention_kernel (longer S, per
//                       (batch, head, 128 query rows), 512 threads)
// MFMA-bound (~170 MFLOP/token for bge-base); LN/softmax/GELU ride in epilogues.
#include "enc_kernels.h"

namespace mrag {

// ------------------------------------------------------------------ parameters
struct Linear {
  uint16_t* w = nullptr;   // [N_pad][K]
  float* b = nullptr;      // [N_pad]
  int N = 0, K = 0, N_pad = 0;
};

struct Layer {
  Linear qkv, attn_out, ffn_in, ffn_out;
  float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
  // fused-LayerNorm flow (built lazily by fold_layernorms): the Linears that CONSUME a LayerNorm with gamma folded into the
  // weights (c_n in .b, s_n beside it), and the biases of the Linears whose RESIDUAL is a LayerNorm output with its beta added
  Linear qkv_f, ffn_in_f;
  float *qkv_s = nullptr, *ffn_in_s = nullptr, *attn_out_bf = nullptr, *ffn_out_bf = nullptr;
};

// One settable parameter (HF BertModel state-dict name): fp32 [rows][cols] from the caller goes to rows [row0, row0 + rows)
// of `dst` -- converted to the storage dtype when dst is a weight matrix, copied as fp32 otherwise (embedding tables,
// biases, LayerNorm vectors: cols = 1 but for the tables).
struct Param {
  std::string name;
  bool matrix;
  void* dst;
  int rows, cols, row0;
  bool have = false;
  int64_t numel() const { return (int64_t)rows * cols; }
};

struct Encoder : Object {
  mrag_encoder_config cfg;
  float *word = nullptr, *pos = nullptr, *type = nullptr, *eln_g = nullptr, *eln_b = nullptr;
  std::vector<Layer> layers;
  std::vector<Param> params;               // every parameter a forward needs, in state-dict order (build_params)
  std::vector<DevBuf> allocs;              // the parameters' storage
  DevBuf ids, mask, x, y, qkv, ctx, ffn, out, stage;
  DevBuf y2, partials, st1, st2;           // fused-LayerNorm flow: second pre-LayerNorm buffer, partial sums, (mu, rstd) per token
  bool folded = false;                     // fold_layernorms done for the current parameters
  Event ev[2];                             // device work of the last forward (embeddings .. pooling), on its stream
  bool timed = false;
};

static int dev_alloc(Encoder* e, void** p, size_t bytes) {
  DevBuf b;
  MRAG_TRY(b.alloc(bytes));
  (void)hipMemset(b.p, 0, bytes);
  *p = b.p;
  e->allocs.push_back(std::move(b));
  return MRAG_OK;
}

// Rows of the allocation behind a Linear of N outputs (weights, bias and the vectors folded from them): whole 256-row tiles.
// The fused-LayerNorm flow runs the 256 x 256 kernel on every Linear, those with N < 256 included (hidden 64 / 128: N_pad 128),
// and that kernel stages whole 256-row weight tiles: whatever N_pad says, the rows up to the next multiple of 256 exist, as zeros.
static size_t tile_rows(int N) { return (size_t)round_up(N, G2_T); }

static int alloc_linear(Encoder* e, Linear& l, int N, int K) {
  l.N = N; l.K = K; l.N_pad = (int)round_up(N, N >= G2_T ? G2_T : GN);   // 256-row padding lets the 256 x 256 kernel serve it
  MRAG_TRY(dev_alloc(e, (void**)&l.w, tile_rows(N) * K * 2));
  MRAG_TRY(dev_alloc(e, (void**)&l.b, tile_rows(N) * 4));
  return MRAG_OK;
}

// The parameter table of this configuration.  The query, key and value projections are three row blocks of the fused qkv Linear.
static void build_params(Encoder* e) {
  const mrag_encoder_config& c = e->cfg;
  const int H = c.hidden;
  std::vector<Param>& t = e->params;
  auto f32 = [&](const std::string& name, float* dst, int rows, int cols = 1, int row0 = 0) { t.push_back({name, false, dst, rows, cols, row0}); };
  auto linear = [&](const std::string& name, Linear& l, int rows, int row0 = 0) {
    t.push_back({name + ".weight", true, l.w, rows, l.K, row0});
    f32(name + ".bias", l.b, rows, 1, row0);
  };
  auto norm = [&](const std::string& name, float* g, float* b) { f32(name + ".weight", g, H); f32(name + ".bias", b, H); };
  f32("embeddings.word_embeddings.weight", e->word, c.vocab_size, H);
  f32("embeddings.position_embeddings.weight", e->pos, c.max_position, H);
  f32("embeddings.token_type_embeddings.weight", e->type, c.type_vocab_size, H);
  norm("embeddings.LayerNorm", e->eln_g, e->eln_b);
  for (int i = 0; i < c.layers; ++i) {
    Layer& L = e->layers[i];
    const std::string p = "encoder.layer." + std::to_string(i) + ".";
    linear(p + "attention.self.query", L.qkv, H, 0);
    linear(p + "attention.self.key", L.qkv, H, H);
    linear(p + "attention.self.value", L.qkv, H, 2 * H);
    linear(p + "attention.output.dense", L.attn_out, H);
    linear(p + "intermediate.dense", L.ffn_in, c.intermediate);
    linear(p + "output.dense", L.ffn_out, H);
    norm(p + "attention.output.LayerNorm", L.ln1_g, L.ln1_b);
    norm(p + "output.LayerNorm", L.ln2_g, L.ln2_b);
  }
}

// fp32 [rows][K] -> storage dtype at dst rows [row0, row0+rows) of a [N_pad][K] matrix
static int upload_matrix(Encoder* e, const float* src, int is_device, int rows, int K, uint16_t* dst, int row0, hipStream_t stream) {
  const void* s = src;
  if (!is_device) {
    MRAG_TRY(e->stage.ensure((size_t)rows * K * 4));
    MRAG_HIP(hipMemcpyAsync(e->stage.p, src, (size_t)rows * K * 4, hipMemcpyHostToDevice, stream));
    s = e->stage.p;
  }
  MRAG_TRY(launch_prep_rows(s, MRAG_F32, rows, K, dst + (size_t)row0 * K, K, e->cfg.compute_dtype, 0, stream));
  MRAG_HIP(hipStreamSynchronize(stream));
  return MRAG_OK;
}

static int upload_f32(const float* src, int is_device, int64_t n, float* dst, hipStream_t stream) {
  MRAG_HIP(hipMemcpyAsync(dst, src, (size_t)n * 4, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
  MRAG_HIP(hipStreamSynchronize(stream));
  return MRAG_OK;
}

// ------------------------------------------------------------------ forward
// One forward call: its shape, its stream, the activation buffers and which per-layer flow it takes.
struct Fwd {
  Encoder* e;
  int dt, B, S;
  int64_t M;                          // tokens
  int M_pad;                          // rows of every activation buffer: whole 128- or 256-row tiles
  hipStream_t stream;
  uint16_t *x, *y, *qkv, *ctx, *ffn;   // [M_pad][H | H | 3H | H | I]
  bool fused;                         // layer_fused instead of layer_plain
};

// 256 x 256 tiles only when they fill the chip: a small batch (the reference embeds one question, then candidates 50 at a
// time) leaves most CUs idle with 9-72 such tiles, the 128 x 128 kernel gives it four times the workgroups
static bool tiles256_fill_chip(int64_t tiles_m, int64_t tiles_n) { return tiles_m * tiles_n >= enc_device_cus() / 2; }

// C = epi(A l.w^T + l.b [+ R]) on the kernel this batch and this Linear call for
static int run_gemm(const Fwd& f, const uint16_t* A, const Linear& l, const uint16_t* R, uint16_t* C, int epi) {
  if (f.M <= 64 && l.K % 384 == 0 && l.N % 4 == 0)
    return launch_gemm_skinny(f.dt, epi, A, l.w, l.b, R, C, (int)f.M, l.N, l.N_pad, l.K, f.stream);
  if (f.M_pad % G2_T == 0 && l.N_pad % G2_T == 0 && tiles256_fill_chip(f.M_pad / G2_T, l.N_pad / G2_T))
    return launch_gemm256(f.dt, epi, 0, A, l.w, l.b, R, C, f.M_pad, l.N, l.K, LnArgs{}, f.stream);
  return launch_gemm128(f.dt, epi, A, l.w, l.b, R, C, f.M_pad, l.N, l.N_pad, l.K, f.stream);
}

// Shape, buffers (padding rows zeroed) and flow of a forward over B x S tokens.
// MRAG_ENC_NO_FUSED_LN=1 keeps the plain flow (A/B, and the path small batches always take); it is read per forward, not
// once per process: the A/B test flips it between two calls.
static int fwd_begin(Encoder* e, int B, int S, hipStream_t stream, Fwd& f) {
  const int H = e->cfg.hidden, I = e->cfg.intermediate;
  const int64_t M = (int64_t)B * S;
  const int M_pad = (int)round_up(M, M >= 2 * G2_T ? G2_T : GM);
  MRAG_TRY(e->x.ensure((size_t)M_pad * H * 2));
  MRAG_TRY(e->y.ensure((size_t)M_pad * H * 2));
  MRAG_TRY(e->qkv.ensure((size_t)M_pad * 3 * H * 2));
  MRAG_TRY(e->ctx.ensure((size_t)M_pad * H * 2));
  MRAG_TRY(e->ffn.ensure((size_t)M_pad * I * 2));
  const char* off = getenv("MRAG_ENC_NO_FUSED_LN");
  const bool fused = !(off && atoi(off) != 0) && M_pad % G2_T == 0 && H % 16 == 0 && tiles256_fill_chip(round_up(H, G2_T) / G2_T, M_pad / G2_T);
  f = Fwd{e, e->cfg.compute_dtype, B, S, M, M_pad, stream, (uint16_t*)e->x.p, (uint16_t*)e->y.p, (uint16_t*)e->qkv.p, (uint16_t*)e->ctx.p,
          (uint16_t*)e->ffn.p, fused};
  if (M_pad > M) {   // padding rows feed the GEMMs: keep them finite
    MRAG_HIP(hipMemsetAsync(f.x + (size_t)M * H, 0, (size_t)(M_pad - M) * H * 2, stream));
    MRAG_HIP(hipMemsetAsync(f.ctx + (size_t)M * H, 0, (size_t)(M_pad - M) * H * 2, stream));
  }
  return MRAG_OK;
}

// Plain flow, the layer after its attention (x = the layer's input, ctx = the attention context):
//   y = ctx Wo + bo + x          x = LN1(y)
//   ffn = gelu(x W1 + b1)
//   y = ffn W2 + b2 + x          x = LN2(y)   = the next layer's input
static int layer_plain(const Fwd& f, const Layer& L) {
  const int H = f.e->cfg.hidden;
  const float eps = f.e->cfg.layer_norm_eps;
  MRAG_TRY(run_gemm(f, f.ctx, L.attn_out, f.x, f.y, EPI_RESID));
  MRAG_TRY(launch_ln(f.dt, f.y, f.M, H, L.ln1_g, L.ln1_b, eps, f.x, f.stream));
  MRAG_TRY(run_gemm(f, f.x, L.ffn_in, nullptr, f.ffn, EPI_GELU));
  MRAG_TRY(run_gemm(f, f.ffn, L.ffn_out, f.x, f.y, EPI_RESID));
  return launch_ln(f.dt, f.y, f.M, H, L.ln2_g, L.ln2_b, eps, f.x, f.stream);
}

// ------------------------------------------------------------------ fused-LayerNorm flow
// Large batches, every GEMM of a layer on the 256 x 256 kernel: the two LayerNorms of a layer never run as kernels -- the GEMM
// before one emits per-token partial sums, a tiny kernel turns them into (mu, rstd), and the GEMMs after it take the
// PRE-LayerNorm tensor as operand / residual (LnArgs in enc_kernels.h).  Only the last layer's output LayerNorm is
// materialised, for the pooling.
static int ln_slots(int H) { return 2 * (int)(round_up(H, G2_T) / G2_T); }   // partial (sum, sum of squares) per token: two per column tile

// gamma-scaled weights, s / c vectors and beta-augmented biases of the flow, from the plain parameters
static int fold_layernorms(Encoder* e, hipStream_t stream) {
  const int dt = e->cfg.compute_dtype, H = e->cfg.hidden;
  auto fold = [&](const Linear& src, Linear& dst, float*& svec, const float* g, const float* b) -> int {
    if (!dst.w) {
      dst.N = src.N; dst.K = src.K; dst.N_pad = src.N_pad;
      MRAG_TRY(dev_alloc(e, (void**)&dst.w, tile_rows(src.N) * dst.K * 2));
      MRAG_TRY(dev_alloc(e, (void**)&dst.b, tile_rows(src.N) * 4));
      MRAG_TRY(dev_alloc(e, (void**)&svec, tile_rows(src.N) * 4));
    }
    return launch_fold_ln(dt, src.w, src.b, g, b, src.N, src.K, dst.w, dst.b, svec, stream);
  };
  auto add = [&](const float* bias, const float* beta, float*& out) -> int {
    if (!out) MRAG_TRY(dev_alloc(e, (void**)&out, tile_rows(H) * 4));
    return launch_add_vec(bias, beta, H, out, stream);
  };
  for (int li = 0; li < e->cfg.layers; ++li) {
    Layer& L = e->layers[li];
    MRAG_TRY(fold(L.ffn_in, L.ffn_in_f, L.ffn_in_s, L.ln1_g, L.ln1_b));
    MRAG_TRY(add(L.ffn_out.b, L.ln1_b, L.ffn_out_bf));
    if (li > 0) {
      Layer& P = e->layers[li - 1];
      MRAG_TRY(fold(L.qkv, L.qkv_f, L.qkv_s, P.ln2_g, P.ln2_b));
      MRAG_TRY(add(L.attn_out.b, P.ln2_b, L.attn_out_bf));
    }
  }
  e->folded = true;
  return MRAG_OK;
}

// the folded parameters (once per parameter set) and the flow's own buffers
static int fused_begin(const Fwd& f) {
  Encoder* e = f.e;
  if (!e->folded) MRAG_TRY(fold_layernorms(e, f.stream));
  MRAG_TRY(e->y2.ensure((size_t)f.M_pad * e->cfg.hidden * 2));
  MRAG_TRY(e->partials.ensure((size_t)f.M_pad * ln_slots(e->cfg.hidden) * 8));
  MRAG_TRY(e->st1.ensure((size_t)f.M_pad * 8));
  MRAG_TRY(e->st2.ensure((size_t)f.M_pad * 8));
  return MRAG_OK;
}

// qkv = x Wqkv + b for the first layer; after it x = LN2'(y2) of the layer before exists only as y2 and its statistics st2,
// and the LayerNorm is folded into the GEMM: qkv = LN2'(y2) Wqkv + b
static int qkv_fused(const Fwd& f, int li) {
  const Layer& L = f.e->layers[li];
  const int H = f.e->cfg.hidden;
  if (li == 0) return run_gemm(f, f.x, L.qkv, nullptr, f.qkv, EPI_BIAS);
  LnArgs a{}; a.a_stats = (const float*)f.e->st2.p; a.s_vec = L.qkv_s;
  return launch_gemm256(f.dt, EPI_BIAS, 1, (const uint16_t*)f.e->y2.p, L.qkv_f.w, L.qkv_f.b, nullptr, f.qkv, f.M_pad, 3 * H, H, a, f.stream);
}

// The layer after its attention.  y1, y2 are the PRE-LayerNorm tensors, st1, st2 their (mu, rstd) per token; ' = the layer before:
//   y1 = ctx Wo + bo + x            first layer                                               (+ partial sums of y1 -> st1)
//   y1 = ctx Wo + bo + LN2'(y2)     every other layer: bias bo + beta2', residual gamma2' (y2 - mu) rstd from st2    (+ same)
//   ffn = gelu(LN1(y1) W1 + b1)     LN1 folded into the weights and the bias, (mu, rstd) from st1
//   y2 = ffn W2 + b2 + LN1(y1)      bias b2 + beta1, residual gamma1 (y1 - mu) rstd from st1   (+ partial sums of y2 -> st2)
//   x = LN2(y2)                     last layer only: the encoder's output, the one LayerNorm that is materialised
static int layer_fused(const Fwd& f, int li) {
  Encoder* e = f.e;
  const Layer& L = e->layers[li];
  const int H = e->cfg.hidden, I = e->cfg.intermediate, np = ln_slots(H);
  const float eps = e->cfg.layer_norm_eps;
  uint16_t *y1 = f.y, *y2 = (uint16_t*)e->y2.p;
  float *st1 = (float*)e->st1.p, *st2 = (float*)e->st2.p, *partials = (float*)e->partials.p;
  LnArgs a{}; a.partials = partials; a.np = np;
  if (li == 0) {
    MRAG_TRY(launch_gemm256(f.dt, EPI_RESID, 4, f.ctx, L.attn_out.w, L.attn_out.b, f.x, y1, f.M_pad, H, H, a, f.stream));
  } else {
    a.r_stats = st2; a.r_gamma = e->layers[li - 1].ln2_g;
    MRAG_TRY(launch_gemm256(f.dt, EPI_RESID, 6, f.ctx, L.attn_out.w, L.attn_out_bf, y2, y1, f.M_pad, H, H, a, f.stream));
  }
  MRAG_TRY(launch_ln_stats(partials, np, f.M_pad, H, eps, st1, f.stream));
  LnArgs u{}; u.a_stats = st1; u.s_vec = L.ffn_in_s;
  MRAG_TRY(launch_gemm256(f.dt, EPI_GELU, 1, y1, L.ffn_in_f.w, L.ffn_in_f.b, nullptr, f.ffn, f.M_pad, I, H, u, f.stream));
  LnArgs d{}; d.partials = partials; d.np = np; d.r_stats = st1; d.r_gamma = L.ln1_g;
  MRAG_TRY(launch_gemm256(f.dt, EPI_RESID, 6, f.ffn, L.ffn_out.w, L.ffn_out_bf, y1, y2, f.M_pad, H, I, d, f.stream));
  MRAG_TRY(launch_ln_stats(partials, np, f.M_pad, H, eps, st2, f.stream));
  if (li + 1 == e->cfg.layers) MRAG_TRY(launch_ln(f.dt, y2, f.M, H, L.ln2_g, L.ln2_b, eps, f.x, f.stream));
  return MRAG_OK;
}

// embed -> for each layer: qkv -> attention -> layer_plain | layer_fused -> pool
static int forward(Encoder* e, int B, int S, float* d_out, int pool, int normalize, hipStream_t stream) {
  const mrag_encoder_config& c = e->cfg;
  const int H = c.hidden;
  const int32_t* mask = (const int32_t*)e->mask.p;
  Fwd f;
  MRAG_TRY(fwd_begin(e, B, S, stream, f));
  MRAG_TRY(launch_embed_ln(f.dt, (const int32_t*)e->ids.p, f.M, S, H, c.vocab_size, e->word, e->pos, e->type, e->eln_g, e->eln_b, c.layer_norm_eps,
                           f.x, stream));
  if (f.fused) MRAG_TRY(fused_begin(f));
  for (int li = 0; li < c.layers; ++li) {
    const Layer& L = e->layers[li];
    MRAG_TRY(f.fused ? qkv_fused(f, li) : run_gemm(f, f.x, L.qkv, nullptr, f.qkv, EPI_BIAS));
    MRAG_TRY(launch_attention(f.dt, H / c.heads, f.qkv, mask, f.ctx, B, S, H, c.heads, stream));
    MRAG_TRY(f.fused ? layer_fused(f, li) : layer_plain(f, L));
  }
  return launch_pool(f.dt, f.x, mask, B, S, H, pool, normalize, d_out, stream);
}

}  // namespace mrag

using namespace mrag;

extern "C" {

int mrag_encoder_create(const mrag_encoder_config* cfg, int device, mrag_handle* out) {
  if (!cfg || !out) return fail(MRAG_ERR_INVALID, "NULL argument");
  const mrag_encoder_config& c = *cfg;
  if (c.hidden <= 0 || c.hidden % 64 || c.heads <= 0 || c.hidden % c.heads || c.layers <= 0 || c.intermediate <= 0 ||
      c.intermediate % 64 || c.vocab_size <= 0 || c.max_position <= 0 || c.type_vocab_size <= 0)
    return fail(MRAG_ERR_INVALID, "bad encoder config (hidden and intermediate must be multiples of 64)");
  const int dh = c.hidden / c.heads;
  if (dh != 32 && dh != 64) return fail(MRAG_ERR_UNSUPPORTED, "head dim %d not supported (32 or 64)", dh);
  if (c.compute_dtype != MRAG_F16 && c.compute_dtype != MRAG_BF16) return fail(MRAG_ERR_INVALID, "compute dtype must be fp16 or bf16");
  MRAG_TRY(use_device(device));
  Encoder* e = new Encoder();
  e->kind = KIND_ENCODER; e->device = device; e->cfg = c;
  int st = MRAG_OK;
  const int H = c.hidden;
  if (st == MRAG_OK) st = dev_alloc(e, (void**)&e->word, (size_t)c.vocab_size * H * 4);
  if (st == MRAG_OK) st = dev_alloc(e, (void**)&e->pos, (size_t)c.max_position * H * 4);
  if (st == MRAG_OK) st = dev_alloc(e, (void**)&e->type, (size_t)c.type_vocab_size * H * 4);
  if (st == MRAG_OK) st = dev_alloc(e, (void**)&e->eln_g, (size_t)H * 4);
  if (st == MRAG_OK) st = dev_alloc(e, (void**)&e->eln_b, (size_t)H * 4);
  e->layers.resize(c.layers);
  for (int i = 0; i < c.layers && st == MRAG_OK; ++i) {
    Layer& L = e->layers[i];
    if (st == MRAG_OK) st = alloc_linear(e, L.qkv, 3 * H, H);
    if (st == MRAG_OK) st = alloc_linear(e, L.attn_out, H, H);
    if (st == MRAG_OK) st = alloc_linear(e, L.ffn_in, c.intermediate, H);
    if (st == MRAG_OK) st = alloc_linear(e, L.ffn_out, H, c.intermediate);
    for (float** p : {&L.ln1_g, &L.ln1_b, &L.ln2_g, &L.ln2_b})
      if (st == MRAG_OK) st = dev_alloc(e, (void**)p, (size_t)H * 4);
  }
  if (st != MRAG_OK) { delete e; return st; }
  build_params(e);
  *out = register_object(e);
  return MRAG_OK;
}

int mrag_encoder_destroy(mrag_handle h) { return destroy_object(h, KIND_ENCODER); }

int mrag_encoder_set_param(mrag_handle h, const char* name, const float* data, int64_t numel, int is_device, void* stream_) {
  Encoder* e = (Encoder*)lookup(h, KIND_ENCODER);
  if (!e) return MRAG_ERR_INVALID;
  if (!name || !data) return fail(MRAG_ERR_INVALID, "NULL argument");
  MRAG_TRY(use_device(e->device));
  hipStream_t stream = (hipStream_t)stream_;
  const auto p = std::find_if(e->params.begin(), e->params.end(), [&](const Param& q) { return q.name == name; });
  if (p == e->params.end()) return fail(MRAG_ERR_INVALID, "unknown parameter %s", name);
  if (numel != p->numel())
    return fail(MRAG_ERR_INVALID, "%s: expected %lld elements, got %lld", name, (long long)p->numel(), (long long)numel);
  const int st = p->matrix ? upload_matrix(e, data, is_device, p->rows, p->cols, (uint16_t*)p->dst, p->row0, stream)
                           : upload_f32(data, is_device, numel, (float*)p->dst + (size_t)p->row0 * p->cols, stream);
  if (st == MRAG_OK) { p->have = true; e->folded = false; }
  return st;
}

int mrag_encoder_missing_params(mrag_handle h, int* out_missing) {
  Encoder* e = (Encoder*)lookup(h, KIND_ENCODER);
  if (!e) return MRAG_ERR_INVALID;
  if (!out_missing) return fail(MRAG_ERR_INVALID, "out_missing is NULL");
  int miss = 0;
  const Param* first = nullptr;
  for (const Param& p : e->params)
    if (!p.have) { if (!miss) first = &p; ++miss; }
  if (miss) set_error("%d parameters missing, first: %s", miss, first->name.c_str());
  *out_missing = miss;
  return MRAG_OK;
}

int mrag_encoder_forward(mrag_handle h, const int32_t* ids, const int32_t* mask, int B, int S, float* out, int pool, int normalize,
                         int io_is_device, void* stream_) {
  Encoder* e = (Encoder*)lookup(h, KIND_ENCODER);
  if (!e) return MRAG_ERR_INVALID;
  if (B < 0 || S <= 0) return fail(MRAG_ERR_INVALID, "bad batch shape B=%d S=%d", B, S);
  if (S > e->cfg.max_position) return fail(MRAG_ERR_INVALID, "sequence length %d exceeds max_position %d", S, e->cfg.max_position);
  if (pool != MRAG_POOL_MEAN && pool != MRAG_POOL_CLS) return fail(MRAG_ERR_INVALID, "unknown pooling %d", pool);
  if (B == 0) return MRAG_OK;
  if (!ids || !mask || !out) return fail(MRAG_ERR_INVALID, "NULL buffer");
  if ((int64_t)B * S > (1ll << 30)) return fail(MRAG_ERR_UNSUPPORTED, "batch too large; split it");
  int miss = 0;
  MRAG_TRY(mrag_encoder_missing_params(h, &miss));
  if (miss) return fail(MRAG_ERR_INVALID, "encoder has %d unset parameters (%s)", miss, mrag_last_error());
  MRAG_TRY(use_device(e->device));
  hipStream_t stream = (hipStream_t)stream_;
  const size_t nb = (size_t)B * S * 4;
  MRAG_TRY(e->ids.ensure(nb));
  MRAG_TRY(e->mask.ensure(nb));
  const hipMemcpyKind kin = io_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  MRAG_HIP(hipMemcpyAsync(e->ids.p, ids, nb, kin, stream));
  MRAG_HIP(hipMemcpyAsync(e->mask.p, mask, nb, kin, stream));
  float* d_out = out;
  if (!io_is_device) { MRAG_TRY(e->out.ensure((size_t)B * e->cfg.hidden * 4)); d_out = (float*)e->out.p; }
  e->timed = false;
  for (auto& v : e->ev)
    MRAG_TRY(v.create(true));
  MRAG_HIP(hipEventRecord(e->ev[0], stream));
  MRAG_TRY(forward(e, B, S, d_out, pool, normalize, stream));
  MRAG_HIP(hipEventRecord(e->ev[1], stream));
  e->timed = true;
  if (!io_is_device) {
    MRAG_HIP(hipMemcpyAsync(out, d_out, (size_t)B * e->cfg.hidden * 4, hipMemcpyDeviceToHost, stream));
    MRAG_HIP(hipStreamSynchronize(stream));
  }
  return MRAG_OK;
}

int mrag_encoder_last_timing(mrag_handle h, float* out_ms) {
  Encoder* e = (Encoder*)lookup(h, KIND_ENCODER);
  if (!e) return MRAG_ERR_INVALID;
  if (!e->timed) return fail(MRAG_ERR_INVALID, "no completed forward to time");
  if (!out_ms) return fail(MRAG_ERR_INVALID, "out_ms is NULL");
  MRAG_TRY(use_device(e->device));
  MRAG_HIP(hipEventSynchronize(e->ev[1]));
  MRAG_HIP(hipEventElapsedTime(out_ms, e->ev[0], e->ev[1]));
  return MRAG_OK;
}

}  // extern "C"

