// C-ABI layer (include/dk_hip.h), part 1: the error string, dk_tune_set, the layout rules (dk_weight_pitch*, dk_mx_scale_bytes) and every
// stand-alone operator entry.  The engines are mmdit_engine.hip and vae_engine.hip.  Host code only: no kernels are defined here.
#include <cmath>
#include <cstdio>

#include "dk_engine.h"

// The library's two thread-local objects: the last error, and the attention workspace of the stand-alone dk_attention_* entries below
// (dk_attention_set_workspace; the engines pass their own region and never consult it)
static thread_local std::string g_last_error;
static thread_local AttnWs g_attn_ws;
void dk_set_error(const std::string& msg) { g_last_error = msg; }

extern "C" int dk_abi_version(void) { return DK_ABI_VERSION; }
extern "C" const char* dk_last_error(void) { return g_last_error.c_str(); }

// Rows of K >= g_dk_pitch_min_k elements (the [h, 5h] linear2 and [h, 4h] fc2 weights of FLUX and the activations they
// multiply) are stored with 64 elements of padding: a 24-30 KB row stride makes the K-tile DMA of 256 rows camp on a few
// memory channels (linear2 of FLUX: 369 -> 345 us with the padded pitch, profiles/archive/r01_gemm_lab_pitch.log).
int g_dk_pitch_min_k = 8192;
extern "C" int32_t dk_weight_pitch(int32_t k) { return k >= g_dk_pitch_min_k ? k + 64 : k; }
extern "C" int32_t dk_weight_pitch_fp8(int32_t k) { return k >= g_dk_pitch_min_k ? k + 128 : k; }
extern "C" size_t dk_mx_scale_bytes(int64_t rows, int32_t k) { return (size_t)((k + 127) / 128) * (size_t)mx_nblk((long)rows) * 512; }

// every knob is defined, with its values and its default, in the file that reads it
extern "C" int dk_tune_set(const char* key, int32_t value) {
  static const struct { const char* key; int* knob; } knobs[] = {
      {"gemm", &g_dk_gemm_mode}, {"gemm_v4", &g_dk_v4_auto}, {"gemm_skew", &g_dk_v4_skew}, {"gemm_mf", &g_dk_v3_mf},
      {"gemm_split", &g_dk_v3_split}, {"gemm_split_min", &g_dk_v3_split_min}, {"gemm_pair_nk", &g_dk_pair_split_nk},
      {"gemm_fuse_k", &g_dk_fuse_k}, {"gemm_fuse_q", &g_dk_fuse_qg}, {"attn", &g_dk_attn_mode}, {"attn_fuse_q", &g_dk_fuse_q},
      {"attn_split", &g_dk_attn5_split}, {"attn_track", &g_dk_attn5_track}, {"pitch_min_k", &g_dk_pitch_min_k}, {"conv_halo", &g_dk_conv_halo}, {"conv_v4", &g_dk_conv_v4}};
  DK_REQUIRE(key != nullptr, "null key");
  for (const auto& k : knobs)
    if (strcmp(key, k.key) == 0) { *k.knob = value; return 0; }
  dk_set_error(std::string("unknown tuning key: ") + key);
  return -1;
}

// ---------------------------------------------------------------------------------------------
// operator-level wrappers: one implementation per operator, which takes the element type; the *_bf16 / *_f16 entries name theirs
// ---------------------------------------------------------------------------------------------
static GemmParams gemm_params_from_desc(int dtype, const dk_gemm_desc* d) {
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.dtype = dtype;
  p.A = (const bf16_t*)d->A; p.W = (const bf16_t*)d->W; p.C = (bf16_t*)d->C;
  p.bias = (const bf16_t*)d->bias; p.gate = (const bf16_t*)d->gate; p.res = (const bf16_t*)d->res;
  p.M = d->M; p.N = d->N; p.K = d->K;
  p.lda = d->lda; p.ldc = d->ldc; p.ldr = d->ldr;
  p.a_seg_len = d->a_seg_len > 0 ? d->a_seg_len : d->M; p.a_seg_stride = d->a_seg_stride;
  p.c_seg_len = d->c_seg_len > 0 ? d->c_seg_len : d->M; p.c_seg_stride = d->c_seg_stride;
  p.r_seg_len = d->r_seg_len > 0 ? d->r_seg_len : d->M; p.r_seg_stride = d->r_seg_stride;
  p.gate_seg_len = d->gate_seg_len > 0 ? d->gate_seg_len : d->M; p.gate_stride = d->gate_stride;
  p.alpha = d->alpha; p.epi = d->epilogue; p.ldw = d->ldw;
  p.workspace = d->workspace; p.workspace_bytes = d->workspace_bytes;
  return p;
}

extern "C" size_t dk_gemm_workspace_bytes(void) { return dk_gemm_split_workspace_bytes(); }

static int gemm(int dtype, const dk_gemm_desc* d, void* stream) {
  DK_REQUIRE(d != nullptr, "null descriptor");
  return dk_launch_gemm(gemm_params_from_desc(dtype, d), S_(stream));
}
extern "C" int dk_gemm_bf16(const dk_gemm_desc* d, void* stream) { return gemm(DK_DTYPE_BF16, d, stream); }
extern "C" int dk_gemm_f16(const dk_gemm_desc* d, void* stream) { return gemm(DK_DTYPE_F16, d, stream); }

static int gemm_plan(int dtype, const dk_gemm_desc* d, const dk_gemm_desc* d2, dk_gemm_plan_t* plan) {
  DK_REQUIRE(d != nullptr && plan != nullptr, "null descriptor / plan");
  const GemmParams p2 = d2 != nullptr ? gemm_params_from_desc(dtype, d2) : GemmParams{};
  return dk_gemm_plan_call(gemm_params_from_desc(dtype, d), d2 != nullptr ? &p2 : nullptr, *plan);
}
extern "C" int dk_gemm_plan(const dk_gemm_desc* d, const dk_gemm_desc* d2, dk_gemm_plan_t* plan) { return gemm_plan(DK_DTYPE_BF16, d, d2, plan); }
extern "C" int dk_gemm_plan_f16(const dk_gemm_desc* d, const dk_gemm_desc* d2, dk_gemm_plan_t* plan) { return gemm_plan(DK_DTYPE_F16, d, d2, plan); }

// the engine-only fields of GemmParams beside a descriptor (dk_gemm_side / dk_gemm_fp8_side: same names); null: nothing fused
template <class P, class F>
static void set_fused(P& p, const F* f) {
  if (f == nullptr) return;
  p.n_split = f->n_split; p.C2 = (decltype(p.C2))f->C2; p.ldc2 = f->ldc2; p.epi2 = f->epi2;
  p.kn_w = (const bf16_t*)f->kn_w; p.kn_rope = f->kn_rope;
  p.kn_col0 = f->kn_col0; p.kn_col1 = f->kn_col1; p.kn_D = f->kn_D; p.kn_pos_off = f->kn_pos_off; p.kn_seg_len = f->kn_seg_len; p.kn_eps = f->kn_eps;
  p.qn_w = (const bf16_t*)f->qn_w; p.qn_col0 = f->qn_col0; p.qn_col1 = f->qn_col1;
}

// (no checks of their own: dk_gemm_route / the *_eligible functions decide what a form launches)
static int gemm_fused(int dtype, const dk_gemm_desc* d, const dk_gemm_side* f, const dk_gemm_desc* d2, const dk_gemm_side* f2, void* stream) {
  DK_REQUIRE(d != nullptr && (d2 != nullptr || f2 == nullptr), "null descriptor");
  GemmParams p = gemm_params_from_desc(dtype, d);
  set_fused(p, f);
  if (d2 == nullptr) return dk_launch_gemm(p, S_(stream));
  GemmParams p2 = gemm_params_from_desc(dtype, d2);
  set_fused(p2, f2);
  return dk_launch_gemm_pair(p, p2, S_(stream));
}
extern "C" int dk_gemm_fused_bf16(const dk_gemm_desc* d, const dk_gemm_side* f, const dk_gemm_desc* d2, const dk_gemm_side* f2, void* stream) {
  return gemm_fused(DK_DTYPE_BF16, d, f, d2, f2, stream);
}
extern "C" int dk_gemm_fused_f16(const dk_gemm_desc* d, const dk_gemm_side* f, const dk_gemm_desc* d2, const dk_gemm_side* f2, void* stream) {
  return gemm_fused(DK_DTYPE_F16, d, f, d2, f2, stream);
}

extern "C" int dk_gemm_fused_plan(const dk_gemm_desc* d, const dk_gemm_side* f, const dk_gemm_desc* d2, const dk_gemm_side* f2,
                                  dk_gemm_plan_t* plan) {
  DK_REQUIRE(d != nullptr && plan != nullptr && (d2 != nullptr || f2 == nullptr), "null descriptor / plan");
  GemmParams p = gemm_params_from_desc(DK_DTYPE_BF16, d), p2 = d2 != nullptr ? gemm_params_from_desc(DK_DTYPE_BF16, d2) : GemmParams{};
  set_fused(p, f);
  if (d2 != nullptr) set_fused(p2, f2);
  return dk_gemm_plan_call(p, d2 != nullptr ? &p2 : nullptr, *plan);
}

int conv3x3_launch(int dtype, const dk_conv_desc* d, void* workspace, hipStream_t stream, dk_gemm_plan_t* rec) {  // (dk_engine.h)
  DK_REQUIRE(d != nullptr, "null descriptor");
  GemmParams p;
  memset(&p, 0, sizeof(p));
  p.dtype = dtype;
  p.A = (const bf16_t*)d->x; p.W = (const bf16_t*)d->w; p.C = (bf16_t*)d->y;
  p.bias = (const bf16_t*)d->bias; p.res = (const bf16_t*)d->res;
  p.M = d->B * d->H * d->W; p.N = d->O; p.K = 9 * d->C;
  p.lda = d->C; p.ldc = d->ldy; p.ldr = d->ldr;
  p.a_seg_len = p.c_seg_len = p.r_seg_len = p.gate_seg_len = p.M;
  p.alpha = 1.0f; p.epi = d->epilogue;
  p.conv = 1; p.cB = d->B; p.cH = d->H; p.cW = d->W; p.cC = d->C; p.ups = d->upsample;
  p.zeros = (const bf16_t*)d->zeros;
  if (workspace) { p.workspace = workspace; p.workspace_bytes = dk_gemm_split_workspace_bytes(); }
  DK_REQUIRE(d->upsample >= 0 && d->upsample <= 2, "upsample: 0 plain, 1 nearest-x2 input view, 2 stride-2 (downsample)");
  if (d->upsample == 1) DK_REQUIRE(d->H % 2 == 0 && d->W % 2 == 0, "upsampled conv needs even output size");
  if (rec != nullptr) return dk_gemm_plan_call(p, nullptr, *rec);
  return dk_launch_gemm(p, stream);
}
extern "C" int dk_conv3x3_bf16(const dk_conv_desc* d, void* stream) { return conv3x3_launch(DK_DTYPE_BF16, d, nullptr, S_(stream)); }
extern "C" int dk_conv3x3_f16(const dk_conv_desc* d, void* stream) { return conv3x3_launch(DK_DTYPE_F16, d, nullptr, S_(stream)); }
static int conv3x3_plan(int dtype, const dk_conv_desc* d, dk_gemm_plan_t* plan) {
  DK_REQUIRE(plan != nullptr, "null plan");
  return conv3x3_launch(dtype, d, nullptr, nullptr, plan);
}
extern "C" int dk_conv3x3_plan(const dk_conv_desc* d, dk_gemm_plan_t* plan) { return conv3x3_plan(DK_DTYPE_BF16, d, plan); }
extern "C" int dk_conv3x3_plan_f16(const dk_conv_desc* d, dk_gemm_plan_t* plan) { return conv3x3_plan(DK_DTYPE_F16, d, plan); }
// The same launches with the K-split workspace the VAE engines attach (VaeRun::conv): the buffer and the rules of dk_gemm_desc.workspace.  A
// buffer the split could not use is refused -- it never silently runs unsplit.  (plan: only the size is known, the pointer is a made-up aligned one)
static int conv3x3_ws(int dtype, const dk_conv_desc* d, void* workspace, size_t workspace_bytes, hipStream_t stream, dk_gemm_plan_t* rec) {
  DK_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 255) == 0, "conv K-split workspace: 256-byte aligned, not NULL");
  DK_REQUIRE(workspace_bytes >= dk_gemm_split_workspace_bytes(), "conv K-split workspace too small (dk_gemm_workspace_bytes())");
  return conv3x3_launch(dtype, d, workspace, stream, rec);
}
extern "C" int dk_conv3x3_ws_bf16(const dk_conv_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
  return conv3x3_ws(DK_DTYPE_BF16, d, workspace, workspace_bytes, S_(stream), nullptr);
}
extern "C" int dk_conv3x3_ws_f16(const dk_conv_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
  return conv3x3_ws(DK_DTYPE_F16, d, workspace, workspace_bytes, S_(stream), nullptr);
}
static int conv3x3_ws_plan(int dtype, const dk_conv_desc* d, size_t workspace_bytes, dk_gemm_plan_t* plan) {
  DK_REQUIRE(plan != nullptr, "null plan");
  if (workspace_bytes == 0) return conv3x3_launch(dtype, d, nullptr, nullptr, plan);  // (0: none, as dk_attention_plan)
  return conv3x3_ws(dtype, d, (void*)(uintptr_t)256, workspace_bytes, nullptr, plan);
}
extern "C" int dk_conv3x3_ws_plan(const dk_conv_desc* d, size_t workspace_bytes, dk_gemm_plan_t* plan) {
  return conv3x3_ws_plan(DK_DTYPE_BF16, d, workspace_bytes, plan);
}
extern "C" int dk_conv3x3_ws_plan_f16(const dk_conv_desc* d, size_t workspace_bytes, dk_gemm_plan_t* plan) {
  return conv3x3_ws_plan(DK_DTYPE_F16, d, workspace_bytes, plan);
}

// Workspace of the stand-alone attention launches (dk_attention_*) of this host thread.  attention5.hip splits the query blocks of a launch's last, partial round of the
// CUs along the keys where that shortens the round (dk_attention_route, attention.hip: FLUX 1024 x 1024 with four images, 1632 blocks on 256 CUs -- the
// 96 blocks of the seventh round in two key ranges each; with one image the 152 blocks of the second round stay whole); the partial results (bf16
// O / l, offset, l per row) go through this buffer.  Without one (or with one too small for a launch) the blocks are not split: same results up
// to the rounding of the partials, a longer last round.
extern "C" size_t dk_attention_workspace_bytes(void) { return (size_t)1020 * DK_ATTN5_JOB_BYTES; }  // <= 255 blocks x 4 key ranges
extern "C" int dk_attention_set_workspace(void* workspace, size_t bytes) {
  DK_REQUIRE(workspace == nullptr || ((uintptr_t)workspace & 255) == 0, "attention workspace: 256-byte aligned (or NULL)");
  g_attn_ws = AttnWs{workspace, workspace ? bytes : 0};
  return 0;
}

extern "C" int dk_attention_bf16(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t H, int32_t S,
                                 int32_t D, int32_t ld, int32_t ldo, float scale, void* stream) {
  AttnParams p;
  p.Q = (const bf16_t*)q; p.K = (const bf16_t*)k; p.V = (const bf16_t*)v; p.O = (bf16_t*)out;
  p.B = B; p.H = H; p.S = S; p.D = D; p.ld = ld; p.ldo = ldo; p.scale = scale;
  return dk_launch_attention(p, g_attn_ws, S_(stream));
}

extern "C" int dk_attention_bias_bf16(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t H, int32_t S, int32_t D,
                                      int32_t ld, int32_t ldo, float scale, const void* bias, int64_t bias_head_stride, int32_t ldb,
                                      void* stream) {
  DK_REQUIRE(bias != nullptr, "bias missing (use dk_attention_bf16 without one)");
  AttnParams p;
  p.Q = (const bf16_t*)q; p.K = (const bf16_t*)k; p.V = (const bf16_t*)v; p.O = (bf16_t*)out;
  p.B = B; p.H = H; p.S = S; p.D = D; p.ld = ld; p.ldo = ldo; p.scale = scale;
  p.bias = (const bf16_t*)bias; p.bias_head_stride = (long)bias_head_stride; p.ldb = ldb;
  return dk_launch_attention(p, g_attn_ws, S_(stream));
}
static int attn_params_from_desc(int dtype, const dk_attention_desc* d, AttnParams& p) {
  DK_REQUIRE(d != nullptr, "null descriptor");
  p.Q = (const bf16_t*)d->q; p.K = (const bf16_t*)d->k; p.V = (const bf16_t*)d->v; p.O = (bf16_t*)d->out;
  p.B = d->B; p.H = d->H; p.S = d->S; p.D = d->D; p.ld = d->ld; p.ldo = d->ldo; p.scale = d->scale;
  p.bias = (const bf16_t*)d->bias; p.bias_head_stride = (long)d->bias_head_stride; p.ldb = d->ldb;
  p.qn_a = (const bf16_t*)d->qn_a; p.qn_b = (const bf16_t*)d->qn_b; p.qn_split = d->qn_split; p.qn_eps = d->qn_eps; p.q_rope = d->q_rope;
  p.score_bound = d->score_bound;
  p.dtype = dtype;
  if (d->O8 != nullptr) {
    DK_REQUIRE(d->O8_scales != nullptr && d->o8_rows >= (int64_t)d->B * d->S && d->o8_ld >= d->H * d->D && d->o8_ld % 32 == 0,
               "MX-fp8 output copy: scales, B * S rows inside the buffer, a row pitch of at least H * D bytes (multiple of 32)");
    p.O8 = (unsigned char*)d->O8; p.O8_scales = (unsigned char*)d->O8_scales; p.o8_ld = d->o8_ld; p.o8_nblk = mx_nblk((long)d->o8_rows);
  }
  return 0;
}
static int attention_desc(int dtype, const dk_attention_desc* d, void* stream) {
  AttnParams p;
  if (const int rc = attn_params_from_desc(dtype, d, p)) return rc;
  return dk_launch_attention(p, g_attn_ws, S_(stream));
}
extern "C" int dk_attention_desc_bf16(const dk_attention_desc* d, void* stream) { return attention_desc(DK_DTYPE_BF16, d, stream); }
extern "C" int dk_attention_desc_f16(const dk_attention_desc* d, void* stream) { return attention_desc(DK_DTYPE_F16, d, stream); }
// the route of that call with a region of workspace_bytes bytes; plan->o8_split is read (dk_hip.h), every other field written
static int attention_plan(int dtype, const dk_attention_desc* d, size_t workspace_bytes, dk_attention_plan_t* plan) {
  DK_REQUIRE(plan != nullptr, "null plan");
  AttnParams p;
  if (const int rc = attn_params_from_desc(dtype, d, p)) return rc;
  if (p.O8 != nullptr) {
    p.o8_split = plan->o8_split;
    p.o8_txt_row0 = p.B * (p.S - p.o8_split);  // (the text rows right behind the image rows)
  }
  AttnRoute r;
  if (const int rc = dk_attention_route(p, workspace_bytes, dk_device_cu_count(), r)) return rc;
  *plan = dk_attention_plan_t{r.kernel, r.qfuse, r.blocks, r.whole, r.split, r.jobs, r.jobs > 0, r.quantize, r.launches, r.n_cu, p.o8_split, r.untracked};
  return 0;
}
extern "C" int dk_attention_plan(const dk_attention_desc* d, size_t workspace_bytes, dk_attention_plan_t* plan) {
  return attention_plan(DK_DTYPE_BF16, d, workspace_bytes, plan);
}
extern "C" int dk_attention_plan_f16(const dk_attention_desc* d, size_t workspace_bytes, dk_attention_plan_t* plan) {
  return attention_plan(DK_DTYPE_F16, d, workspace_bytes, plan);
}
// identity attention (include/dk_hip.h): the descriptor's launch with AttnParams::ident_from set; every check is dk_attention_route's
static int attention_identity(int dtype, const dk_attention_desc* d, int32_t ident_from, void* stream, dk_attention_plan_t* plan) {
  AttnParams p;
  if (const int rc = attn_params_from_desc(dtype, d, p)) return rc;
  DK_REQUIRE(ident_from != 0, "identity attention: 1 <= ident_from < S");  // (0 is the plain launch's value of the field)
  p.ident_from = ident_from;
  if (plan == nullptr) return dk_launch_attention(p, g_attn_ws, S_(stream));
  AttnRoute r;
  if (const int rc = dk_attention_route(p, 0, dk_device_cu_count(), r)) return rc;
  *plan = dk_attention_plan_t{r.kernel, r.qfuse, r.blocks, r.whole, r.split, r.jobs, r.jobs > 0, r.quantize, r.launches, r.n_cu, 0, r.untracked};
  return 0;
}
extern "C" int dk_attention_identity_bf16(const dk_attention_desc* d, int32_t ident_from, void* stream) {
  return attention_identity(DK_DTYPE_BF16, d, ident_from, stream, nullptr);
}
extern "C" int dk_attention_identity_f16(const dk_attention_desc* d, int32_t ident_from, void* stream) {
  return attention_identity(DK_DTYPE_F16, d, ident_from, stream, nullptr);
}
extern "C" int dk_attention_identity_plan(const dk_attention_desc* d, int32_t ident_from, int32_t f16, dk_attention_plan_t* plan) {
  DK_REQUIRE(plan != nullptr, "null plan");
  return attention_identity(f16 ? DK_DTYPE_F16 : DK_DTYPE_BF16, d, ident_from, nullptr, plan);
}
extern "C" int32_t dk_attention_d512_tp(int32_t T) { return (int32_t)align_up((size_t)(T > 0 ? T : 0), 64); }
int attention_d512(int dtype, const bf16_t* q, const bf16_t* k, const bf16_t* v, bf16_t* out, int B, int T, int ld, int ldo, float scale,
                   bf16_t* vt, hipStream_t st) {  // (dk_engine.h)
  DK_REQUIRE(ld == 512, "attention_d512: q / k / v rows of exactly 512 columns (the transpose reads dense [T, 512] matrices)");
  const int Tp = dk_attention_d512_tp(T);
  for (int b = 0; b < B; ++b) {
    const int rc = DK_EL(dtype, dk_launch_transpose)(v + (size_t)b * T * ld, vt + (size_t)b * 512 * Tp, T, 512, st, Tp);
    if (rc) return rc;
  }
  Attn512Params a;
  a.Q = q; a.K = k; a.Vt = vt; a.O = out; a.T = T; a.Tp = Tp; a.B = B; a.ld = ld; a.ldo = ldo; a.scale = scale; a.dtype = dtype;
  return dk_launch_attention512(a, st);
}
static int attention_d512_checked(int dtype, const void* q, const void* k, const void* v, void* out, int B, int T, int ld, int ldo, float scale,
                                  void* vt_scratch, void* stream) {
  DK_REQUIRE(q && k && v && out && vt_scratch && B > 0 && T > 0, "null / empty argument");
  return attention_d512(dtype, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, B, T, ld, ldo, scale, (bf16_t*)vt_scratch,
                        S_(stream));
}
extern "C" int dk_attention_d512_bf16(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t T, int32_t ld, int32_t ldo,
                                      float scale, void* vt_scratch, void* stream) {
  return attention_d512_checked(DK_DTYPE_BF16, q, k, v, out, B, T, ld, ldo, scale, vt_scratch, stream);
}
extern "C" int dk_attention_d512_f16(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t T, int32_t ld, int32_t ldo,
                                     float scale, void* vt_scratch, void* stream) {
  return attention_d512_checked(DK_DTYPE_F16, q, k, v, out, B, T, ld, ldo, scale, vt_scratch, stream);
}
extern "C" int dk_embedding_bf16(const void* table, const int32_t* ids, const void* pos, int32_t pos_rows, void* out_bf16, float* out_f32,
                                 int32_t n, int32_t dim, int32_t vocab, void* stream) {
  DK_REQUIRE(table && ids && (out_bf16 || out_f32), "null argument");
  return dk_launch_embedding((const bf16_t*)table, ids, (const bf16_t*)pos, pos_rows, (bf16_t*)out_bf16, out_f32, n, dim, vocab, S_(stream));
}
extern "C" int dk_layernorm_bf16(const void* x, void* out, int32_t M, int32_t h, const void* weight, const void* bias, float eps,
                                 void* stream) {
  DK_REQUIRE(x && out && weight && M > 0 && h > 0, "bad argument");
  return dk_launch_layernorm((const bf16_t*)x, (bf16_t*)out, M, h, (const bf16_t*)weight, (const bf16_t*)bias, eps, S_(stream));
}
extern "C" int dk_t5_rmsnorm_bf16(const float* x, void* out, int32_t M, int32_t h, const void* weight, float eps, void* stream) {
  DK_REQUIRE(x && out && weight && M > 0 && h > 0, "bad argument");
  return dk_launch_t5_rmsnorm(x, (bf16_t*)out, M, h, (const bf16_t*)weight, eps, S_(stream));
}
extern "C" int dk_text_elementwise(const void* a, const void* b, void* y, float* r, int64_t n, int32_t op, void* stream) {
  DK_REQUIRE(a && n > 0 && op >= 0 && op <= 2 && (op == 2 ? r != nullptr : y != nullptr) && (op != 1 || b != nullptr), "bad argument");
  return dk_launch_text_elementwise((const bf16_t*)a, (const bf16_t*)b, (bf16_t*)y, r, (long)n, op, S_(stream));
}
extern "C" int dk_t5_bias_bf16(const void* emb, const int32_t* rel_bucket, int32_t H, int32_t S, int32_t ld, void* out, void* stream) {
  DK_REQUIRE(emb && rel_bucket && out && H > 0 && S > 0 && ld >= S && ld % 64 == 0, "bad argument");
  return dk_launch_t5_bias((const bf16_t*)emb, rel_bucket, H, S, ld, (bf16_t*)out, S_(stream));
}

static int ln_modulate(int dtype, const void* x, int ldx, void* out, int ldo, int M, int h, const void* shift, const void* scale, int mod_stride,
                       int mod_seg_len, int x_seg_len, int x_seg_stride, float eps, void* stream) {
  return DK_EL(dtype, dk_launch_ln_modulate)((const bf16_t*)x, ldx, (bf16_t*)out, ldo, M, h, (const bf16_t*)shift, (const bf16_t*)scale,
                                             mod_stride, mod_seg_len > 0 ? mod_seg_len : M, x_seg_len > 0 ? x_seg_len : M, x_seg_stride,
                                             eps, S_(stream));
}
extern "C" int dk_ln_modulate_bf16(const void* x, int32_t ldx, void* out, int32_t ldo, int32_t M, int32_t h, const void* shift,
                                   const void* scale, int32_t mod_stride, int32_t mod_seg_len, int32_t x_seg_len,
                                   int32_t x_seg_stride, float eps, void* stream) {
  return ln_modulate(DK_DTYPE_BF16, x, ldx, out, ldo, M, h, shift, scale, mod_stride, mod_seg_len, x_seg_len, x_seg_stride, eps, stream);
}
extern "C" int dk_ln_modulate_f16(const void* x, int32_t ldx, void* out, int32_t ldo, int32_t M, int32_t h, const void* shift,
                                  const void* scale, int32_t mod_stride, int32_t mod_seg_len, int32_t x_seg_len,
                                  int32_t x_seg_stride, float eps, void* stream) {
  return ln_modulate(DK_DTYPE_F16, x, ldx, out, ldo, M, h, shift, scale, mod_stride, mod_seg_len, x_seg_len, x_seg_stride, eps, stream);
}

static int ln_modulate_dual(int dtype, const void* x, void* out_a, void* out_b, int M, const void* shift_a, const void* scale_a, const void* shift_b,
                            const void* scale_b, int seg, const void* x1, void* out1, int M1, const void* shift1, const void* scale1, int seg1, int ldx,
                            int ldo, int h, int mod_stride, int x_seg_stride, int x_seg_stride1, float eps, void* stream) {
  DK_REQUIRE(M > 0 && M1 >= 0 && h > 0, "bad argument");
  return DK_EL(dtype, dk_launch_ln_modulate2x)((const bf16_t*)x, (bf16_t*)out_a, (bf16_t*)out_b, M, (const bf16_t*)shift_a, (const bf16_t*)scale_a,
                                               (const bf16_t*)shift_b, (const bf16_t*)scale_b, seg > 0 ? seg : M, (const bf16_t*)x1, (bf16_t*)out1, M1,
                                               (const bf16_t*)shift1, (const bf16_t*)scale1, seg1 > 0 ? seg1 : (M1 > 0 ? M1 : 1), ldx, ldo, h, mod_stride,
                                               x_seg_stride, x_seg_stride1, eps, S_(stream));
}
extern "C" int dk_ln_modulate_dual_bf16(const void* x, void* out_a, void* out_b, int32_t M, const void* shift_a, const void* scale_a,
                                        const void* shift_b, const void* scale_b, int32_t mod_seg_len, const void* x1, void* out1, int32_t M1,
                                        const void* shift1, const void* scale1, int32_t mod_seg_len1, int32_t ldx, int32_t ldo, int32_t h,
                                        int32_t mod_stride, int32_t x_seg_stride, int32_t x_seg_stride1, float eps, void* stream) {
  return ln_modulate_dual(DK_DTYPE_BF16, x, out_a, out_b, M, shift_a, scale_a, shift_b, scale_b, mod_seg_len, x1, out1, M1, shift1, scale1, mod_seg_len1,
                          ldx, ldo, h, mod_stride, x_seg_stride, x_seg_stride1, eps, stream);
}
extern "C" int dk_ln_modulate_dual_f16(const void* x, void* out_a, void* out_b, int32_t M, const void* shift_a, const void* scale_a,
                                       const void* shift_b, const void* scale_b, int32_t mod_seg_len, const void* x1, void* out1, int32_t M1,
                                       const void* shift1, const void* scale1, int32_t mod_seg_len1, int32_t ldx, int32_t ldo, int32_t h,
                                       int32_t mod_stride, int32_t x_seg_stride, int32_t x_seg_stride1, float eps, void* stream) {
  return ln_modulate_dual(DK_DTYPE_F16, x, out_a, out_b, M, shift_a, scale_a, shift_b, scale_b, mod_seg_len, x1, out1, M1, shift1, scale1, mod_seg_len1,
                          ldx, ldo, h, mod_stride, x_seg_stride, x_seg_stride1, eps, stream);
}

static int ln_modulate_add(int dtype, void* x, const void* tap, int ldt, float s, void* out, int M, const void* shift, const void* scale, int seg,
                           const void* x1, void* out1, int M1, const void* shift1, const void* scale1, int seg1, int ldx, int ldo, int h,
                           int mod_stride, int x_seg_stride, int x_seg_stride1, float eps, void* stream) {
  DK_REQUIRE(M > 0 && M1 >= 0 && h > 0, "bad argument");
  return DK_EL(dtype, dk_launch_ln_modulate2_add)((bf16_t*)x, (const bf16_t*)tap, ldt, s, (bf16_t*)out, M, (const bf16_t*)shift, (const bf16_t*)scale,
                                                  seg > 0 ? seg : M, (const bf16_t*)x1, (bf16_t*)out1, M1, (const bf16_t*)shift1, (const bf16_t*)scale1,
                                                  seg1 > 0 ? seg1 : (M1 > 0 ? M1 : 1), ldx, ldo, h, mod_stride, x_seg_stride, x_seg_stride1, eps,
                                                  S_(stream));
}
extern "C" int dk_ln_modulate_add_bf16(void* x, const void* tap, int32_t ldt, float s, void* out, int32_t M, const void* shift, const void* scale,
                                       int32_t mod_seg_len, const void* x1, void* out1, int32_t M1, const void* shift1, const void* scale1,
                                       int32_t mod_seg_len1, int32_t ldx, int32_t ldo, int32_t h, int32_t mod_stride, int32_t x_seg_stride,
                                       int32_t x_seg_stride1, float eps, void* stream) {
  return ln_modulate_add(DK_DTYPE_BF16, x, tap, ldt, s, out, M, shift, scale, mod_seg_len, x1, out1, M1, shift1, scale1, mod_seg_len1, ldx, ldo, h,
                         mod_stride, x_seg_stride, x_seg_stride1, eps, stream);
}
extern "C" int dk_ln_modulate_add_f16(void* x, const void* tap, int32_t ldt, float s, void* out, int32_t M, const void* shift, const void* scale,
                                      int32_t mod_seg_len, const void* x1, void* out1, int32_t M1, const void* shift1, const void* scale1,
                                      int32_t mod_seg_len1, int32_t ldx, int32_t ldo, int32_t h, int32_t mod_stride, int32_t x_seg_stride,
                                      int32_t x_seg_stride1, float eps, void* stream) {
  return ln_modulate_add(DK_DTYPE_F16, x, tap, ldt, s, out, M, shift, scale, mod_seg_len, x1, out1, M1, shift1, scale1, mod_seg_len1, ldx, ldo, h,
                         mod_stride, x_seg_stride, x_seg_stride1, eps, stream);
}

extern "C" int dk_ln_modulate_add_joint_bf16(void* x, int32_t ldx, const void* tap, int32_t ldt, float s, int32_t tap_seg, int32_t tap_first, void* out,
                                             int32_t ldo, int32_t M, int32_t h, const void* shift, const void* scale, int32_t mod_stride,
                                             int32_t mod_seg_len, int32_t x_seg_len, int32_t x_seg_stride, float eps, void* stream) {
  DK_REQUIRE(M > 0 && h > 0, "bad argument");
  return dk_launch_ln_modulate_add_joint((bf16_t*)x, ldx, (const bf16_t*)tap, ldt, s, tap_seg, tap_first, (bf16_t*)out, ldo, M, h, (const bf16_t*)shift,
                                         (const bf16_t*)scale, mod_stride, mod_seg_len > 0 ? mod_seg_len : M, x_seg_len > 0 ? x_seg_len : M, x_seg_stride,
                                         eps, S_(stream));
}

extern "C" int dk_ip_attention_bf16(const void* qkv, int32_t ldq, int32_t seg_len, int32_t seg_stride, int32_t first_row, const void* qn, const void* k,
                                    const void* v, int32_t ldkv, int32_t B, int32_t N, int32_t h, int32_t D, float scale, float eps, void* out,
                                    void* stream) {
  return dk_launch_ip_attention((const bf16_t*)qkv, ldq, seg_len, seg_stride, first_row, (const bf16_t*)qn, (const bf16_t*)k, (const bf16_t*)v, ldkv, B, N, h,
                                D, scale, eps, (bf16_t*)out, S_(stream));
}

static int block_probe(int dtype,const void* x, int ldx, int x_seg_len, int x_seg_stride, void* d, const void* d_ref, float* row_partials,
                       float* probe, int M, int h, int rows_per_batch, void* stream) {
  return DK_EL(dtype, dk_launch_block_probe)((const bf16_t*)x, ldx, x_seg_len, x_seg_stride, (bf16_t*)d, (const bf16_t*)d_ref, row_partials, probe, M, h,
                                             rows_per_batch, S_(stream));
}
extern "C" int dk_block_probe_bf16(const void* x, int32_t ldx, int32_t x_seg_len, int32_t x_seg_stride, void* d, const void* d_ref,
                                   float* row_partials, float* probe, int32_t M, int32_t h, int32_t rows_per_batch, void* stream) {
  return block_probe(DK_DTYPE_BF16, x, ldx, x_seg_len, x_seg_stride, d, d_ref, row_partials, probe, M, h, rows_per_batch, stream);
}
extern "C" int dk_block_probe_f16(const void* x, int32_t ldx, int32_t x_seg_len, int32_t x_seg_stride, void* d, const void* d_ref,
                                  float* row_partials, float* probe, int32_t M, int32_t h, int32_t rows_per_batch, void* stream) {
  return block_probe(DK_DTYPE_F16, x, ldx, x_seg_len, x_seg_stride, d, d_ref, row_partials, probe, M, h, rows_per_batch, stream);
}
static int block_residual(int dtype, void* x, int ldx, int x_seg_len, int x_seg_stride, void* r, int M, int h, int reuse, void* stream) {
  return DK_EL(dtype, dk_launch_block_residual)((bf16_t*)x, ldx, x_seg_len, x_seg_stride, (bf16_t*)r, M, h, reuse != 0, S_(stream));
}
extern "C" int dk_block_residual_bf16(void* x, int32_t ldx, int32_t x_seg_len, int32_t x_seg_stride, void* r, int32_t M, int32_t h,
                                      int32_t reuse, void* stream) {
  return block_residual(DK_DTYPE_BF16, x, ldx, x_seg_len, x_seg_stride, r, M, h, reuse, stream);
}
extern "C" int dk_block_residual_f16(void* x, int32_t ldx, int32_t x_seg_len, int32_t x_seg_stride, void* r, int32_t M, int32_t h,
                                     int32_t reuse, void* stream) {
  return block_residual(DK_DTYPE_F16, x, ldx, x_seg_len, x_seg_stride, r, M, h, reuse, stream);
}

// mx8_out: the descriptor's C_scales / c_rows / c_row0 / c_col0 describe an MX-fp8 output (its own, or the second one of a column split)
static int gemm_f8_params_from_desc(const dk_gemm_fp8_desc* d, bool mx8_out, GemmF8Params& p) {
  memset(&p, 0, sizeof(p));
  p.A = (const unsigned char*)d->A; p.SA = (const unsigned char*)d->A_scales; p.W = (const unsigned char*)d->W; p.wscale = d->w_scale;
  p.C = d->C; p.bias = (const bf16_t*)d->bias; p.gate = (const bf16_t*)d->gate; p.res = (const bf16_t*)d->res;
  p.M = d->M; p.N = d->N; p.K = d->K; p.lda = d->lda; p.ldw = d->ldw; p.ldc = d->ldc; p.ldr = d->ldr;
  p.a_seg_len = d->a_seg_len > 0 ? d->a_seg_len : (d->M + 127) / 128 * 128; p.a_seg_stride = d->a_seg_stride; p.a_row0 = d->a_row0;
  p.sa_nblk = mx_nblk(d->a_rows);
  p.c_seg_len = d->c_seg_len > 0 ? d->c_seg_len : d->M; p.c_seg_stride = d->c_seg_stride;
  p.r_seg_len = d->r_seg_len > 0 ? d->r_seg_len : d->M; p.r_seg_stride = d->r_seg_stride;
  p.gate_seg_len = d->gate_seg_len > 0 ? d->gate_seg_len : d->M; p.gate_stride = d->gate_stride;
  p.epi = d->epilogue; p.c_mx8 = d->c_mx8;
  if (mx8_out) {
    DK_REQUIRE(d->c_col0 % 32 == 0 && d->C_scales != nullptr, "MX-fp8 output: scales, column offset a multiple of 32");
    p.SC = (unsigned char*)d->C_scales; p.sc_nblk = mx_nblk(d->c_rows); p.c_row0 = d->c_row0; p.sc_kb0 = d->c_col0 / 32;
  }
  p.workspace = d->workspace; p.workspace_bytes = d->workspace_bytes;
  return 0;
}

extern "C" int dk_gemm_fp8(const dk_gemm_fp8_desc* d, void* stream) {
  DK_REQUIRE(d != nullptr, "null descriptor");
  GemmF8Params p;
  if (const int rc = gemm_f8_params_from_desc(d, d->c_mx8 != 0, p)) return rc;
  return dk_launch_gemm256f8(p, nullptr, S_(stream));
}

extern "C" int dk_gemm_fp8_fused(const dk_gemm_fp8_desc* d, const dk_gemm_fp8_side* f, const dk_gemm_fp8_desc* d2, const dk_gemm_fp8_side* f2,
                                 void* stream) {
  DK_REQUIRE(d != nullptr && (d2 != nullptr || f2 == nullptr), "null descriptor");
  GemmF8Params p, p2;
  if (const int rc = gemm_f8_params_from_desc(d, d->c_mx8 != 0 || (f != nullptr && f->c2_mx8 != 0), p)) return rc;
  set_fused(p, f);
  if (f != nullptr) p.c2_mx8 = f->c2_mx8;
  if (d2 == nullptr) return dk_launch_gemm256f8(p, nullptr, S_(stream));
  if (const int rc = gemm_f8_params_from_desc(d2, d2->c_mx8 != 0 || (f2 != nullptr && f2->c2_mx8 != 0), p2)) return rc;
  set_fused(p2, f2);
  if (f2 != nullptr) p2.c2_mx8 = f2->c2_mx8;
  return dk_launch_gemm256f8(p, &p2, S_(stream));
}
extern "C" int dk_quantize_mx8(const void* x, int32_t ldx, int32_t M, int32_t h, void* out, int32_t ldo, void* out_scales, int64_t out_rows,
                               int32_t out_row0, int32_t out_col0, void* stream) {
  DK_REQUIRE(x && out && out_scales && M > 0, "bad argument");
  DK_REQUIRE(out_row0 >= 0 && (int64_t)out_row0 + M <= out_rows, "rows [out_row0, out_row0 + M) must lie inside the [out_rows, ldo] output");
  DK_REQUIRE(out_col0 >= 0 && ldo >= out_col0 + h, "columns [out_col0, out_col0 + h) must lie inside a row of ldo bytes");
  return dk_launch_quantize_mx8((const bf16_t*)x, ldx, M, 0, M, h, mx8_out(out, out_scales, ldo, (long)out_rows, out_row0, M, 0, out_col0), S_(stream));
}
extern "C" int dk_ln_modulate_mx8(const void* x, int32_t ldx, int32_t M, int32_t h, const void* shift, const void* scale, int32_t mod_stride,
                                  int32_t mod_seg_len, float eps, void* out, int32_t ldo, void* out_scales, int64_t out_rows,
                                  int32_t out_row0, void* stream) {
  DK_REQUIRE(x && out && out_scales && M > 0, "bad argument");
  DK_REQUIRE(out_row0 >= 0 && (int64_t)out_row0 + M <= out_rows, "rows [out_row0, out_row0 + M) must lie inside the [out_rows, ldo] output");
  DK_REQUIRE(ldo >= h, "a row of the output holds h bytes");
  return dk_launch_ln_modulate_mx8((const bf16_t*)x, ldx, M, h, (const bf16_t*)shift, (const bf16_t*)scale, mod_stride,
                                   mod_seg_len > 0 ? mod_seg_len : M, M, 0, eps, mx8_out(out, out_scales, ldo, (long)out_rows, out_row0, M, 0, 0),
                                   S_(stream));
}

static int qk_norm_rope(int dtype, void* qkv, int ld, int q_off, int k_off, int rows, int H, int D, const void* q_weight, const void* k_weight,
                        float eps, const float* rope_table, int row_seg_len, int row_seg_stride, int pos_off, void* stream) {
  return DK_EL(dtype, dk_launch_qk_norm_rope)((bf16_t*)qkv, ld, q_off, k_off, rows, H, D, (const bf16_t*)q_weight, (const bf16_t*)k_weight, eps,
                                              rope_table, row_seg_len > 0 ? row_seg_len : rows, row_seg_stride, pos_off, 0, S_(stream), 0);
}
extern "C" int dk_qk_norm_rope_bf16(void* qkv, int32_t ld, int32_t q_off, int32_t k_off, int32_t rows, int32_t H, int32_t D,
                                    const void* q_weight, const void* k_weight, float eps, const float* rope_table,
                                    int32_t row_seg_len, int32_t row_seg_stride, int32_t pos_off, void* stream) {
  return qk_norm_rope(DK_DTYPE_BF16, qkv, ld, q_off, k_off, rows, H, D, q_weight, k_weight, eps, rope_table, row_seg_len, row_seg_stride, pos_off, stream);
}
extern "C" int dk_qk_norm_rope_f16(void* qkv, int32_t ld, int32_t q_off, int32_t k_off, int32_t rows, int32_t H, int32_t D,
                                   const void* q_weight, const void* k_weight, float eps, const float* rope_table,
                                   int32_t row_seg_len, int32_t row_seg_stride, int32_t pos_off, void* stream) {
  return qk_norm_rope(DK_DTYPE_F16, qkv, ld, q_off, k_off, rows, H, D, q_weight, k_weight, eps, rope_table, row_seg_len, row_seg_stride, pos_off, stream);
}

extern "C" int dk_rope_table_f32(float* table, int32_t S_txt, int32_t gh, int32_t gw, const int32_t* axes_dim, int32_t n_axes,
                                 float theta, void* stream) {
  return dk_launch_rope_table(table, S_txt, gh, gw, axes_dim, n_axes, theta, S_(stream));
}
extern "C" int dk_rope_table_segments_f32(float* table, int32_t S_txt, int32_t n_seg, const int32_t* seg, const int32_t* axes_dim,
                                          int32_t n_axes, float theta, void* stream) {
  return dk_launch_rope_table_segments(table, S_txt, n_seg, seg, axes_dim, n_axes, theta, S_(stream));
}

static int timestep_embedding(int dtype, const float* t_dev, int n, int dim, float max_period, int embed_dtype, void* out, void* stream) {
  return DK_EL(dtype, dk_launch_timestep_embedding)(t_dev, n, 1, dim, max_period, embed_dtype, (bf16_t*)out, S_(stream));
}
extern "C" int dk_timestep_embedding_bf16(const float* t_dev, int32_t n, int32_t dim, float max_period, int32_t embed_dtype,
                                          void* out, void* stream) {
  return timestep_embedding(DK_DTYPE_BF16, t_dev, n, dim, max_period, embed_dtype, out, stream);
}
extern "C" int dk_timestep_embedding_f16(const float* t_dev, int32_t n, int32_t dim, float max_period, int32_t embed_dtype,
                                         void* out, void* stream) {
  return timestep_embedding(DK_DTYPE_F16, t_dev, n, dim, max_period, embed_dtype, out, stream);
}

static int latent_to_tokens(int dtype, const float* x, void* tokens, int n_img, int dup, int Hl, int Wl, int C, int p, int reshape_order,
                            void* stream) {
  DK_REQUIRE(Hl % p == 0 && Wl % p == 0, "latent size must be divisible by the patch size");
  return DK_EL(dtype, dk_launch_latent_to_tokens)(x, (bf16_t*)tokens, n_img, dup, Hl, Wl, C, p, reshape_order, S_(stream));
}
extern "C" int dk_latent_to_tokens(const float* x, void* tokens, int32_t n_img, int32_t dup, int32_t Hl, int32_t Wl, int32_t C,
                                   int32_t p, int32_t reshape_order, void* stream) {
  return latent_to_tokens(DK_DTYPE_BF16, x, tokens, n_img, dup, Hl, Wl, C, p, reshape_order, stream);
}
extern "C" int dk_latent_to_tokens_f16(const float* x, void* tokens, int32_t n_img, int32_t dup, int32_t Hl, int32_t Wl, int32_t C,
                                       int32_t p, int32_t reshape_order, void* stream) {
  return latent_to_tokens(DK_DTYPE_F16, x, tokens, n_img, dup, Hl, Wl, C, p, reshape_order, stream);
}

// ---- the step tail: fourteen entries (Euler, coefficient row, guided, skip-layer, noisy; plain and masked; bf16 and fp16) over one parameter block, one check, one launcher
// Every requirement of a step launch.  The guided entries' own come first, then the common ones, so that a call that breaks one rule is told what it
// always was; the structured binding gives the fields the names the messages quote.
static int check_step(const StepParams& s) {
  const auto& [x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl, C, p, reshape_order, sigma, sigma_next, cfg_weight, has_row, cx, cd, ch, hx, hd,
               hist, reads_h, writes_h, masked, x_orig, noise, mask, mask_per_image, guided, mode, phi, eta, r, beta, m, reads_m, writes_m, workspace,
               workspace_bytes, slg, slg_scale, noisy, cn, seeds, draw] = s;
  if (noisy) {
    DK_REQUIRE(std::isfinite(cn), "cn must be finite");
    DK_REQUIRE(seeds || cn == 0.0f, "seeds is null while the row carries a noise term (cn != 0)");
    DK_REQUIRE(draw >= 0 || cn == 0.0f, "draw must not be negative where the row carries a noise term (cn != 0)");
    DK_REQUIRE(((long)Hl * Wl * C) % 4 == 0, "the latent of one image must hold a multiple of 4 elements (Hl * Wl * C % 4 == 0): a Philox block is four normals");
  }
  if (slg) {
    DK_REQUIRE(cfg_on != 0, "skip-layer guidance adds its term to a guided prediction: cfg_on must be set");
    DK_REQUIRE(std::isfinite(slg_scale), "slg_scale must be finite");
  }
  if (guided) {
    DK_REQUIRE(cfg_on != 0, "guidance modes combine two predictions: cfg_on must be set (an unguided row is dk_lms_cfg_step with cfg_on = 0)");
    DK_REQUIRE(mode >= 0 && mode <= 2, "unknown guidance mode (0 cfg, 1 rescale, 2 apg)");
    DK_REQUIRE(std::isfinite(phi) && std::isfinite(eta) && std::isfinite(r) && std::isfinite(beta) && std::isfinite(cfg_weight),
               "the guidance parameters must be finite");
    DK_REQUIRE(phi >= 0.0f && phi <= 1.0f, "the rescale factor phi must lie in [0, 1]");
    DK_REQUIRE(C > 0 && Hl > 0 && Wl > 0, "the latent size must be positive");
  }
  DK_REQUIRE(sigma != 0.0f, "sigma must be non-zero");
  DK_REQUIRE(p > 0 && Hl % p == 0 && Wl % p == 0, "latent size must be divisible by the patch size");
  if (!has_row && masked) DK_REQUIRE(x && model_out && tokens && x_orig && noise && mask, "null argument");  // (dk_euler_cfg_step_masked's wording)
  DK_REQUIRE(x && model_out && tokens, "null argument");
  DK_REQUIRE(n_img > 0, "n_img must be positive");
  if (has_row) {
    DK_REQUIRE(hist || !(reads_h || writes_h), "hist is null while the row reads or writes the history");
    const float coef[5] = {cx, cd, ch, hx, hd};
    for (float v : coef) DK_REQUIRE(std::isfinite(v), "the coefficients of the row must be finite");
    DK_REQUIRE(std::isfinite(sigma) && std::isfinite(sigma_next), "sigma and sigma_next must be finite");
  }
  if (masked) DK_REQUIRE(x_orig && noise && mask, "null argument");
  if (mode != 0) {
    DK_REQUIRE(m || !(reads_m || writes_m), "the momentum buffer M is null while the row reads or writes it");
    DK_REQUIRE(workspace && workspace_bytes >= dk_guidance_workspace_size(n_img, Hl, Wl, C),
               "the guidance workspace is null or shorter than dk_guidance_workspace_bytes");
  }
  return 0;
}
static int step(int dtype, const StepParams& s, void* stream) {
  const int rc = check_step(s);
  return rc ? rc : DK_EL(dtype, dk_launch_step)(s, S_(stream));
}
// the fields the entries' arguments name, group by group (StepParams, dk_elem_launchers.h); whatever an entry does not name stays zero
static StepParams step_operands(float* x, const void* model_out, int ld_out, void* tokens, int n_img, int cfg_on, int Hl, int Wl, int C, int p,
                                int reshape_order, float sigma, float sigma_next, float cfg_weight) {
  StepParams s = {};
  s.x = x, s.model_out = (const bf16_t*)model_out, s.ld_out = ld_out, s.tok = (bf16_t*)tokens, s.n_img = n_img, s.cfg_on = cfg_on;
  s.Hl = Hl, s.Wl = Wl, s.C = C, s.p = p, s.reshape_order = reshape_order, s.sigma = sigma, s.sigma_next = sigma_next, s.cfg_weight = cfg_weight;
  return s;
}
static StepParams with_row(StepParams s, float* hist, float cx, float cd, float ch, float hx, float hd, int reads_h, int writes_h) {
  s.has_row = true, s.hist = hist, s.cx = cx, s.cd = cd, s.ch = ch, s.hx = hx, s.hd = hd, s.reads_h = reads_h != 0, s.writes_h = writes_h != 0;
  return s;
}
static StepParams with_blend(StepParams s, bool masked, const float* x_orig, const float* noise, const float* mask, int mask_per_image) {
  s.masked = masked, s.x_orig = x_orig, s.noise = noise, s.mask = mask, s.mask_per_image = mask_per_image != 0;
  return s;
}
// (the momentum flags count under APG alone)
static StepParams with_guidance(StepParams s, int mode, float phi, float eta, float r, float beta, int reads_m, int writes_m, float* m, void* workspace,
                                size_t workspace_bytes) {
  s.guided = true, s.mode = mode, s.phi = phi, s.eta = eta, s.r = r, s.beta = beta, s.m = m, s.workspace = workspace, s.workspace_bytes = workspace_bytes;
  s.reads_m = mode == 2 && reads_m != 0, s.writes_m = mode == 2 && writes_m != 0;
  return s;
}
extern "C" int dk_euler_cfg_step(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on,
                                 int32_t Hl, int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma,
                                 float sigma_next, float cfg_weight, void* stream) {
  return step(DK_DTYPE_BF16, step_operands(x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl, C, p, reshape_order, sigma, sigma_next, cfg_weight),
              stream);
}
extern "C" int dk_euler_cfg_step_f16(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on,
                                     int32_t Hl, int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma,
                                     float sigma_next, float cfg_weight, void* stream) {
  return step(DK_DTYPE_F16, step_operands(x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl, C, p, reshape_order, sigma, sigma_next, cfg_weight),
              stream);
}
extern "C" int dk_euler_cfg_step_masked(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on,
                                        int32_t Hl, int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma,
                                        float sigma_next, float cfg_weight, const float* x_orig, const float* noise, const float* mask,
                                        int32_t mask_per_image, void* stream) {
  const StepParams s = step_operands(x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl, C, p, reshape_order, sigma, sigma_next, cfg_weight);
  return step(DK_DTYPE_BF16, with_blend(s, true, x_orig, noise, mask, mask_per_image), stream);
}
extern "C" int dk_euler_cfg_step_masked_f16(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on,
                                            int32_t Hl, int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma,
                                            float sigma_next, float cfg_weight, const float* x_orig, const float* noise,
                                            const float* mask, int32_t mask_per_image, void* stream) {
  const StepParams s = step_operands(x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl, C, p, reshape_order, sigma, sigma_next, cfg_weight);
  return step(DK_DTYPE_F16, with_blend(s, true, x_orig, noise, mask, mask_per_image), stream);
}

// second-order samplers: the step as a coefficient row (x' = cx x + cd d + ch H, H' = hx x + hd d); masked = the inpainting blend behind it
extern "C" int dk_lms_cfg_step(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on, int32_t Hl, int32_t Wl,
                               int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight, float* hist, float cx, float cd,
                               float ch, float hx, float hd, float sigma_next, int32_t reads_h, int32_t writes_h, void* stream) {
  const StepParams s = step_operands(x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl, C, p, reshape_order, sigma, sigma_next, cfg_weight);
  return step(DK_DTYPE_BF16, with_row(s, hist, cx, cd, ch, hx, hd, reads_h, writes_h), stream);
}
extern "C" int dk_lms_cfg_step_f16(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on, int32_t Hl,
                                   int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight, float* hist, float cx,
                                   float cd, float ch, float hx, float hd, float sigma_next, int32_t reads_h, int32_t writes_h, void* stream) {
  const StepParams s = step_operands(x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl, C, p, reshape_order, sigma, sigma_next, cfg_weight);
  return step(DK_DTYPE_F16, with_row(s, hist, cx, cd, ch, hx, hd, reads_h, writes_h), stream);
}
extern "C" int dk_lms_cfg_step_masked(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on, int32_t Hl,
                                      int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight, float* hist,
                                      float cx, float cd, float ch, float hx, float hd, float sigma_next, int32_t reads_h, int32_t writes_h,
                                      const float* x_orig, const float* noise, const float* mask, int32_t mask_per_image, void* stream) {
  const StepParams s = step_operands(x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl, C, p, reshape_order, sigma, sigma_next, cfg_weight);
  return step(DK_DTYPE_BF16, with_blend(with_row(s, hist, cx, cd, ch, hx, hd, reads_h, writes_h), true, x_orig, noise, mask, mask_per_image), stream);
}
extern "C" int dk_lms_cfg_step_masked_f16(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on, int32_t Hl,
                                          int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight, float* hist,
                                          float cx, float cd, float ch, float hx, float hd, float sigma_next, int32_t reads_h, int32_t writes_h,
                                          const float* x_orig, const float* noise, const float* mask, int32_t mask_per_image, void* stream) {
  const StepParams s = step_operands(x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl, C, p, reshape_order, sigma, sigma_next, cfg_weight);
  return step(DK_DTYPE_F16, with_blend(with_row(s, hist, cx, cd, ch, hx, hd, reads_h, writes_h), true, x_orig, noise, mask, mask_per_image), stream);
}

// guidance modes: the coefficient-row step behind the per-image moments of the two predictions (mode 0: dk_lms_cfg_step itself); masked iff a
// mask operand is given
extern "C" size_t dk_guidance_workspace_bytes(int32_t n_img, int32_t Hl, int32_t Wl, int32_t C) {
  if (n_img <= 0 || Hl <= 0 || Wl <= 0 || C <= 0) return 0;
  return dk_guidance_workspace_size(n_img, Hl, Wl, C);
}
extern "C" int dk_guided_cfg_step(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on, int32_t Hl, int32_t Wl,
                                  int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight, float* hist, float cx, float cd,
                                  float ch, float hx, float hd, float sigma_next, int32_t reads_h, int32_t writes_h, const float* x_orig,
                                  const float* noise, const float* mask, int32_t mask_per_image, int32_t mode, float phi, float eta, float r,
                                  float beta, int32_t reads_m, int32_t writes_m, float* m, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  const StepParams s = step_operands(x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl, C, p, reshape_order, sigma, sigma_next, cfg_weight);
  const StepParams b = with_blend(with_row(s, hist, cx, cd, ch, hx, hd, reads_h, writes_h), x_orig || noise || mask, x_orig, noise, mask, mask_per_image);
  return step(DK_DTYPE_BF16, with_guidance(b, mode, phi, eta, r, beta, reads_m, writes_m, m, workspace, workspace_bytes), stream);
}
extern "C" int dk_guided_cfg_step_f16(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on, int32_t Hl,
                                      int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight, float* hist, float cx,
                                      float cd, float ch, float hx, float hd, float sigma_next, int32_t reads_h, int32_t writes_h,
                                      const float* x_orig, const float* noise, const float* mask, int32_t mask_per_image, int32_t mode, float phi,
                                      float eta, float r, float beta, int32_t reads_m, int32_t writes_m, float* m, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  const StepParams s = step_operands(x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl, C, p, reshape_order, sigma, sigma_next, cfg_weight);
  const StepParams b = with_blend(with_row(s, hist, cx, cd, ch, hx, hd, reads_h, writes_h), x_orig || noise || mask, x_orig, noise, mask, mask_per_image);
  return step(DK_DTYPE_F16, with_guidance(b, mode, phi, eta, r, beta, reads_m, writes_m, m, workspace, workspace_bytes), stream);
}

// skip-layer guidance: the guided step on three row groups, den + slg_scale (c - k)
static StepParams with_skip_layers(StepParams s, float slg_scale) {
  s.slg = true, s.slg_scale = slg_scale;
  return s;
}
extern "C" int dk_slg_cfg_step(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on, int32_t Hl, int32_t Wl,
                               int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight, float* hist, float cx, float cd, float ch,
                               float hx, float hd, float sigma_next, int32_t reads_h, int32_t writes_h, const float* x_orig, const float* noise,
                               const float* mask, int32_t mask_per_image, int32_t mode, float phi, float eta, float r, float beta, int32_t reads_m,
                               int32_t writes_m, float* m, void* workspace, size_t workspace_bytes, float slg_scale, void* stream) {
  const StepParams s = step_operands(x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl, C, p, reshape_order, sigma, sigma_next, cfg_weight);
  const StepParams b = with_blend(with_row(s, hist, cx, cd, ch, hx, hd, reads_h, writes_h), x_orig || noise || mask, x_orig, noise, mask, mask_per_image);
  return step(DK_DTYPE_BF16, with_skip_layers(with_guidance(b, mode, phi, eta, r, beta, reads_m, writes_m, m, workspace, workspace_bytes), slg_scale),
              stream);
}
extern "C" int dk_slg_cfg_step_f16(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on, int32_t Hl,
                                   int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight, float* hist, float cx,
                                   float cd, float ch, float hx, float hd, float sigma_next, int32_t reads_h, int32_t writes_h, const float* x_orig,
                                   const float* noise, const float* mask, int32_t mask_per_image, int32_t mode, float phi, float eta, float r,
                                   float beta, int32_t reads_m, int32_t writes_m, float* m, void* workspace, size_t workspace_bytes, float slg_scale,
                                   void* stream) {
  const StepParams s = step_operands(x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl, C, p, reshape_order, sigma, sigma_next, cfg_weight);
  const StepParams b = with_blend(with_row(s, hist, cx, cd, ch, hx, hd, reads_h, writes_h), x_orig || noise || mask, x_orig, noise, mask, mask_per_image);
  return step(DK_DTYPE_F16, with_skip_layers(with_guidance(b, mode, phi, eta, r, beta, reads_m, writes_m, m, workspace, workspace_bytes), slg_scale),
              stream);
}

// stochastic samplers: dk_slg_cfg_step's row with the flags `guided` and `slg` spelled out (0: the group is left out, and an unguided row runs with
// cfg_on = 0) and one more term, cn xi(seeds[img], draw), drawn in the launch
static StepParams with_noise(StepParams s, float cn, const uint64_t* seeds, int draw) {
  s.noisy = true, s.cn = cn, s.seeds = (const unsigned long long*)seeds, s.draw = draw;
  return s;
}
static int noisy_step(int dtype, float* x, const void* model_out, int ld_out, void* tokens, int n_img, int cfg_on, int Hl, int Wl, int C, int p,
                      int reshape_order, float sigma, float cfg_weight, float* hist, float cx, float cd, float ch, float hx, float hd, float sigma_next,
                      int reads_h, int writes_h, const float* x_orig, const float* noise, const float* mask, int mask_per_image, int guided, int mode,
                      float phi, float eta, float r, float beta, int reads_m, int writes_m, float* m, void* workspace, size_t workspace_bytes, int slg,
                      float slg_scale, float cn, const uint64_t* seeds, int draw, void* stream) {
  DK_REQUIRE(guided != 0 || mode == 0, "a row without the guidance group (guided = 0) takes mode 0");
  const StepParams s = step_operands(x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl, C, p, reshape_order, sigma, sigma_next, cfg_weight);
  StepParams b = with_blend(with_row(s, hist, cx, cd, ch, hx, hd, reads_h, writes_h), x_orig || noise || mask, x_orig, noise, mask, mask_per_image);
  if (guided) b = with_guidance(b, mode, phi, eta, r, beta, reads_m, writes_m, m, workspace, workspace_bytes);
  if (slg) b = with_skip_layers(b, slg_scale);
  return step(dtype, with_noise(b, cn, seeds, draw), stream);
}
extern "C" int dk_noisy_cfg_step(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on, int32_t Hl, int32_t Wl,
                                 int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight, float* hist, float cx, float cd, float ch,
                                 float hx, float hd, float sigma_next, int32_t reads_h, int32_t writes_h, const float* x_orig, const float* noise,
                                 const float* mask, int32_t mask_per_image, int32_t mode, float phi, float eta, float r, float beta, int32_t reads_m,
                                 int32_t writes_m, float* m, void* workspace, size_t workspace_bytes, float slg_scale, int32_t guided, int32_t slg,
                                 float cn, const uint64_t* seeds, int32_t draw, void* stream) {
  return noisy_step(DK_DTYPE_BF16, x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl, C, p, reshape_order, sigma, cfg_weight, hist, cx, cd, ch, hx, hd,
                    sigma_next, reads_h, writes_h, x_orig, noise, mask, mask_per_image, guided, mode, phi, eta, r, beta, reads_m, writes_m, m, workspace,
                    workspace_bytes, slg, slg_scale, cn, seeds, draw, stream);
}
extern "C" int dk_noisy_cfg_step_f16(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on, int32_t Hl,
                                     int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight, float* hist, float cx,
                                     float cd, float ch, float hx, float hd, float sigma_next, int32_t reads_h, int32_t writes_h, const float* x_orig,
                                     const float* noise, const float* mask, int32_t mask_per_image, int32_t mode, float phi, float eta, float r,
                                     float beta, int32_t reads_m, int32_t writes_m, float* m, void* workspace, size_t workspace_bytes, float slg_scale,
                                     int32_t guided, int32_t slg, float cn, const uint64_t* seeds, int32_t draw, void* stream) {
  return noisy_step(DK_DTYPE_F16, x, model_out, ld_out, tokens, n_img, cfg_on, Hl, Wl, C, p, reshape_order, sigma, cfg_weight, hist, cx, cd, ch, hx, hd,
                    sigma_next, reads_h, writes_h, x_orig, noise, mask, mask_per_image, guided, mode, phi, eta, r, beta, reads_m, writes_m, m, workspace,
                    workspace_bytes, slg, slg_scale, cn, seeds, draw, stream);
}
// the generator where tests can reach it: out f32 [n_img, n_per_img], row j from seeds[j] (u64 on the device), quads quad_offset, quad_offset + 1, ...
extern "C" int dk_philox_normal_f32(float* out, const uint64_t* seeds, int32_t n_img, int64_t n_per_img, int32_t draw, int32_t stream_tag,
                                    uint64_t quad_offset, void* stream) {
  DK_REQUIRE(out && seeds, "null argument");
  DK_REQUIRE(n_img > 0 && n_per_img > 0, "n_img and n_per_img must be positive");
  DK_REQUIRE(n_per_img % 4 == 0, "n_per_img must be a multiple of 4: a Philox block is four normals");
  DK_REQUIRE(draw >= 0 && stream_tag >= 0, "draw and stream must not be negative");
  DK_REQUIRE(quad_offset <= ~0ull - (uint64_t)(n_per_img / 4), "quad_offset + n_per_img / 4 must stay below 2^64");
  return dk_launch_philox_normal(out, (const unsigned long long*)seeds, n_img, (long)n_per_img, (unsigned)draw, (unsigned)stream_tag,
                                 (unsigned long long)quad_offset, S_(stream));
}

// FlowEdit: the edit loop's step (elementwise.hip: dk_flowedit_step_kernel).  Every requirement of the launch, then the launcher of the element type.
static int flowedit_step(int dtype, float* z, const float* x_src, const void* model_out, int ld_out, void* tokens, float* zs_out, float* zt_out,
                         int n_img, int cfg_on, int Hl, int Wl, int C, int p, int reshape_order, float w_src, float w_tar, float c, float sigma_in,
                         const uint64_t* seeds, int draw, int prime, void* stream) {
  DK_REQUIRE(z && x_src && tokens && zt_out && seeds, "null argument (zs_out alone may be null)");
  DK_REQUIRE(model_out || prime, "model_out is null while the launch reads it (prime = 0)");
  DK_REQUIRE(n_img > 0 && Hl > 0 && Wl > 0 && C > 0, "n_img and the latent size must be positive");
  DK_REQUIRE(p > 0 && Hl % p == 0 && Wl % p == 0, "latent size must be divisible by the patch size");
  DK_REQUIRE(C % 4 == 0, "C must be a multiple of 4: a thread takes the four channels of one Philox block");
  DK_REQUIRE(prime || (ld_out >= p * p * C && ld_out % 4 == 0), "ld_out must be at least p * p * C and a multiple of 4");
  const uintptr_t f32s = (uintptr_t)z | (uintptr_t)x_src | (uintptr_t)zs_out | (uintptr_t)zt_out;
  DK_REQUIRE((f32s & 15) == 0, "z, x_src, zs_out and zt_out must be 16-byte aligned");
  DK_REQUIRE((((uintptr_t)tokens | (prime ? 0 : (uintptr_t)model_out)) & 7) == 0, "model_out and tokens must be 8-byte aligned");
  DK_REQUIRE(std::isfinite(w_src) && std::isfinite(w_tar) && std::isfinite(c) && std::isfinite(sigma_in), "w_src, w_tar, c and sigma_in must be finite");
  DK_REQUIRE(draw >= 0, "draw must not be negative");
  FlowEditParams s = {};
  s.z = z, s.x_src = x_src, s.model_out = (const bf16_t*)model_out, s.ld_out = ld_out, s.tok = (bf16_t*)tokens, s.zs_out = zs_out, s.zt_out = zt_out;
  s.n_img = n_img, s.cfg_on = cfg_on != 0, s.Hl = Hl, s.Wl = Wl, s.C = C, s.p = p, s.reshape_order = reshape_order != 0;
  s.w_src = w_src, s.w_tar = w_tar, s.c = c, s.sigma_in = sigma_in, s.seeds = (const unsigned long long*)seeds, s.draw = draw, s.prime = prime != 0;
  return DK_EL(dtype, dk_launch_flowedit_step)(s, S_(stream));
}
extern "C" int dk_flowedit_step(float* z, const float* x_src, const void* model_out, int32_t ld_out, void* tokens, float* zs_out, float* zt_out,
                                int32_t n_img, int32_t cfg_on, int32_t Hl, int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float w_src,
                                float w_tar, float c, float sigma_in, const uint64_t* seeds, int32_t draw, int32_t prime, void* stream) {
  return flowedit_step(DK_DTYPE_BF16, z, x_src, model_out, ld_out, tokens, zs_out, zt_out, n_img, cfg_on, Hl, Wl, C, p, reshape_order, w_src, w_tar, c,
                       sigma_in, seeds, draw, prime, stream);
}
extern "C" int dk_flowedit_step_f16(float* z, const float* x_src, const void* model_out, int32_t ld_out, void* tokens, float* zs_out, float* zt_out,
                                    int32_t n_img, int32_t cfg_on, int32_t Hl, int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float w_src,
                                    float w_tar, float c, float sigma_in, const uint64_t* seeds, int32_t draw, int32_t prime, void* stream) {
  return flowedit_step(DK_DTYPE_F16, z, x_src, model_out, ld_out, tokens, zs_out, zt_out, n_img, cfg_on, Hl, Wl, C, p, reshape_order, w_src, w_tar, c,
                       sigma_in, seeds, draw, prime, stream);
}

extern "C" int dk_mask_to_latent_f32(const uint8_t* mask, float* out, int32_t n_mask, int32_t H, int32_t W, int32_t f, void* stream) {
  DK_REQUIRE(mask && out, "null argument");
  DK_REQUIRE(n_mask > 0, "n_mask must be positive");
  DK_REQUIRE(f > 0 && f <= 64 && H > 0 && W > 0 && H % f == 0 && W % f == 0, "mask size must be divisible by the factor (1..64)");
  return dk_launch_mask_to_latent(mask, out, n_mask, H, W, f, S_(stream));
}

extern "C" int dk_image_composite_u8(const uint8_t* dec, const uint8_t* orig, const uint8_t* mask, uint8_t* out, int32_t B, int32_t H,
                                     int32_t W, int32_t orig_per_image, int32_t mask_per_image, void* stream) {
  DK_REQUIRE(dec && orig && mask && out, "null argument");
  DK_REQUIRE(B > 0 && H > 0 && W > 0, "B, H and W must be positive");
  return dk_launch_image_composite_u8(dec, orig, mask, out, B, H, W, orig_per_image != 0, mask_per_image != 0, S_(stream));
}

extern "C" int dk_image_mask_out_f32(const uint8_t* image, const uint8_t* mask, float* out, int32_t n, int32_t n_mask, int32_t H, int32_t W,
                                     void* stream) {
  DK_REQUIRE(image && mask && out, "null argument");
  DK_REQUIRE(n > 0 && H > 0 && W > 0, "n, H and W must be positive");
  DK_REQUIRE(n_mask == 1 || n_mask == n, "n_mask must be 1 (one mask for every image) or n");
  return dk_launch_image_mask_out_f32(image, mask, out, n, H, W, n_mask == n && n > 1, S_(stream));
}

extern "C" int dk_fill_condition_tokens(const float* z, const uint8_t* mask, void* tokens, int32_t n, int32_t n_mask, int32_t Hl, int32_t Wl,
                                        int32_t C, int32_t patch, void* stream) {
  DK_REQUIRE(z && tokens, "null argument");
  DK_REQUIRE(n > 0 && C > 0 && patch > 0 && patch <= 16, "n, C and patch (1..16) must be positive");
  DK_REQUIRE(Hl > 0 && Wl > 0 && Hl % patch == 0 && Wl % patch == 0, "latent sides must be positive multiples of the patch size");
  DK_REQUIRE(Hl <= (1 << 20) && Wl <= (1 << 20), "latent sides too large");
  if (mask) DK_REQUIRE(n_mask == 1 || n_mask == n, "n_mask must be 1 (one mask for every image) or n");
  return dk_launch_fill_condition_tokens(z, mask, (bf16_t*)tokens, n, mask != nullptr && n_mask == n && n > 1, Hl, Wl, C, patch, S_(stream));
}

extern "C" int dk_affine_f32(const float* x, float* y, int64_t n, float a, float b, void* stream) {
  return dk_launch_affine_f32(x, y, (long)n, a, b, S_(stream));
}

static int gn_nchunk(long HW, int C) {
  const long ppi = 256 / (C / 8);
  long n = HW / (ppi * 8);
  if (n < 1) n = 1;
  if (n > 1024) n = 1024;
  return (int)n;
}
extern "C" size_t dk_groupnorm_scratch_floats(int32_t B, int32_t G) { return (size_t)B * 1024 * 2 * G + (size_t)B * G * 2; }
int groupnorm_launch(int dtype, const void* x, void* y, int B, long HW, int C, int G, const void* gamma, const void* beta, float eps,
                     int fuse_silu, float* scratch, hipStream_t st) {  // (dk_engine.h)
  // (dk_launch_groupnorm_apply's bound, asked before the statistics pass: a refused call launches nothing)
  DK_REQUIRE(C >= 8 && C % 8 == 0, "channels must be 8 * 2^k <= 2048");
  DK_REQUIRE((double)HW * (C / 8) < 2147483648.0, "one batch row must hold < 2^31 16-byte chunks");
  const int nchunk = gn_nchunk(HW, C);
  float* mean_rstd = scratch + (size_t)B * 1024 * 2 * G;
  int rc = DK_EL(dtype, dk_launch_groupnorm_stats)((const bf16_t*)x, B, HW, C, G, scratch, nchunk, mean_rstd, eps, st);
  if (rc) return rc;
  return DK_EL(dtype, dk_launch_groupnorm_apply)((const bf16_t*)x, (bf16_t*)y, B, HW, C, G, mean_rstd, (const bf16_t*)gamma, (const bf16_t*)beta,
                                                 fuse_silu, st);
}
extern "C" int dk_groupnorm_bf16(const void* x, void* y, int32_t B, int64_t HW, int32_t C, int32_t G, const void* gamma,
                                 const void* beta, float eps, int32_t fuse_silu, float* scratch, void* stream) {
  return groupnorm_launch(DK_DTYPE_BF16, x, y, B, (long)HW, C, G, gamma, beta, eps, fuse_silu, scratch, S_(stream));
}
extern "C" int dk_groupnorm_f16(const void* x, void* y, int32_t B, int64_t HW, int32_t C, int32_t G, const void* gamma,
                                const void* beta, float eps, int32_t fuse_silu, float* scratch, void* stream) {
  return groupnorm_launch(DK_DTYPE_F16, x, y, B, (long)HW, C, G, gamma, beta, eps, fuse_silu, scratch, S_(stream));
}

int groupnorm_table_launch(int dtype, const void* x, int B, long HW, int C, int G, const void* gamma, const void* beta, float eps,
                           float* scratch, int n_partial, float* scale_shift, hipStream_t st) {  // (dk_engine.h)
  DK_REQUIRE(gamma && beta && scratch && scale_shift && B > 0 && G > 0 && C % G == 0, "groupnorm table arguments");
  DK_REQUIRE(x != nullptr || n_partial > 0, "either x or the number of partials a conv launch left in scratch");
  // (the finalisation takes every partial of a conv launch for one 16 x 16-pixel tile: it weighs the pairs by their element counts)
  DK_REQUIRE(x != nullptr || (long)n_partial * 256 == HW, "partials of a conv launch: one per 16 x 16-pixel tile, n_partial * 256 == HW");
  const int nchunk = x ? gn_nchunk(HW, C) : n_partial;
  float* mean_rstd = scratch + (size_t)B * (nchunk > 1024 ? nchunk : 1024) * 2 * G;
  if (x) {  // the partial sums only: the one finalisation below builds mean / rstd AND the table
    const int rc = DK_EL(dtype, dk_launch_groupnorm_partials)((const bf16_t*)x, B, HW, C, G, scratch, nchunk, st);
    if (rc) return rc;
  }
  return DK_EL(dtype, dk_launch_groupnorm_finalize)(scratch, nchunk, B, G, HW, eps, mean_rstd, (const bf16_t*)gamma,
                                                    (const bf16_t*)beta, C, scale_shift, st);
}
extern "C" int dk_groupnorm_table_bf16(const void* x, int32_t B, int64_t HW, int32_t C, int32_t G, const void* gamma, const void* beta,
                                       float eps, float* scratch, int32_t n_partial, float* scale_shift, void* stream) {
  return groupnorm_table_launch(DK_DTYPE_BF16, x, B, (long)HW, C, G, gamma, beta, eps, scratch, n_partial, scale_shift, S_(stream));
}
extern "C" int dk_groupnorm_table_f16(const void* x, int32_t B, int64_t HW, int32_t C, int32_t G, const void* gamma, const void* beta,
                                      float eps, float* scratch, int32_t n_partial, float* scale_shift, void* stream) {
  return groupnorm_table_launch(DK_DTYPE_F16, x, B, (long)HW, C, G, gamma, beta, eps, scratch, n_partial, scale_shift, S_(stream));
}

static ConvHaloParams conv_halo_params(int dtype, const dk_conv_gn_desc* d) {
  ConvHaloParams p;
  memset(&p, 0, sizeof(p));
  p.dtype = dtype;
  p.x = (const bf16_t*)d->x; p.w = (const bf16_t*)d->w; p.bias = (const bf16_t*)d->bias; p.bias2 = (const bf16_t*)d->bias2;
  p.res = (const bf16_t*)d->res; p.y = (bf16_t*)d->y; p.gn_ss = d->gn_scale_shift; p.gn_silu = d->gn_silu;
  p.x2 = (const bf16_t*)d->x2; p.C2 = d->C2; p.stats_out = d->stats_partial; p.G_out = d->stats_groups;
  p.img = d->image_f32; p.u8 = d->image_u8; p.raw = (bf16_t*)d->raw_bf16; p.out_channels = d->O <= 4 ? d->O : 0;
  p.B = d->B; p.H = d->H; p.W = d->W; p.C = d->C; p.O = d->O; p.ups = d->upsample; p.ldw = d->ldw; p.ldy = d->ldy; p.ldr = d->ldr;
  return p;
}
static int conv3x3_gn(int dtype, const dk_conv_gn_desc* d, void* stream) {
  DK_REQUIRE(d && d->x && d->w && d->bias, "null argument");
  const bool img = d->image_f32 || d->image_u8 || d->raw_bf16;
  DK_REQUIRE(img || d->y, "no output");
  return dk_launch_conv_halo(conv_halo_params(dtype, d), S_(stream));
}
extern "C" int dk_conv3x3_gn_bf16(const dk_conv_gn_desc* d, void* stream) { return conv3x3_gn(DK_DTYPE_BF16, d, stream); }
extern "C" int dk_conv3x3_gn_f16(const dk_conv_gn_desc* d, void* stream) { return conv3x3_gn(DK_DTYPE_F16, d, stream); }

static int softmax_rows(int dtype, void* x, int rows, int cols, int ld, void* stream) {
  return DK_EL(dtype, dk_launch_softmax_rows)((bf16_t*)x, rows, cols, ld, S_(stream));
}
extern "C" int dk_softmax_rows_bf16(void* x, int32_t rows, int32_t cols, int32_t ld, void* stream) { return softmax_rows(DK_DTYPE_BF16, x, rows, cols, ld, stream); }
extern "C" int dk_softmax_rows_f16(void* x, int32_t rows, int32_t cols, int32_t ld, void* stream) { return softmax_rows(DK_DTYPE_F16, x, rows, cols, ld, stream); }
static int transpose(int dtype, const void* x, void* y, int R, int C, void* stream) {
  return DK_EL(dtype, dk_launch_transpose)((const bf16_t*)x, (bf16_t*)y, R, C, S_(stream), 0);
}
extern "C" int dk_transpose_bf16(const void* x, void* y, int32_t R, int32_t C, void* stream) { return transpose(DK_DTYPE_BF16, x, y, R, C, stream); }
extern "C" int dk_transpose_f16(const void* x, void* y, int32_t R, int32_t C, void* stream) { return transpose(DK_DTYPE_F16, x, y, R, C, stream); }
