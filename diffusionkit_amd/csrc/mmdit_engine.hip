// C-ABI layer (include/dk_hip.h), part 2: the MMDiT engine (dk_mmdit_*), which sequences the gfx950 kernels of the transformer blocks.
// Host code only: no kernels are defined here.
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#include "dk_engine.h"
#include "dk_score_bound.h"

int g_dk_fuse_k = 1;  // dk_tune_set("gemm_fuse_k", v): QKNorm + RoPE of the keys inside the q / k / v projection's tail (1, default) or as a separate pass (0)
int g_dk_fuse_qg = -1;  // dk_tune_set("gemm_fuse_q", v): ... and of the QUERIES there too (1) instead of in the attention kernel's Q load (0); -1 (default): on
                         // the fp8 path only -- measured in the model (profiles/r04_attention_qfuse_in_model.log): +1.0 % per step with fp8 weights, flat in bf16
int g_dk_fuse_q = 1;  // dk_tune_set("attn_fuse_q", v): QKNorm + RoPE of the queries inside the attention kernel's Q load (1, default) or as a separate pass (0)

// every attention kernel can normalise / rotate the queries in its Q load
static int fuse_q() { return g_dk_fuse_q ? 1 : 0; }
// the keys' QKNorm + RoPE rides in the q / k / v projection's tail (only together with the fused query side: the stand-alone pass
// then has nothing left to do)
static bool fuse_k(const bf16_t* kn) { return g_dk_fuse_k != 0 && fuse_q() && kn != nullptr; }
// ... and the queries' with it (round 4): the attention kernel then loads finished queries
static bool fuse_qg(const bf16_t* qn, bool f8) { return (g_dk_fuse_qg < 0 ? f8 : g_dk_fuse_qg != 0) && qn != nullptr; }
template <typename P>
static void set_key_norm(P& p, const bf16_t* kn, const bf16_t* qn, int h, int D, const float* rope, int pos_off, int seg_len) {
  p.kn_w = kn; p.kn_rope = rope; p.kn_col0 = h; p.kn_col1 = 2 * h; p.kn_D = D; p.kn_pos_off = pos_off; p.kn_seg_len = seg_len; p.kn_eps = 1e-6f;
  if (fuse_qg(qn, std::is_same<P, GemmF8Params>::value)) { p.qn_w = qn; p.qn_col0 = 0; p.qn_col1 = h; }
}
struct StreamW {  // one TransformerBlock's weights (mmdit.py:395-438)
  const bf16_t *qkv_w = nullptr, *qkv_b = nullptr, *qn = nullptr, *kn = nullptr;
  const bf16_t *o_w = nullptr, *o_b = nullptr, *fc1_w = nullptr, *fc1_b = nullptr, *fc2_w = nullptr, *fc2_b = nullptr;
  const bf16_t *l2_w = nullptr, *l2_b = nullptr;  // single blocks: [h, 5h] = [o_proj | fc2]
  // fp8_linears: e4m3 weights + per-output-channel scales instead of the bf16 matrices above (biases stay bf16)
  const unsigned char *qkv_w8 = nullptr, *o_w8 = nullptr, *fc1_w8 = nullptr, *fc2_w8 = nullptr, *l2_w8 = nullptr;
  const float *qkv_ws = nullptr, *o_ws = nullptr, *fc1_ws = nullptr, *fc2_ws = nullptr, *l2_ws = nullptr;
  // MMDiT-X (dk_mmdit_set_dual_attention), image stream of a dual block: the second attention's q | k | v matrix with its FULL bias (attn2's
  // k_proj keeps its bias), its own QKNorm weights and its output projection
  const bf16_t *qkv2_w = nullptr, *qkv2_b = nullptr, *qn2 = nullptr, *kn2 = nullptr, *o2_w = nullptr, *o2_b = nullptr;
  // max|w| of qn / kn, read once when the weights are resolved (norm_weight_maxima); 0: no such weight, or not bf16 -- no bound (dk_score_bound.h)
  float qn_max = 0.f, kn_max = 0.f;
};

struct dk_mmdit {
  dk_mmdit_config cfg;
  std::unordered_map<std::string, const void*> named;
  bool resolved = false;
  bool norm_max_ready = false;  // StreamW::qn_max / kn_max hold the resolved weights' maxima (norm_weight_maxima)
  // resolved weights
  const bf16_t *xemb_w, *xemb_b, *pos_w, *ctx_w, *ctx_b, *y0_w, *y0_b, *y2_w, *y2_b, *t0_w, *t0_b, *t2_w, *t2_b;
  const bf16_t *adaln_w, *adaln_b, *final_w, *final_b;
  std::vector<StreamW> dimg, dtxt, single;
  // shape
  // S_i: the rows the model predicts (tokens_in / tokens_out, the final layer, the first-block cache's buffers).  S_x: the rows of the
  // image stream inside the blocks = S_i + S_r, with S_r the reference image's rows behind the image rows (dk_mmdit_set_reference_grid;
  // 0 without one: S_x == S_i).  S = S_t + S_x
  int B = 0, Hl = 0, Wl = 0, S_t = 0, S_i = 0, S_r = 0, S_x = 0, S = 0, n_t = 0;
  int ref_h = 0, ref_w = 0;  // the reference latent's sides (0, 0: off)
  bf16_t* REFE = nullptr;    // x_embedder(reference tokens) [B, S_r, h], step-invariant (dk_mmdit_cache_reference)
  bool ref_ready = false;
  int ref_rows(int p) const { return (ref_h / p) * (ref_w / p); }
  // channel-concatenated conditioning (dk_mmdit_set_condition_width): x_embedder.proj.weight is [h, F + cond_f]; the condition's share of the
  // sum is step-invariant and kept in CONDE [B, S_i, h] (dk_mmdit_cache_condition), the residual operand of the x_embedder launch
  int cond_f = 0;
  bf16_t* CONDE = nullptr;
  bool cond_ready = false;
  bool prepared = false, mod_ready = false;
  // workspace views
  bf16_t *X, *XN, *QKV, *ATT, *CAT, *HID, *MOD, *POS;
  bf16_t* CTXE = nullptr;  // context_embedder(text) [B, S_t, h], step-invariant (dk_mmdit_cache_context)
  bool ctx_ready = false;
  int ldh = 0, ldcat = 0;  // row pitch of HID / CAT (dk_weight_pitch of r*h / (1+r)*h at carve time; fc2 / linear2 weights use the same)
  void* GWS = nullptr;  // GEMM split workspace (fp32 slabs + flags), dk_gemm_split_workspace_bytes()
  void* AWS = nullptr;  // attention5.hip's key-split partial results of THIS engine's launches (dk_attention_workspace_bytes(); D = 128 only)
  size_t AWS_bytes = 0;
  bf16_t *temb, *t1, *tvec, *y1, *yvec, *vec;
  float *rope, *tdev;
  // guidance embedding (cfg.guidance_embed): MLPEmbedder weights, the value set by dk_mmdit_set_guidance, scratch rows
  const bf16_t *g0_w = nullptr, *g0_b = nullptr, *g2_w = nullptr, *g2_b = nullptr;
  float guidance = 3.5f;
  bf16_t *gemb = nullptr, *g1 = nullptr, *gvec = nullptr;
  // ... or one value per batch row (dk_mmdit_set_guidance_rows; empty: the scalar above): 1000 g[b] as the embedding takes it.  The B-row twins of
  // the scratch rows live in QKV while the table is computed (dk_mmdit_cache_modulation_params): the workspace is the size it was
  std::vector<float> g_rows;
  // fp8_linears: MX-fp8 activation buffers + their scale side arrays (layout dk_mx_scale_index)
  unsigned char *XN8 = nullptr, *ATT8 = nullptr, *HC8 = nullptr;    // [rows8, h], [rows8, h], max([rows8, ldh8], [rows8, ldcat8])
  unsigned char *SXN = nullptr, *SATT = nullptr, *SHID = nullptr, *SCAT = nullptr;
  int ldh8 = 0, ldcat8 = 0, nblk = 0;
  // row order of the double blocks' fp8 buffers: image rows of all batch rows [0, B * S_i), text rows from txt0_8 =
  // ceil128(B * S_i) -- every row range an fp8 GEMM reads starts on a 128-row scale block; rows8 = txt0_8 + B * S_t >= B * S
  int txt0_8 = 0;
  long rows8 = 0;
  // element type of every bound tensor, activation buffer and of the token / text / pooled I/O (dk_mmdit_set_activation_dtype): sizes are the same
  int dtype = DK_DTYPE_BF16;
  // MMDiT-X dual attention (dk_mmdit_set_dual_attention): double blocks [0, n_dual) run a second attention over the image stream alone, from a
  // second modulation of the block's LayerNorm (XN2 [B S_x, h]) through QKV2 [B S_x, 3h] into ATT2 [B S_x, h]; their image modules have 9 rows
  int n_dual = 0;
  bf16_t *XN2 = nullptr, *QKV2 = nullptr, *ATT2 = nullptr;
  int img_rows(int i) const { return i < n_dual ? 9 : 6; }
  // skip-layer guidance (dk_mmdit_set_skip_layers): the last fork_rows batch rows are a copy of the first fork_rows that joins in front of double
  // block min(skip) and sits out the blocks in skip (sorted, distinct).  Empty / 0: off
  std::vector<int32_t> skip;
  int fork_rows = 0;
  bool slg() const { return !skip.empty(); }
  bool skipped(int g) const { return std::find(skip.begin(), skip.end(), g) != skip.end(); }
  // perturbed-attention guidance (dk_mmdit_set_perturbed_attention): the same fork (fork_rows is shared: one of the two features at a time), joining in
  // front of double block min(pag); in the blocks of pag (sorted, distinct) the fork rows' main attention is the identity launch.  Empty: off
  std::vector<int32_t> pag;
  bool perturbed() const { return !pag.empty(); }
  bool perturbed(int g) const { return std::find(pag.begin(), pag.end(), g) != pag.end(); }
  // first-block cache (dk_mmdit_set_block_cache; include/dk_hip.h): image rows [B * S_i, h] each.  BC_R: X1 at the start of a compute tail, R
  // behind it.  BC_D[bc_cur]: X0 before block 0, D_cur behind the probe; BC_D[1 - bc_cur]: D_ref -- a compute tail swaps the two.
  // BC_ROWS: the probe's (num, den) per image row.  bc_valid: R / D_ref come from a computed step since the last reset; bc_pending: the step
  // whose head ran last and waits for its tail, or -1
  bool bc_on = false, bc_valid = false;
  int bc_cur = 0, bc_pending = -1;
  bf16_t *BC_R = nullptr, *BC_D[2] = {nullptr, nullptr};
  float* BC_ROWS = nullptr;
  void bc_reset() { bc_valid = false; bc_pending = -1; }
  // SD3 ControlNet (include/dk_hip.h).  control_net (dk_mmdit_set_control_net): this engine IS the ControlNet -- no final layer, a second
  // patch embedder whose step-invariant share POS + pos_embed_input(control tokens) sits in CONDE (dk_mmdit_cache_control_image), one tap
  // Linear per block.  taps (dk_mmdit_set_control_taps): this engine is the MAIN model and adds tap_scale * taps[tap_of(g)] behind block g
  bool control_net = false, ctrl_ready = false;
  const bf16_t *cin_w = nullptr, *cin_b = nullptr;
  std::vector<const bf16_t*> tap_w, tap_b;
  const bf16_t* taps = nullptr;  // [n_taps, B, S_i, h], the caller's
  int n_taps = 0;
  float tap_scale = 0.f;
  int tap_of(int g) const { return (int)((long)g * n_taps / cfg.depth_multimodal); }
  // FLUX ControlNet (the layout of diffusers' FluxControlNetModel).  control_flux (dk_mmdit_set_flux_control_net, with control_net): the ControlNet
  // of FLUX geometry -- RoPE, single blocks, controlnet_x_embedder in the place of pos_embed_input, CONDE without positional rows, tap Linears
  // tap_w / tap_b [0, depth_multimodal) behind the double and [depth_multimodal, +depth_unified) behind the single blocks.  n_dtaps / n_staps
  // (dk_mmdit_set_flux_control_taps): the MAIN engine's taps [n_dtaps + n_staps, B, S_i, h], double taps first; tap g / ceil(depth / n) behind
  // block g of each kind, the last block of a kind included
  bool control_flux = false;
  const bf16_t *cxe_w = nullptr, *cxe_b = nullptr;
  int n_dtaps = 0, n_staps = 0;
  bool flux_tapped() const { return n_dtaps + n_staps > 0; }
  bool tapped() const { return n_taps > 0 || flux_tapped(); }
  static int flux_tap_of(int g, int n, int depth) { return g / ((depth + n - 1) / n); }
  // FLUX IP-Adapter (dk_mmdit_set_ip_adapter; include/dk_hip.h): ip_n image-prompt tokens of ip_c features per image.  ipkv_w / ipkv_b: the
  // adapter's to_k_ip / to_v_ip of every double block as ONE matrix [depth_multimodal * 2h, ip_c] (rows [i 2h, i 2h + h) block i's keys, the next
  // h its values) and its bias.  IPKV [B * ip_n, depth_multimodal * 2h]: their step-invariant projections (dk_mmdit_cache_ip_tokens) -- block i's
  // keys of image b at rows b ip_n .., columns i 2h .., its values h columns further.  IP [B * S_i, h]: the adapter's output of the double block
  // that ran last, added with ip_scale in the LayerNorm launch that reads the image rows next (the tap slot) -- one buffer for all blocks
  int ip_n = 0, ip_c = 0;
  const bf16_t *ipkv_w = nullptr, *ipkv_b = nullptr;
  bf16_t *IPKV = nullptr, *IP = nullptr;
  bool ip_ready = false;
  float ip_scale = 0.f;
  bool ip_active() const { return ip_n > 0 && ip_scale != 0.f; }
  float tap_s() const { return ip_active() ? ip_scale : tap_scale; }  // (taps and the adapter are never set together)
  // the tap added behind block g of the global order (in front of whatever reads the image rows next), or null
  const bf16_t* tap_behind(int g) const {
    const int nd = cfg.depth_multimodal;
    const size_t tap = (size_t)B * S_i * cfg.hidden_size;
    if (ip_active()) return g >= 0 && g < nd ? IP : nullptr;  // (the adapter's output behind every double block, nothing behind a single one)
    if (g < 0 || !tapped()) return nullptr;
    if (n_taps > 0) return g < nd - 1 ? taps + (size_t)tap_of(g) * tap : nullptr;  // (SD3: nothing behind the last block)
    if (g < nd) return n_dtaps > 0 ? taps + (size_t)flux_tap_of(g, n_dtaps, nd) * tap : nullptr;
    return n_staps > 0 ? taps + (size_t)(n_dtaps + flux_tap_of(g - nd, n_staps, cfg.depth_unified)) * tap : nullptr;
  }
  // what a call on `stream` hands its launches: this engine's element type and ITS regions (for D = 64 no attention region: unsplit launches)
  LaunchCtx ctx(void* stream) const { return LaunchCtx{S_(stream), dtype, GWS, AttnWs{AWS, AWS_bytes}}; }
  bool fp8() const { return cfg.fp8_linears != 0; }
  // precision policy: the first n_bf16() double-stream blocks keep bf16 Linears under fp8_linears (global block index = double-block index)
  int n_bf16() const { return fp8() ? (cfg.fp8_bf16_double_blocks < cfg.depth_multimodal ? cfg.fp8_bf16_double_blocks : cfg.depth_multimodal) : 0; }

  // row views of the joint-stream buffers [B, S, ld] (X, QKV, ATT; text rows first in every batch row): the image / the text rows of all batch
  // rows.  XN, HID and CAT hold plain [M, ld] rows: dense(ptr, ld).  img: the image STREAM (reference rows included); own: the S_i image
  // rows alone
  Rows img(bf16_t* buf, int ld) const { return Rows{buf + (size_t)S_t * ld, ld, S_x, S}; }
  Rows own(bf16_t* buf, int ld) const { return Rows{buf + (size_t)S_t * ld, ld, S_i, S}; }
  Rows txt(bf16_t* buf, int ld) const { return Rows{buf, ld, S_t, S}; }

  int h() const { return cfg.hidden_size; }
  int D() const { return cfg.hidden_size / cfg.num_heads; }
  int F() const { return cfg.patch_size * cfg.patch_size * cfg.vae_latent_dim; }
  bool txt_skipped(int i) const { return i == cfg.depth_multimodal - 1 && cfg.depth_unified < 1; }
  int mod_rows() const {
    int n = 0;
    for (int i = 0; i < cfg.depth_multimodal; ++i) n += img_rows(i) + (txt_skipped(i) ? 2 : 6);
    return n + 3 * cfg.depth_unified + (control_net ? 0 : 2);  // (a control-net engine has no final layer, and no rows for one)
  }
  int mod_offset(int kind, int index) const {
    int n = 0;
    for (int i = 0; i < cfg.depth_multimodal; ++i) {
      if (kind == 0 && i == index) return n;
      n += img_rows(i);
      if (kind == 1 && i == index) return n;
      n += txt_skipped(i) ? 2 : 6;
    }
    for (int i = 0; i < cfg.depth_unified; ++i) {
      if (kind == 2 && i == index) return n;
      n += 3;
    }
    if (kind == 3) return n;
    return -1;
  }
};

extern "C" int dk_mmdit_create(const dk_mmdit_config* cfg, dk_mmdit** out) {
  DK_REQUIRE(cfg && out, "null argument");
  DK_REQUIRE(cfg->hidden_size % cfg->num_heads == 0, "hidden_size must be divisible by num_heads");
  const int D = cfg->hidden_size / cfg->num_heads;
  DK_REQUIRE(D == 64 || D == 128, "head_dim must be 64 or 128");
  DK_REQUIRE(cfg->hidden_size % 64 == 0, "hidden_size must be a multiple of 64");
  DK_REQUIRE((cfg->patch_size * cfg->patch_size * cfg->vae_latent_dim) % 64 == 0, "patch feature size must be a multiple of 64");
  DK_REQUIRE(cfg->token_level_text_embed_dim % 64 == 0 && cfg->pooled_text_embed_dim % 64 == 0 &&
                 cfg->frequency_embed_dim % 64 == 0,
             "embedding dims must be multiples of 64");
  if (cfg->use_rope) {
    int half = 0;
    for (int i = 0; i < cfg->n_rope_axes; ++i) half += cfg->rope_axes_dim[i] / 2;
    DK_REQUIRE(half * 2 == D, "rope axes must sum to head_dim");
  }
  if (cfg->fp8_linears) DK_REQUIRE(D == 128 && cfg->hidden_size % 256 == 0, "fp8_linears: head_dim 128 and hidden_size a multiple of 256");
  dk_mmdit* m = new dk_mmdit();
  m->cfg = *cfg;
  *out = m;
  return 0;
}
extern "C" int dk_mmdit_set_guidance(dk_mmdit* m, float guidance) {
  DK_REQUIRE(m != nullptr, "null handle");
  DK_REQUIRE(m->cfg.guidance_embed, "this configuration has no guidance embedding (guidance_embed = 0)");
  m->guidance = guidance;
  m->mod_ready = false;
  return 0;
}
extern "C" int dk_mmdit_set_guidance_rows(dk_mmdit* m, const float* g, int32_t n) {
  DK_REQUIRE(m != nullptr, "null handle");
  DK_REQUIRE(m->cfg.guidance_embed, "this configuration has no guidance embedding (guidance_embed = 0)");
  if (g == nullptr || n == 0) {  // back to the scalar of dk_mmdit_set_guidance
    if (!m->g_rows.empty()) m->mod_ready = false;
    m->g_rows.clear();
    return 0;
  }
  DK_REQUIRE(m->prepared, "dk_mmdit_prepare must precede dk_mmdit_set_guidance_rows: the rows are those of the prepared batch");
  DK_REQUIRE(n == m->B, "guidance rows: n must be the prepared batch");
  for (int b = 0; b < n; ++b) DK_REQUIRE(std::isfinite(g[b]), "guidance rows must be finite");
  m->g_rows.resize(n);
  for (int b = 0; b < n; ++b) m->g_rows[b] = 1000.0f * g[b];
  m->mod_ready = false;
  return 0;
}
extern "C" int dk_mmdit_set_activation_dtype(dk_mmdit* m, int32_t dtype) {
  DK_REQUIRE(m != nullptr, "null handle");
  DK_REQUIRE(dtype == DK_DTYPE_BF16 || dtype == DK_DTYPE_F16, "activation dtype: 0 bf16, 1 fp16");
  DK_REQUIRE(m->named.empty() && !m->prepared, "dk_mmdit_set_activation_dtype must precede the first dk_mmdit_bind");
  if (dtype == DK_DTYPE_F16)
    DK_REQUIRE(m->D() == 64 && m->cfg.depth_unified == 0 && m->cfg.fp8_linears == 0,
               "fp16 activations are the SD3 family's: head_dim == 64, depth_unified == 0, fp8_linears == 0");
  m->dtype = dtype;
  return 0;
}
extern "C" int dk_mmdit_set_dual_attention(dk_mmdit* m, int32_t n_blocks) {
  DK_REQUIRE(m != nullptr, "null handle");
  DK_REQUIRE(!m->resolved && !m->prepared, "dk_mmdit_set_dual_attention is legal only before the weights are resolved (the first dk_mmdit_prepare)");
  DK_REQUIRE(n_blocks >= 0 && n_blocks <= m->cfg.depth_multimodal, "dual attention blocks must lie in [0, depth_multimodal]");
  if (n_blocks > 0) {
    DK_REQUIRE(m->cfg.depth_unified == 0 && m->cfg.fp8_linears == 0,
               "dual attention blocks are the SD3 family's (MMDiT-X): depth_unified == 0 and fp8_linears == 0");
    DK_REQUIRE(!m->control_net && !m->tapped(), "dual attention blocks cannot be set on a control-net engine or while control taps are set");
    DK_REQUIRE(m->ip_n == 0, "dual attention blocks cannot be set on an engine with an IP-Adapter (dk_mmdit_set_ip_adapter)");
  }
  m->n_dual = n_blocks;
  m->mod_ready = false;
  return 0;
}
extern "C" void dk_mmdit_destroy(dk_mmdit* m) { delete m; }

extern "C" int dk_mmdit_bind(dk_mmdit* m, const char* name, const void* dev_ptr) {
  DK_REQUIRE(m && name && dev_ptr, "null argument");
  m->named[name] = dev_ptr;
  m->resolved = false;
  return 0;
}
extern "C" int dk_mmdit_mod_rows(const dk_mmdit* m) { return m->mod_rows(); }
extern "C" int dk_mmdit_mod_offset(const dk_mmdit* m, int32_t kind, int32_t index) { return m->mod_offset(kind, index); }

// the matrix of one Linear: bf16 "<name>.weight", or (fp8_linears) e4m3 "<name>.weight_fp8" + f32 "<name>.wscale"
static int need_matrix(dk_mmdit* m, bool f8, const std::string& name, const bf16_t** w, const unsigned char** w8, const float** ws) {
  if (!f8) return need(m->named, name + ".weight", w);
  const bf16_t *a = nullptr, *b = nullptr;
  DK_TRY(need(m->named, name + ".weight_fp8", &a));
  DK_TRY(need(m->named, name + ".wscale", &b));
  *w8 = (const unsigned char*)a;
  *ws = (const float*)b;
  return 0;
}
static int resolve_stream(dk_mmdit* m, const std::string& p, StreamW& w, bool single, bool skip_post, bool f8) {
  const auto& n = m->named;
  if (single) {  // fused [q|k|v|fc1] matrix; fc1 views point into it
    DK_TRY(need_matrix(m, f8, p + ".linear1", &w.qkv_w, &w.qkv_w8, &w.qkv_ws));
    DK_TRY(need(n, p + ".linear1.bias", &w.qkv_b));
    if (!f8) w.fc1_w = w.qkv_w + (size_t)3 * m->h() * m->h();
    w.fc1_b = w.qkv_b + 3 * m->h();
  } else {
    DK_TRY(need_matrix(m, f8, p + ".attn.qkv", &w.qkv_w, &w.qkv_w8, &w.qkv_ws));
    DK_TRY(need(n, p + ".attn.qkv.bias", &w.qkv_b));
  }
  if (m->cfg.use_qk_norm) {
    DK_TRY(need(n, p + ".qk_norm.q_norm.weight", &w.qn));
    DK_TRY(need(n, p + ".qk_norm.k_norm.weight", &w.kn));
  }
  if (skip_post) return 0;
  if (!single) {
    DK_TRY(need_matrix(m, f8, p + ".mlp.fc1", &w.fc1_w, &w.fc1_w8, &w.fc1_ws));
    DK_TRY(need(n, p + ".mlp.fc1.bias", &w.fc1_b));
  }
  if (single) {
    DK_TRY(need_matrix(m, f8, p + ".linear2", &w.l2_w, &w.l2_w8, &w.l2_ws));
    DK_TRY(need(n, p + ".linear2.bias", &w.l2_b));
  } else {
    DK_TRY(need_matrix(m, f8, p + ".attn.o_proj", &w.o_w, &w.o_w8, &w.o_ws));
    DK_TRY(need(n, p + ".attn.o_proj.bias", &w.o_b));
    DK_TRY(need_matrix(m, f8, p + ".mlp.fc2", &w.fc2_w, &w.fc2_w8, &w.fc2_ws));
    DK_TRY(need(n, p + ".mlp.fc2.bias", &w.fc2_b));
  }
  return 0;
}

// the second attention of an MMDiT-X image stream: required inside the dual range, refused outside it (a checkpoint with attn2 tensors on an
// engine that would ignore them is a configuration error, not something to run)
static int resolve_attn2(dk_mmdit* m, const std::string& p, StreamW& w, bool dual) {
  const auto& n = m->named;
  static const char* const kNames[] = {".attn2.qkv.weight", ".attn2.qkv.bias", ".attn2.o_proj.weight", ".attn2.o_proj.bias", ".qk_norm2.q_norm.weight",
                                       ".qk_norm2.k_norm.weight"};
  if (!dual) {
    for (const char* s : kNames)
      if (n.find(p + s) != n.end()) {
        dk_set_error("weight bound outside the dual attention range (dk_mmdit_set_dual_attention): " + p + s);
        return -3;
      }
    return 0;
  }
  DK_TRY(need(n, p + ".attn2.qkv.weight", &w.qkv2_w));
  DK_TRY(need(n, p + ".attn2.qkv.bias", &w.qkv2_b));
  DK_TRY(need(n, p + ".attn2.o_proj.weight", &w.o2_w));
  DK_TRY(need(n, p + ".attn2.o_proj.bias", &w.o2_b));
  if (m->cfg.use_qk_norm) {
    DK_TRY(need(n, p + ".qk_norm2.q_norm.weight", &w.qn2));
    DK_TRY(need(n, p + ".qk_norm2.k_norm.weight", &w.kn2));
  }
  return 0;
}

// The QKNorm vectors of every block (D values each) come to the host ONCE per resolved set of weights: what bounds the attention scores of a
// launch (joint_attention).  Load-time work -- dk_mmdit_bind clears `resolved`, mmdit_resolve clears `norm_max_ready`, and the first prepare
// behind it comes through here, where its device work begins (resolving alone touches no device).  bf16 engines only (the kernel that uses
// the bound is bf16 only); the copies are ordered behind whatever `st` holds, the stream the caller prepares on.
static int norm_weight_maxima(dk_mmdit* m, hipStream_t st) {
  if (m->norm_max_ready) return 0;
  std::vector<StreamW*> ws;
  for (auto* v : {&m->dimg, &m->dtxt, &m->single})
    for (StreamW& w : *v) {
      w.qn_max = w.kn_max = 0.f;
      if (m->dtype == DK_DTYPE_BF16 && w.qn != nullptr && w.kn != nullptr) ws.push_back(&w);
    }
  const int D = m->D();
  std::vector<uint16_t> host(ws.size() * 2 * (size_t)D);
  for (size_t i = 0; i < ws.size(); ++i) {
    DK_CHECK_HIP(hipMemcpyAsync(&host[(2 * i) * D], ws[i]->qn, (size_t)D * 2, hipMemcpyDeviceToHost, st));
    DK_CHECK_HIP(hipMemcpyAsync(&host[(2 * i + 1) * D], ws[i]->kn, (size_t)D * 2, hipMemcpyDeviceToHost, st));
  }
  if (!ws.empty()) DK_CHECK_HIP(hipStreamSynchronize(st));
  std::vector<float> mx(ws.size() * 2);
  dk_norm_weight_maxima(host.data(), mx.size(), D, mx.data());
  for (size_t i = 0; i < ws.size(); ++i) ws[i]->qn_max = mx[2 * i], ws[i]->kn_max = mx[2 * i + 1];
  m->norm_max_ready = true;
  return 0;
}

static int mmdit_resolve(dk_mmdit* m) {
  if (m->resolved) return 0;
  const auto& n = m->named;
  DK_TRY(need(n, "x_embedder.proj.weight", &m->xemb_w));
  DK_TRY(need(n, "x_embedder.proj.bias", &m->xemb_b));
  DK_TRY(need(n, "x_pos_embedder.pos_embed.weight", &m->pos_w, !m->cfg.use_pos_embed));
  DK_TRY(need(n, "context_embedder.weight", &m->ctx_w));
  DK_TRY(need(n, "context_embedder.bias", &m->ctx_b));
  DK_TRY(need(n, "y_embedder.mlp.layers.0.weight", &m->y0_w));
  DK_TRY(need(n, "y_embedder.mlp.layers.0.bias", &m->y0_b));
  DK_TRY(need(n, "y_embedder.mlp.layers.2.weight", &m->y2_w));
  DK_TRY(need(n, "y_embedder.mlp.layers.2.bias", &m->y2_b));
  DK_TRY(need(n, "t_embedder.mlp.layers.0.weight", &m->t0_w));
  DK_TRY(need(n, "t_embedder.mlp.layers.0.bias", &m->t0_b));
  DK_TRY(need(n, "t_embedder.mlp.layers.2.weight", &m->t2_w));
  DK_TRY(need(n, "t_embedder.mlp.layers.2.bias", &m->t2_b));
  DK_TRY(need(n, "adaLN.weight", &m->adaln_w));
  DK_TRY(need(n, "adaLN.bias", &m->adaln_b));
  DK_TRY(need(n, "final_layer.linear.weight", &m->final_w, m->control_net));
  DK_TRY(need(n, "final_layer.linear.bias", &m->final_b, m->control_net));
  if (m->control_net) {
    if (m->control_flux) {
      DK_TRY(need(n, "controlnet_x_embedder.proj.weight", &m->cxe_w));
      DK_TRY(need(n, "controlnet_x_embedder.proj.bias", &m->cxe_b));
    } else {
      DK_TRY(need(n, "pos_embed_input.proj.weight", &m->cin_w));
      DK_TRY(need(n, "pos_embed_input.proj.bias", &m->cin_b));
    }
    const int nd = m->cfg.depth_multimodal, ns = m->control_flux ? m->cfg.depth_unified : 0;
    m->tap_w.assign(nd + ns, nullptr);
    m->tap_b.assign(nd + ns, nullptr);
    for (int i = 0; i < nd; ++i) {
      DK_TRY(need(n, "controlnet_blocks." + std::to_string(i) + ".weight", &m->tap_w[i]));
      DK_TRY(need(n, "controlnet_blocks." + std::to_string(i) + ".bias", &m->tap_b[i]));
    }
    for (int i = 0; i < ns; ++i) {
      DK_TRY(need(n, "controlnet_single_blocks." + std::to_string(i) + ".weight", &m->tap_w[nd + i]));
      DK_TRY(need(n, "controlnet_single_blocks." + std::to_string(i) + ".bias", &m->tap_b[nd + i]));
    }
  }
  if (m->cfg.guidance_embed) {
    DK_TRY(need(n, "guidance_in.mlp.layers.0.weight", &m->g0_w));
    DK_TRY(need(n, "guidance_in.mlp.layers.0.bias", &m->g0_b));
    DK_TRY(need(n, "guidance_in.mlp.layers.2.weight", &m->g2_w));
    DK_TRY(need(n, "guidance_in.mlp.layers.2.bias", &m->g2_b));
  }
  m->dimg.assign(m->cfg.depth_multimodal, StreamW());
  m->dtxt.assign(m->cfg.depth_multimodal, StreamW());
  m->single.assign(m->cfg.depth_unified, StreamW());
  for (int i = 0; i < m->cfg.depth_multimodal; ++i) {
    const std::string b = "multimodal_transformer_blocks." + std::to_string(i);
    const bool f8 = m->fp8() && i >= m->n_bf16();
    DK_TRY(resolve_stream(m, b + ".image_transformer_block", m->dimg[i], false, false, f8));
    DK_TRY(resolve_stream(m, b + ".text_transformer_block", m->dtxt[i], false, m->txt_skipped(i), f8));
    // (the fused QKNorm decisions of a double block are taken per stream from these pointers and must agree: ADVICE r4)
    DK_REQUIRE((m->dimg[i].qn == nullptr) == (m->dtxt[i].qn == nullptr) && (m->dimg[i].kn == nullptr) == (m->dtxt[i].kn == nullptr),
               "QKNorm weights must be bound for both streams of a double block or for neither");
    DK_TRY(resolve_attn2(m, b + ".image_transformer_block", m->dimg[i], i < m->n_dual));
  }
  for (int i = 0; i < m->cfg.depth_unified; ++i)
    DK_TRY(resolve_stream(m, "unified_transformer_blocks." + std::to_string(i) + ".transformer_block", m->single[i], true, false, m->fp8()));
  m->ipkv_w = m->ipkv_b = nullptr;
  if (m->ip_n > 0) {  // the adapter's Linears: bound by their own names, read as one matrix by one GEMM (dk_mmdit_cache_ip_tokens)
    const size_t hh = (size_t)m->h();
    for (int i = 0; i < m->cfg.depth_multimodal; ++i) {
      const std::string b = "ip_adapter." + std::to_string(i);
      const bf16_t *kw, *kb, *vw, *vb;
      DK_TRY(need(n, b + ".to_k_ip.weight", &kw));
      DK_TRY(need(n, b + ".to_k_ip.bias", &kb));
      DK_TRY(need(n, b + ".to_v_ip.weight", &vw));
      DK_TRY(need(n, b + ".to_v_ip.bias", &vb));
      if (i == 0) { m->ipkv_w = kw; m->ipkv_b = kb; }
      if (kw != m->ipkv_w + (size_t)i * 2 * hh * m->ip_c || vw != kw + hh * m->ip_c || kb != m->ipkv_b + (size_t)i * 2 * hh || vb != kb + hh) {
        dk_set_error("the IP-Adapter's tensors must be views of one stacked [depth_multimodal * 2h, token_dim] matrix and one [depth_multimodal * 2h] bias, block i's "
                     "to_k_ip rows at i * 2h and its to_v_ip rows h further: " + b);
        return -3;
      }
    }
  }
  m->norm_max_ready = false;  // (the StreamW records are new: maxima 0, no bound, until norm_weight_maxima has read the weights)
  m->resolved = true;
  return 0;
}

static size_t mmdit_carve(dk_mmdit* m, Carver& c, int B, int Hl, int Wl, int S_t, int n_t) {
  const int h = m->h(), p = m->cfg.patch_size;
  const int S_i = (Hl / p) * (Wl / p), S_r = m->ref_rows(p), S_x = S_i + S_r, S = S_t + S_x;
  const size_t BS = (size_t)B * S;
  m->X = (bf16_t*)c.take(BS * h * 2);
  m->XN = (bf16_t*)c.take(BS * h * 2);
  m->QKV = (bf16_t*)c.take(BS * 3 * h * 2);
  m->ATT = (bf16_t*)c.take(BS * h * 2);
  m->ldh = dk_weight_pitch(m->cfg.mlp_ratio * h);
  m->ldcat = dk_weight_pitch((1 + m->cfg.mlp_ratio) * h);
  const size_t hid = BS * m->ldh * 2;  // MLP hidden of both streams of a double block (image rows first)
  const size_t cat = m->cfg.depth_unified > 0 ? BS * (size_t)m->ldcat * 2 : 0;
  // single blocks: [attn | gelu(fc1)]; double blocks: MLP hidden (fp8_linears: only the bf16 double blocks of the precision policy need it)
  m->CAT = (bf16_t*)c.take(m->fp8() ? (m->n_bf16() > 0 ? hid : 0) : (cat > hid ? cat : hid));
  m->HID = m->CAT;
  if (m->fp8()) {  // the same buffers in MX-fp8 (the bf16 X, QKV, ATT above stay: residual stream, attention operands / output)
    const int r = m->cfg.mlp_ratio;
    m->ldh8 = dk_weight_pitch_fp8(r * h);
    m->ldcat8 = dk_weight_pitch_fp8((1 + r) * h);
    // (a ragged image token count pads the image rows to the next scale block; aligned counts: rows8 == BS, the sizes they always had)
    m->txt0_8 = (int)align_up((size_t)B * S_x, 128);
    m->rows8 = (long)m->txt0_8 + (long)B * S_t;
    const size_t R8 = (size_t)m->rows8;
    m->nblk = mx_nblk(m->rows8);
    m->XN8 = (unsigned char*)c.take(R8 * h);
    m->ATT8 = (unsigned char*)c.take(R8 * h);
    const size_t hid8 = R8 * (size_t)m->ldh8, cat8 = m->cfg.depth_unified > 0 ? R8 * (size_t)m->ldcat8 : 0;
    m->HC8 = (unsigned char*)c.take(cat8 > hid8 ? cat8 : hid8);
    m->SXN = (unsigned char*)c.take(dk_mx_scale_bytes(m->rows8, h));
    m->SATT = (unsigned char*)c.take(dk_mx_scale_bytes(m->rows8, h));
    m->SHID = (unsigned char*)c.take(dk_mx_scale_bytes(m->rows8, r * h));
    m->SCAT = (unsigned char*)c.take(m->cfg.depth_unified > 0 ? dk_mx_scale_bytes(m->rows8, (1 + r) * h) : 0);
  }
  m->MOD = (bf16_t*)c.take((size_t)n_t * B * m->mod_rows() * h * 2);
  m->POS = (bf16_t*)c.take(m->cfg.use_pos_embed ? (size_t)S_i * h * 2 : 0);
  m->CTXE = (bf16_t*)c.take((size_t)B * S_t * h * 2);
  m->temb = (bf16_t*)c.take((size_t)n_t * m->cfg.frequency_embed_dim * 2);
  m->t1 = (bf16_t*)c.take((size_t)n_t * h * 2);
  m->tvec = (bf16_t*)c.take((size_t)n_t * h * 2);
  m->y1 = (bf16_t*)c.take((size_t)B * h * 2);
  m->yvec = (bf16_t*)c.take((size_t)B * h * 2);
  m->vec = (bf16_t*)c.take((size_t)n_t * B * h * 2);
  m->gemb = (bf16_t*)c.take(m->cfg.guidance_embed ? (size_t)m->cfg.frequency_embed_dim * 2 : 0);
  m->g1 = (bf16_t*)c.take(m->cfg.guidance_embed ? (size_t)h * 2 : 0);
  m->gvec = (bf16_t*)c.take(m->cfg.guidance_embed ? (size_t)h * 2 : 0);
  m->rope = (float*)c.take(m->cfg.use_rope ? (size_t)S * m->D() * 4 : 0);
  m->tdev = (float*)c.take((size_t)n_t * 4);
  m->GWS = c.take(dk_gemm_split_workspace_bytes());
  // this engine's own region for the key-split jobs of attention5.hip (two engines, or an engine and ops.attention, driven from one
  // host thread on different streams must not share the partial results of their split launches)
  m->AWS_bytes = m->D() == 128 ? dk_attention_workspace_bytes() : 0;
  m->AWS = c.take(m->AWS_bytes);
  if (m->bc_on) {  // (behind everything else: with the cache off the carve is what it was)
    const size_t img = (size_t)B * S_i * h * 2;
    m->BC_R = (bf16_t*)c.take(img);
    m->BC_D[0] = (bf16_t*)c.take(img);
    m->BC_D[1] = (bf16_t*)c.take(img);
    m->BC_ROWS = (float*)c.take((size_t)B * S_i * 2 * 4);
  }
  m->REFE = nullptr;
  if (S_r > 0) m->REFE = (bf16_t*)c.take((size_t)B * S_r * h * 2);  // (behind everything else, and no take at all without a reference)
  m->CONDE = nullptr;
  if (m->cond_f > 0 || m->control_net) m->CONDE = (bf16_t*)c.take((size_t)B * S_i * h * 2);  // (the same: no take with both off)
  m->XN2 = m->QKV2 = m->ATT2 = nullptr;
  if (m->n_dual > 0) {  // (the same: no take without dual blocks)
    const size_t Mi = (size_t)B * S_x;
    m->XN2 = (bf16_t*)c.take(Mi * h * 2);
    m->QKV2 = (bf16_t*)c.take(Mi * 3 * h * 2);
    m->ATT2 = (bf16_t*)c.take(Mi * h * 2);
  }
  m->IPKV = m->IP = nullptr;
  if (m->ip_n > 0) {  // (the same: no take without an IP-Adapter)
    m->IPKV = (bf16_t*)c.take((size_t)m->cfg.depth_multimodal * B * m->ip_n * 2 * h * 2);
    m->IP = (bf16_t*)c.take((size_t)B * S_i * h * 2);
  }
  return c.off;
}

extern "C" size_t dk_mmdit_workspace_bytes(const dk_mmdit* m, int32_t batch, int32_t latent_h, int32_t latent_w, int32_t text_len,
                                           int32_t n_timesteps) {
  dk_mmdit tmp = *m;
  Carver c(nullptr, 0);
  return mmdit_carve(&tmp, c, batch, latent_h, latent_w, text_len, n_timesteps) + 256;
}

extern "C" int dk_mmdit_prepare(dk_mmdit* m, int32_t batch, int32_t latent_h, int32_t latent_w, int32_t text_len,
                                int32_t n_timesteps, void* workspace, size_t workspace_bytes, void* stream) {
  DK_REQUIRE(m && workspace, "null argument");
  DK_REQUIRE(batch > 0 && text_len > 0 && n_timesteps > 0, "empty problem");
  const int p = m->cfg.patch_size;
  DK_REQUIRE(latent_h % p == 0 && latent_w % p == 0, "latent size must be divisible by the patch size");
  DK_TRY(mmdit_resolve(m));
  // (the image token count is free: a last, partial scale block is handled by the row order of the fp8 buffers, mmdit_carve)
  if (m->fp8()) DK_REQUIRE(text_len % 128 == 0, "fp8_linears: only text lengths that are multiples of 128 are supported (MX scale blocks of 128 rows; the image token count is free)");
  DK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  Carver c(workspace, workspace_bytes);
  const size_t need_bytes = mmdit_carve(m, c, batch, latent_h, latent_w, text_len, n_timesteps);
  DK_REQUIRE(need_bytes <= workspace_bytes, "workspace too small");
  m->g_rows.clear();  // (they were the rows of the batch prepared before)
  m->B = batch; m->Hl = latent_h; m->Wl = latent_w; m->S_t = text_len;
  m->S_i = (latent_h / p) * (latent_w / p); m->S_r = m->ref_rows(p); m->S_x = m->S_i + m->S_r; m->S = m->S_t + m->S_x; m->n_t = n_timesteps;
  hipStream_t st = S_(stream);
  DK_TRY(norm_weight_maxima(m, st));
  if (m->cfg.use_rope) {  // the image at index 0 and, behind it, the reference image's own grid at index 1
    const int seg[6] = {latent_h / p, latent_w / p, 0, m->ref_h / p, m->ref_w / p, 1};
    DK_TRY(dk_launch_rope_table_segments(m->rope, m->S_t, m->S_r > 0 ? 2 : 1, seg, m->cfg.rope_axes_dim, m->cfg.n_rope_axes,
                                         (float)m->cfg.rope_theta, st));
  }
  if (m->cfg.use_pos_embed) {
    // centre crop of the learned table (mmdit.py:334-349): rows y0..y0+gh, cols x0..x0+gw
    const int mh = m->cfg.max_latent_resolution, gh = latent_h / p, gw = latent_w / p;
    DK_REQUIRE(gh <= mh && gw <= mh, "latent larger than the positional table");
    const int y0 = (mh - gh) / 2, x0 = (mh - gw) / 2;
    DK_CHECK_HIP(hipMemcpy2DAsync(m->POS, (size_t)gw * m->h() * 2, m->pos_w + ((size_t)y0 * mh + x0) * m->h(),
                                  (size_t)mh * m->h() * 2, (size_t)gw * m->h() * 2, gh, hipMemcpyDeviceToDevice, st));
  }
  // the flag region of the GEMM split workspace must be zero before the first launch (the kernels leave it zero)
  DK_CHECK_HIP(hipMemsetAsync((char*)m->GWS + DK_KSPLIT_FLAGS_OFF, 0, DK_KSPLIT_FLAG_BYTES, st));
  m->prepared = true;
  m->mod_ready = false;
  m->ctx_ready = false;
  m->ref_ready = false;
  m->cond_ready = false;
  m->ctrl_ready = false;
  m->taps = nullptr; m->n_taps = 0; m->tap_scale = 0.f;  // (the caller's taps had the previous problem's shape: set again after prepare)
  m->n_dtaps = m->n_staps = 0;
  m->ip_ready = false;  // (the cache lives in the workspace that was just carved; the scale stays)
  m->bc_reset();
  return 0;
}

// ---- reference-image conditioning (include/dk_hip.h) --------------------------------------------------------------------------------
extern "C" int dk_mmdit_set_reference_grid(dk_mmdit* m, int32_t ref_latent_h, int32_t ref_latent_w) {
  DK_REQUIRE(m != nullptr, "null handle");
  if (ref_latent_h != 0 || ref_latent_w != 0) {
    const int p = m->cfg.patch_size;
    DK_REQUIRE(m->cond_f == 0, "a reference grid and a condition width cannot be set at the same time");
    DK_REQUIRE(!m->control_net && !m->tapped(), "a reference grid cannot be set on a control-net engine or while control taps are set");
    DK_REQUIRE(m->ip_n == 0, "a reference grid cannot be set on an engine with an IP-Adapter (dk_mmdit_set_ip_adapter)");
    DK_REQUIRE(m->cfg.use_rope, "a reference grid needs RoPE (use_rope = 1, the FLUX family): the reference rows are told from the image rows by their position index");
    DK_REQUIRE(ref_latent_h > 0 && ref_latent_w > 0 && ref_latent_h % p == 0 && ref_latent_w % p == 0,
               "reference latent sides must both be positive multiples of the patch size, or both 0 (off)");
    DK_REQUIRE((long)(ref_latent_h / p) * (ref_latent_w / p) <= (1L << 24), "reference grid too large");
  }
  if (m->ref_h != ref_latent_h || m->ref_w != ref_latent_w) m->prepared = false;  // (another carve: dk_mmdit_prepare must follow)
  m->ref_h = ref_latent_h; m->ref_w = ref_latent_w;
  m->ref_ready = false;
  m->bc_reset();
  return 0;
}
extern "C" int dk_mmdit_cache_reference(dk_mmdit* m, const void* ref_tokens, int32_t per_image, void* stream) {
  DK_REQUIRE(m && m->prepared && ref_tokens, "prepare must precede cache_reference");
  DK_REQUIRE(m->S_r > 0, "cache_reference needs a reference grid: dk_mmdit_set_reference_grid before dk_mmdit_prepare");
  const int h = m->h(), F = m->F(), S_r = m->S_r;
  // x_embedder as in mmdit_embed (no split workspace), one launch per batch row: a shared reference gives every batch row the bits a
  // per-image copy of it would
  for (int b = 0; b < m->B; ++b) {
    const bf16_t* src = (const bf16_t*)ref_tokens + (per_image ? (size_t)b * S_r * F : 0);
    DK_TRY(dk_launch_gemm(Linear(m->dtype, dense(src, F), m->xemb_w, m->xemb_b, dense(m->REFE + (size_t)b * S_r * h, h), S_r, h, F, DK_EPI_BIAS), S_(stream)));
  }
  m->ref_ready = true;
  m->bc_reset();  // (R and D_ref belong to the conditioning they were computed under)
  return 0;
}
// what every entry that runs blocks asks of an engine with a reference grid
static int need_reference(const dk_mmdit* m) {
  DK_REQUIRE(m->S_r == 0 || m->ref_ready, "an engine with a reference grid needs dk_mmdit_cache_reference after dk_mmdit_prepare");
  return 0;
}

// ---- channel-concatenated conditioning (include/dk_hip.h) ---------------------------------------------------------------------------
extern "C" int dk_mmdit_set_condition_width(dk_mmdit* m, int32_t cond_features) {
  DK_REQUIRE(m != nullptr, "null handle");
  if (cond_features != 0) {
    DK_REQUIRE(cond_features > 0 && cond_features % 64 == 0 && cond_features <= (1 << 16), "the condition width must be a positive multiple of 64, or 0 (off)");
    DK_REQUIRE(m->cfg.use_pos_embed == 0, "a condition width needs use_pos_embed == 0 (the FLUX family): the residual operand of the x_embedder launch carries the condition's share");
    DK_REQUIRE(m->ref_h == 0 && m->ref_w == 0, "a condition width and a reference grid cannot be set at the same time");
    DK_REQUIRE(m->dtype == DK_DTYPE_BF16, "a condition width needs bf16 activations");
    DK_REQUIRE(m->ip_n == 0, "a condition width cannot be set on an engine with an IP-Adapter (dk_mmdit_set_ip_adapter)");
    DK_REQUIRE(!m->control_net && !m->tapped(), "a condition width cannot be set on a control-net engine or while control taps are set");
  }
  if (m->cond_f != cond_features) m->prepared = false;  // (another carve: dk_mmdit_prepare must follow)
  m->cond_f = cond_features;
  m->cond_ready = false;
  m->bc_reset();
  return 0;
}
extern "C" int dk_mmdit_cache_condition(dk_mmdit* m, const void* cond_tokens, int32_t per_image, void* stream) {
  DK_REQUIRE(m && m->prepared && cond_tokens, "prepare must precede cache_condition");
  DK_REQUIRE(m->cond_f > 0, "cache_condition needs a condition width: dk_mmdit_set_condition_width before dk_mmdit_prepare");
  const int h = m->h(), F = m->F(), Fc = m->cond_f, S_i = m->S_i;
  // the condition columns of x_embedder's weight, W[:, F:], without the bias (the x_embedder launch of every evaluation adds it once); one
  // launch per batch row: a shared condition gives every batch row the bits a per-image copy of it would
  for (int b = 0; b < m->B; ++b) {
    const bf16_t* src = (const bf16_t*)cond_tokens + (per_image ? (size_t)b * S_i * Fc : 0);
    DK_TRY(dk_launch_gemm(Linear(m->dtype, dense(src, Fc), m->xemb_w + F, nullptr, dense(m->CONDE + (size_t)b * S_i * h, h), S_i, h, Fc, DK_EPI_BIAS, F + Fc),
                          S_(stream)));
  }
  m->cond_ready = true;
  m->bc_reset();  // (R and D_ref belong to the conditioning they were computed under)
  return 0;
}
// what every entry that runs blocks asks of an engine with a condition width
static int need_condition(const dk_mmdit* m) {
  DK_REQUIRE(m->cond_f == 0 || m->cond_ready, "an engine with a condition width needs dk_mmdit_cache_condition after dk_mmdit_prepare");
  return 0;
}

extern "C" int dk_mmdit_cache_modulation_params(dk_mmdit* m, const void* pooled, const float* timesteps_host, int32_t n,
                                                void* stream) {
  DK_REQUIRE(m && m->prepared, "dk_mmdit_prepare must be called first");
  DK_REQUIRE(n > 0 && n <= m->n_t, "more timesteps than the workspace was prepared for");
  hipStream_t st = S_(stream);
  const int dt = m->dtype;
  const int h = m->h(), B = m->B, P = m->cfg.pooled_text_embed_dim, Fq = m->cfg.frequency_embed_dim;
  DK_CHECK_HIP(hipMemcpyAsync(m->tdev, timesteps_host, (size_t)n * 4, hipMemcpyHostToDevice, st));
  DK_TRY(DK_EL(dt, dk_launch_timestep_embedding)(m->tdev, n, 1, Fq, (float)m->cfg.max_period, m->cfg.embed_dtype, m->temb, st));
  // t_embedder / y_embedder: Linear -> SiLU -> Linear (mmdit.py:352-392)
  DK_TRY(dk_launch_gemm(Linear(dt, dense(m->temb, Fq), m->t0_w, m->t0_b, dense(m->t1, h), n, h, Fq, DK_EPI_BIAS_SILU), st));
  DK_TRY(dk_launch_gemm(Linear(dt, dense(m->t1, h), m->t2_w, m->t2_b, dense(m->tvec, h), n, h, h, DK_EPI_BIAS), st));
  DK_TRY(dk_launch_gemm(Linear(dt, dense((const bf16_t*)pooled, P), m->y0_w, m->y0_b, dense(m->y1, h), B, h, P, DK_EPI_BIAS_SILU), st));
  DK_TRY(dk_launch_gemm(Linear(dt, dense(m->y1, h), m->y2_w, m->y2_b, dense(m->yvec, h), B, h, h, DK_EPI_BIAS), st));
  if (m->cfg.guidance_embed && !m->g_rows.empty()) {
    // ... with a value per batch row (dk_mmdit_set_guidance_rows): the same three launches on B rows, and y[b] += g[b] row by row.  Their scratch
    // -- B values, B embeddings, B hidden rows, B vectors -- is the head of QKV, which no launch reads or writes outside a forward (same stream)
    const size_t o1 = align_up((size_t)B * 4, 256), o2 = o1 + align_up((size_t)B * Fq * 2, 256), o3 = o2 + align_up((size_t)B * h * 2, 256);
    DK_REQUIRE(o3 + (size_t)B * h * 2 <= (size_t)B * m->S * 3 * h * 2, "guidance rows: the QKV buffer is too small for their scratch");
    char* const scratch = (char*)m->QKV;
    float* const gdev = (float*)scratch;
    bf16_t *const gemb = (bf16_t*)(scratch + o1), *const g1 = (bf16_t*)(scratch + o2), *const gvec = (bf16_t*)(scratch + o3);
    DK_CHECK_HIP(hipMemcpyAsync(gdev, m->g_rows.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));
    DK_TRY(DK_EL(dt, dk_launch_timestep_embedding)(gdev, B, 1, Fq, (float)m->cfg.max_period, m->cfg.embed_dtype, gemb, st));
    DK_TRY(dk_launch_gemm(Linear(dt, dense(gemb, Fq), m->g0_w, m->g0_b, dense(g1, h), B, h, Fq, DK_EPI_BIAS_SILU), st));
    DK_TRY(dk_launch_gemm(Linear(dt, dense(g1, h), m->g2_w, m->g2_b, dense(gvec, h), B, h, h, DK_EPI_BIAS), st));
    for (int b = 0; b < B; ++b)
      DK_TRY(DK_EL(dt, dk_launch_add)(m->yvec + (size_t)b * h, gvec + (size_t)b * h, 1, m->yvec + (size_t)b * h, 1, h, st));
  } else if (m->cfg.guidance_embed) {
    // FLUX.1-dev guidance embedding (MLPEmbedder, mmdit.py:31-36,945-955): g = guidance_in(timestep_embedding(1000 * guidance)),
    // added to the pooled-text embedding of every batch row, hence to every modulation vector
    const float gt = 1000.0f * m->guidance;
    DK_CHECK_HIP(hipMemcpyAsync(m->tdev, &gt, 4, hipMemcpyHostToDevice, st));  // (tdev[0] was consumed by the launch above, same stream)
    DK_TRY(DK_EL(dt, dk_launch_timestep_embedding)(m->tdev, 1, 1, Fq, (float)m->cfg.max_period, m->cfg.embed_dtype, m->gemb, st));
    DK_TRY(dk_launch_gemm(Linear(dt, dense(m->gemb, Fq), m->g0_w, m->g0_b, dense(m->g1, h), 1, h, Fq, DK_EPI_BIAS_SILU), st));
    DK_TRY(dk_launch_gemm(Linear(dt, dense(m->g1, h), m->g2_w, m->g2_b, dense(m->gvec, h), 1, h, h, DK_EPI_BIAS), st));
    DK_TRY(DK_EL(dt, dk_launch_add)(m->yvec, m->gvec, 1, m->yvec, B, h, st));  // y[b] += g
  }
  // vec[step*B + b] = silu(y[b] + t[step]); adaLN_modulation = SiLU -> Linear (mmdit.py:94-96,430-435)
  DK_TRY(DK_EL(dt, dk_launch_add)(m->yvec, m->tvec, n, m->vec, n * B, h, st));
  DK_TRY(DK_EL(dt, dk_launch_silu)(m->vec, m->vec, (long)n * B * h, st));
  const int Nmod = m->mod_rows() * h;
  DK_TRY(dk_launch_gemm(Linear(dt, dense(m->vec, h), m->adaln_w, m->adaln_b, dense(m->MOD, Nmod), n * B, Nmod, h, DK_EPI_BIAS), st));
  m->mod_ready = true;
  m->bc_reset();  // (R and D_ref belong to the conditioning they were computed under)
  return 0;
}

extern "C" int dk_mmdit_cache_context(dk_mmdit* m, const void* text, void* stream) {
  DK_REQUIRE(m && m->prepared && text, "prepare must precede cache_context");
  const int M = m->B * m->S_t, T = m->cfg.token_level_text_embed_dim;
  // (no split workspace: like the per-step form in dk_mmdit_forward, whose result it stands for)
  DK_TRY(dk_launch_gemm(Linear(m->dtype, dense((const bf16_t*)text, T), m->ctx_w, m->ctx_b, dense(m->CTXE, m->h()), M, m->h(), T, DK_EPI_BIAS), S_(stream)));
  m->ctx_ready = true;
  return 0;
}

// FinalLayer (mmdit.py:767-796) on the image rows
static int mmdit_final_layer(dk_mmdit* m, const bf16_t* mod_step, bf16_t* tokens_out, const LaunchCtx& L) {
  const hipStream_t st = L.st;
  const int h = m->h(), B = m->B, S = m->S, S_t = m->S_t, S_i = m->S_i, F = m->F();
  const int mod_stride = m->mod_rows() * h;
  const bf16_t* mod_fin = mod_step + (size_t)m->mod_offset(3, 0) * h;
  // (FLUX ControlNet taps: the residual behind the last block of the model lands here -- the image rows alone, every one of them tapped)
  const bf16_t* tap = m->tap_behind(m->cfg.depth_multimodal + m->cfg.depth_unified - 1);
  if (tap != nullptr)
    DK_TRY(dk_launch_ln_modulate_add_joint(m->X + (size_t)S_t * h, h, tap, h, m->tap_s(), S_i, 0, m->XN, h, B * S_i, h, mod_fin, mod_fin + h, mod_stride,
                                           S_i, S_i, S, m->cfg.layer_norm_eps, st));
  else
    DK_TRY(DK_EL(L.dtype, dk_launch_ln_modulate)(m->X + (size_t)S_t * h, h, m->XN, h, B * S_i, h, mod_fin, mod_fin + h, mod_stride, S_i, S_i, S,
                                 m->cfg.layer_norm_eps, st));
  return dk_launch_gemm(Linear(L.dtype, dense(m->XN, h), m->final_w, m->final_b, dense(tokens_out, F), B * S_i, F, h, DK_EPI_BIAS), st);
}

// ---- the transformer blocks -----------------------------------------------------------------------------------------------------
// What every block of a call derives from the prepared shape, built once per call (mmdit_blocks)
struct BlockCtx {
  int h, B, S, S_t, S_i, Mi, Mt;  // S_i: rows of the image STREAM per batch row (dk_mmdit::S_x: a reference image's rows included -- to a
                                  // block they are image rows); Mi / Mt: image-stream / text rows of all batch rows
  int mod_stride;                 // modulation rows of one batch row
  float scale;
  const float* rope;
  Rows X_img, X_txt;  // the two streams of the residual m->X
  // fp8 row order.  XN8 / HID8: image rows [0, Mi), text rows [T0, T0 + Mt) with T0 = ceil128(Mi) (= Mi, the bf16 path's row order, for aligned
  // image token counts).  CAT8 is indexed like the joint stream (b * S + s); so is ATT8 while S_i is a multiple of 128 -- with a ragged S_i the
  // image segment of batch row b >= 1 would start inside a scale block, and ATT8 takes the row order of XN8 instead (att_split: the attention
  // launch maps (b, s) to it, the o-projections read two plain row ranges)
  int T0;
  long R8;
  bool att_split;
  Mx8Out xn_img, xn_txt, xn_all;  // (xn_all -- single blocks: the joint stream from row 0, any M)
};
// (B: the batch rows [0, B) the blocks run on -- the prepared batch, or its live rows while a forked row group sits out, dk_mmdit_set_skip_layers)
static BlockCtx block_ctx(const dk_mmdit* m, int B) {
  BlockCtx c;
  memset(&c, 0, sizeof(c));
  c.h = m->h(); c.B = B; c.S = m->S; c.S_t = m->S_t; c.S_i = m->S_x; c.Mi = B * m->S_x; c.Mt = B * m->S_t;
  c.mod_stride = m->mod_rows() * c.h;
  c.scale = 1.0f / sqrtf((float)m->D());
  c.rope = m->cfg.use_rope ? m->rope : nullptr;
  c.X_img = m->img(m->X, c.h); c.X_txt = m->txt(m->X, c.h);
  if (m->fp8()) {
    c.T0 = m->txt0_8; c.R8 = m->rows8; c.att_split = c.S_i % 128 != 0;
    c.xn_img = mx8_out(m->XN8, m->SXN, c.h, c.R8, 0, c.Mi, 0, 0);
    c.xn_txt = mx8_out(m->XN8, m->SXN, c.h, c.R8, c.T0, c.Mt, 0, 0);
    c.xn_all = mx8_out(m->XN8, m->SXN, c.h, c.R8, 0, c.B * c.S, 0, 0);
  }
  return c;
}
// modulation rows of block `index` of `kind` (mod_offset) in the step's table
static const bf16_t* block_mod(const dk_mmdit* m, const bf16_t* mod_step, int kind, int index) {
  return mod_step + (size_t)m->mod_offset(kind, index) * m->h();
}
// QKNorm + RoPE: the keys in the projection's tail (or one pass over the buffer) -- for both streams of a double block or for neither
static bool keys_in_tail(const StreamW& a, const StreamW* b) { return fuse_k(a.kn) && (b == nullptr || fuse_k(b->kn)); }
// ... and the projection's tail finished the queries of every stream of the block too: the attention kernel loads them plain
static bool queries_in_tail(const StreamW& a, const StreamW* b, bool f8) {
  return keys_in_tail(a, b) && fuse_qg(a.qn, f8) && (b == nullptr || fuse_qg(b->qn, f8));
}
// Attention over the joint sequence of m->QKV into O (pitch ldo).  The queries that the projection's tail left raw are normalised / rotated
// in the Q load: text rows with wt's weight, image rows with wi's (double block), or all rows with wt's (single block: wi null).
// O8 / O8_scales / o8_ld: the MX-fp8 copy of the output the fp8 path's next Linear reads (it comes out of the attention kernel or out of a
// quantiser pass behind it: attention.hip); null on the bf16 path
// the bound on |scale * q.k| of a block's joint attention from the maxima of its streams' norm weights (0: unknown)
static float block_score_bound(const StreamW& wt, const StreamW* wi, int D, float scale) {
  return dk_score_bound(std::max(wt.qn_max, wi ? wi->qn_max : 0.f), std::max(wt.kn_max, wi ? wi->kn_max : 0.f), D, scale);
}
static AttnParams joint_attention(const dk_mmdit* m, const BlockCtx& c, bf16_t* O, int ldo, const StreamW& wt, const StreamW* wi,
                                  unsigned char* O8 = nullptr, unsigned char* O8_scales = nullptr, int o8_ld = 0) {
  AttnParams ap;
  ap.dtype = m->dtype;
  ap.Q = m->QKV; ap.K = m->QKV + c.h; ap.V = m->QKV + 2 * c.h; ap.O = O;
  ap.B = c.B; ap.H = m->cfg.num_heads; ap.S = c.S; ap.D = m->D(); ap.ld = 3 * c.h; ap.ldo = ldo; ap.scale = c.scale;
  if (fuse_q() && !queries_in_tail(wt, wi, O8 != nullptr)) {
    ap.qn_a = wt.qn; ap.qn_b = wi ? wi->qn : wt.qn; ap.qn_split = wi ? c.S_t : 0; ap.q_rope = c.rope;
  }
  if (O8 != nullptr) { ap.O8 = O8; ap.O8_scales = O8_scales; ap.o8_ld = o8_ld; ap.o8_nblk = m->nblk; }
  // Every query and key of the launch is QK-normed -- the keys in the projection's tail or by the separate pass, the queries there or in the Q
  // load -- whenever the weights exist: the scores are bounded by the weights' maxima (0 without weights: unknown).  The perturbed-attention
  // launch reuses these parameters on the fork rows (same operands, same bound; its kernel does not read it); the dual-attention launch of
  // MMDiT-X (D = 64, the lean kernel) passes none.
  ap.score_bound = block_score_bound(wt, wi, ap.D, ap.scale);
  return ap;
}
extern "C" float dk_mmdit_score_bound(const dk_mmdit* m, int32_t kind, int32_t index) {
  if (m == nullptr || !m->resolved || !m->norm_max_ready || index < 0) return 0.f;
  const float scale = 1.0f / sqrtf((float)m->D());  // (block_ctx)
  if (kind == 0 && index < (int)m->dimg.size()) return block_score_bound(m->dtxt[index], &m->dimg[index], m->D(), scale);
  if (kind == 2 && index < (int)m->single.size()) return block_score_bound(m->single[index], nullptr, m->D(), scale);
  return 0.f;
}

// MultiModalTransformerBlock i (mmdit.py:568-675), bf16 Linears.  The two streams run the same Linear shapes on different weights; their
// GEMMs are issued as pairs so that the 256 x 256 kernel can place the text tiles in the same wave as the image tiles
// (dk_launch_gemm_pair).  Every block Linear carries the engine's split workspace.
static int double_block_bf16(dk_mmdit* m, const BlockCtx& c, int i, const bf16_t* mod_step, const LaunchCtx& L) {
  const hipStream_t st = L.st;
  const dk_mmdit_config& cf = m->cfg;
  const int h = c.h, S = c.S, S_t = c.S_t, S_i = c.S_i, Mi = c.Mi, Mt = c.Mt, r = cf.mlp_ratio, ldh = m->ldh, mod_stride = c.mod_stride;
  const bf16_t *mod_img = block_mod(m, mod_step, 0, i), *mod_txt = block_mod(m, mod_step, 1, i);
  const StreamW &wi = m->dimg[i], &wt = m->dtxt[i];
  const bool txt_post = !m->txt_skipped(i);
  const Rows X_img = c.X_img, X_txt = c.X_txt;
  const Rows XN_img = dense(m->XN, h), XN_txt = dense(m->XN + (size_t)Mi * h, h);              // (image rows first)
  const Rows HID_img = dense(m->HID, ldh), HID_txt = dense(m->HID + (size_t)Mi * ldh, ldh);  // MLP hidden of both streams
  // pre_sdpa (mmdit.py:440-519): LN-modulate, q/k/v projection, QK-norm (+ RoPE)
  // (image and text stream of each elementwise stage in ONE launch: the 256 text rows do not run alone on the chip)
  // (MMDiT-X dual block: the image rows leave the same pass a second time, under shift_msa2 / scale_msa2 -- rows 6 and 7 of the 9 -- into XN2)
  const bool dual = i < m->n_dual;
  if (dual)
    DK_TRY(DK_EL(L.dtype, dk_launch_ln_modulate2x)(X_img.p, XN_img.p, m->XN2, Mi, mod_img, mod_img + h, mod_img + 6 * h, mod_img + 7 * h, S_i, X_txt.p,
                                                   XN_txt.p, Mt, mod_txt, mod_txt + h, S_t, h, h, h, mod_stride, S, S, cf.layer_norm_eps, st));
  else if (m->tap_behind(i - 1) != nullptr)
    // ControlNet taps (dk_mmdit_set_control_taps / dk_mmdit_set_flux_control_taps): the residual behind block i - 1 is added here, in front of block
    // i -- the same stream state -- in the pass that reads every image row anyway; the image rows are rewritten in place, the text job is the plain one
    DK_TRY(DK_EL(L.dtype, dk_launch_ln_modulate2_add)(X_img.p, m->tap_behind(i - 1), h, m->tap_s(), XN_img.p, Mi, mod_img,
                                                      mod_img + h, S_i, X_txt.p, XN_txt.p, Mt, mod_txt, mod_txt + h, S_t, h, h, h, mod_stride, S, S,
                                                      cf.layer_norm_eps, st));
  else
    DK_TRY(DK_EL(L.dtype, dk_launch_ln_modulate2)(X_img.p, XN_img.p, Mi, mod_img, mod_img + h, S_i, X_txt.p, XN_txt.p, Mt, mod_txt, mod_txt + h, S_t, h, h, h,
                                                  mod_stride, S, cf.layer_norm_eps, st));
  Linear qkv_img = Linear(L.dtype, XN_img, wi.qkv_w, wi.qkv_b, m->img(m->QKV, 3 * h), Mi, 3 * h, h, DK_EPI_BIAS).split_ws(L.kws);
  Linear qkv_txt = Linear(L.dtype, XN_txt, wt.qkv_w, wt.qkv_b, m->txt(m->QKV, 3 * h), Mt, 3 * h, h, DK_EPI_BIAS).split_ws(L.kws);
  // QKNorm + RoPE: the keys in the projection's tail (or one pass over the buffer), the queries inside the attention kernel's Q load
  const bool kf = keys_in_tail(wi, &wt);
  if (kf) {
    set_key_norm(qkv_img, wi.kn, wi.qn, h, m->D(), c.rope, S_t, S_i);
    set_key_norm(qkv_txt, wt.kn, wt.qn, h, m->D(), c.rope, 0, S_t);
  }
  DK_TRY(dk_launch_gemm_pair(qkv_img, qkv_txt, st));
  if (!kf)
    DK_TRY(DK_EL(L.dtype, dk_launch_qk_norm_rope2)(m->QKV + (size_t)S_t * 3 * h, Mi, wi.qn, wi.kn, S_i, S_t, m->QKV, Mt, wt.qn, wt.kn, S_t, 0, 3 * h, 0, h,
                                   cf.num_heads, m->D(), 1e-6f, c.rope, S, st, fuse_q()));
  // FLUX IP-Adapter (dk_mmdit_set_ip_adapter): the image rows' q columns still hold the raw projection (need_ip_adapter: the attention kernel norms
  // and rotates in its Q load), which is the operand the published definition attends from once QK-normed.  The output waits in IP for the
  // LayerNorm launch that reads the image rows next (tap_behind(i)); that launch ran for block i - 1's output before this one overwrites it
  if (m->ip_active())
    DK_TRY(dk_launch_ip_attention(m->QKV, 3 * h, S_i, S, S_t, wi.qn, m->IPKV + (size_t)i * 2 * h, m->IPKV + (size_t)i * 2 * h + h, cf.depth_multimodal * 2 * h,
                                  c.B, m->ip_n, h, m->D(), c.scale, 1e-6f, m->IP, st));
  // attn2's projection on the second modulation, a launch of its own: it has the image job's M and fills the chip as that one does, and the
  // pair above stays the launch of a plain block.  Its QKNorm follows the same switches as the main attention's, without a RoPE table
  const bool kf2 = dual && fuse_k(wi.kn2);
  if (dual) {
    Linear qkv2 = Linear(L.dtype, dense(m->XN2, h), wi.qkv2_w, wi.qkv2_b, dense(m->QKV2, 3 * h), Mi, 3 * h, h, DK_EPI_BIAS).split_ws(L.kws);
    if (kf2) set_key_norm(qkv2, wi.kn2, wi.qn2, h, m->D(), nullptr, 0, S_i);
    DK_TRY(dk_launch_gemm(qkv2, st));
    if (!kf2)
      DK_TRY(DK_EL(L.dtype, dk_launch_qk_norm_rope)(m->QKV2, 3 * h, 0, h, Mi, cf.num_heads, m->D(), wi.qn2, wi.kn2, 1e-6f, nullptr, S_i, S_i, 0, S_i, st, fuse_q()));
  }
  // perturbed attention (dk_mmdit_set_perturbed_attention): in a block of the set, run on the whole batch, the fork rows [live, B) take the identity
  // launch -- the same operands advanced by `live` batch rows, image queries seeing the text keys and their own -- and the live rows the plain one
  const int ident_rows = m->perturbed(i) && c.B == m->B ? m->fork_rows : 0;
  AttnParams att = joint_attention(m, c, m->ATT, h, wt, &wi);
  att.B = c.B - ident_rows;
  DK_TRY(dk_launch_attention(att, L.aws, st));
  if (ident_rows > 0) {
    const size_t rows = (size_t)att.B * S;
    att.Q += rows * 3 * h; att.K += rows * 3 * h; att.V += rows * 3 * h; att.O += rows * h;
    att.B = ident_rows;
    att.ident_from = S_t;
    DK_TRY(dk_launch_attention(att, L.aws, st));
  }
  if (dual) {  // the image stream alone: [B, S_i] dense rows of QKV2, no text rows, no RoPE
    AttnParams ap;
    ap.dtype = m->dtype;
    ap.Q = m->QKV2; ap.K = m->QKV2 + h; ap.V = m->QKV2 + 2 * h; ap.O = m->ATT2;
    ap.B = c.B; ap.H = cf.num_heads; ap.S = S_i; ap.D = m->D(); ap.ld = 3 * h; ap.ldo = h; ap.scale = c.scale;
    if (fuse_q() && !(kf2 && fuse_qg(wi.qn2, false))) { ap.qn_a = wi.qn2; ap.qn_b = wi.qn2; ap.qn_split = 0; }
    DK_TRY(dk_launch_attention(ap, L.aws, st));
  }
  // post_sdpa, sequential form (mmdit.py:537-548): residual += gate_attn * o_proj(attn)
  const Linear o_img = Linear(L.dtype, m->img(m->ATT, h), wi.o_w, wi.o_b, X_img, Mi, h, h, DK_EPI_GATE_RES)
                           .gate_res(mod_img + 2 * h, S_i, mod_stride, X_img).split_ws(L.kws);
  if (txt_post) {
    const Linear o_txt = Linear(L.dtype, m->txt(m->ATT, h), wt.o_w, wt.o_b, X_txt, Mt, h, h, DK_EPI_GATE_RES)
                             .gate_res(mod_txt + 2 * h, S_t, mod_stride, X_txt).split_ws(L.kws);
    DK_TRY(dk_launch_gemm_pair(o_img, o_txt, st));
  } else {
    DK_TRY(dk_launch_gemm(o_img, st));
  }
  // ... += gate_msa2 * attn2.o_proj(a2) (row 8 of the 9): behind o_proj, both write X_img in place
  if (dual)
    DK_TRY(dk_launch_gemm(Linear(L.dtype, dense(m->ATT2, h), wi.o2_w, wi.o2_b, X_img, Mi, h, h, DK_EPI_GATE_RES)
                              .gate_res(mod_img + 8 * h, S_i, mod_stride, X_img).split_ws(L.kws), st));
  // residual += gate_mlp * fc2(gelu(fc1(LN-mod(residual))))
  if (txt_post)
    DK_TRY(DK_EL(L.dtype, dk_launch_ln_modulate2)(X_img.p, XN_img.p, Mi, mod_img + 3 * h, mod_img + 4 * h, S_i, X_txt.p, XN_txt.p, Mt, mod_txt + 3 * h,
                                  mod_txt + 4 * h, S_t, h, h, h, mod_stride, S, cf.layer_norm_eps, st));
  else
    DK_TRY(DK_EL(L.dtype, dk_launch_ln_modulate)(X_img.p, h, XN_img.p, h, Mi, h, mod_img + 3 * h, mod_img + 4 * h, mod_stride, S_i, S_i, S, cf.layer_norm_eps, st));
  const Linear fc1_img = Linear(L.dtype, XN_img, wi.fc1_w, wi.fc1_b, HID_img, Mi, r * h, h, DK_EPI_BIAS_GELU).split_ws(L.kws);
  const Linear fc2_img = Linear(L.dtype, HID_img, wi.fc2_w, wi.fc2_b, X_img, Mi, h, r * h, DK_EPI_GATE_RES, ldh)
                             .gate_res(mod_img + 5 * h, S_i, mod_stride, X_img).split_ws(L.kws);
  if (txt_post) {
    const Linear fc1_txt = Linear(L.dtype, XN_txt, wt.fc1_w, wt.fc1_b, HID_txt, Mt, r * h, h, DK_EPI_BIAS_GELU).split_ws(L.kws);
    const Linear fc2_txt = Linear(L.dtype, HID_txt, wt.fc2_w, wt.fc2_b, X_txt, Mt, h, r * h, DK_EPI_GATE_RES, ldh)
                               .gate_res(mod_txt + 5 * h, S_t, mod_stride, X_txt).split_ws(L.kws);
    DK_TRY(dk_launch_gemm_pair(fc1_img, fc1_txt, st));
    DK_TRY(dk_launch_gemm_pair(fc2_img, fc2_txt, st));
  } else {
    DK_TRY(dk_launch_gemm(fc1_img, st));
    DK_TRY(dk_launch_gemm(fc2_img, st));
  }
  return 0;
}

// UnifiedTransformerBlock i (mmdit.py:693-751), bf16 Linears: parallel attention + MLP
static int single_block_bf16(dk_mmdit* m, const BlockCtx& c, int i, const bf16_t* mod_step, const LaunchCtx& L) {
  const hipStream_t st = L.st;
  const dk_mmdit_config& cf = m->cfg;
  const int h = c.h, S = c.S, M = c.B * c.S, r = cf.mlp_ratio, ldcat = m->ldcat;
  const StreamW& w = m->single[i];
  const bf16_t* mod = block_mod(m, mod_step, 2, i);
  const Rows X = dense(m->X, h), CAT = dense(m->CAT, ldcat);
  // FLUX ControlNet taps (dk_mmdit_set_flux_control_taps): the residual behind the block in front of this one -- single block i - 1, or the last
  // double block -- is added to the image rows of the joint stream in this pass; the text rows take the plain path of the same kernel
  if (const bf16_t* tap = m->tap_behind(cf.depth_multimodal + i - 1))
    DK_TRY(dk_launch_ln_modulate_add_joint(m->X, h, tap, h, m->tap_s(), S, c.S_t, m->XN, h, M, h, mod, mod + h, c.mod_stride, S, M, 0, cf.layer_norm_eps, st));
  else
    DK_TRY(DK_EL(L.dtype, dk_launch_ln_modulate)(m->X, h, m->XN, h, M, h, mod, mod + h, c.mod_stride, S, M, 0, cf.layer_norm_eps, st));
  {  // linear1: [q|k|v] -> QKV, gelu(fc1) -> CAT[:, h:], one pass over the modulated activations
    Linear l1 = Linear(L.dtype, dense(m->XN, h), w.qkv_w, w.qkv_b, dense(m->QKV, 3 * h), M, (3 + r) * h, h, DK_EPI_BIAS).split_ws(L.kws);
    l1.n_split = 3 * h; l1.C2 = m->CAT + h; l1.ldc2 = ldcat; l1.epi2 = DK_EPI_BIAS_GELU;
    if (keys_in_tail(w, nullptr)) set_key_norm(l1, w.kn, w.qn, h, m->D(), c.rope, 0, S);
    DK_TRY(dk_launch_gemm(l1, st));
  }
  if (!keys_in_tail(w, nullptr))
    DK_TRY(DK_EL(L.dtype, dk_launch_qk_norm_rope)(m->QKV, 3 * h, 0, h, M, cf.num_heads, m->D(), w.qn, w.kn, 1e-6f, c.rope, S, S, 0, S, st, fuse_q()));
  DK_TRY(dk_launch_attention(joint_attention(m, c, m->CAT, ldcat, w, nullptr), L.aws, st));
  // x += gate * ([attn | gelu] @ [o_proj | fc2]^T + bias)   (one bias: quirk Q8)
  // (with the split workspace: below 1024 x 1024 the launch is a fraction of a round of the CUs and is cut along K)
  const Linear l2 = Linear(L.dtype, CAT, w.l2_w, w.l2_b, X, M, h, (1 + r) * h, DK_EPI_GATE_RES, ldcat).gate_res(mod + 2 * h, S, c.mod_stride, X).split_ws(L.kws);
  return dk_launch_gemm(l2, st);
}

// ---- fp8_linears: the transformer blocks on the fp8 GEMM (gemm256f8.hip) -------------------------------------------------
// A Linear over MX-fp8 activations.  abuf / sa: the fp8 activation buffer and its scale side array (pitch lda bytes); the GEMM
// reads logical rows through (a_row0, a_seg_len, a_seg_stride): a_row0 a multiple of 128 rows, and either one segment of any length or
// segments of whole 128-row blocks (dk_gemm256f8_eligible; the row order of mmdit_carve provides it for every token count).
// Every one carries the engine's split workspace (the K split of small launches).
static GemmF8Params f8_params(const dk_mmdit* m, const unsigned char* abuf, const unsigned char* sa, int lda, int a_row0, int a_seg_len,
                              int a_seg_stride, const unsigned char* W, int ldw, const float* ws, const bf16_t* bias, int M, int N, int K,
                              int epi) {
  GemmF8Params p;
  memset(&p, 0, sizeof(p));
  p.A = abuf + (size_t)a_row0 * lda; p.SA = sa; p.W = W; p.wscale = ws; p.bias = bias;
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldw = ldw;
  p.a_seg_len = a_seg_len; p.a_seg_stride = a_seg_stride; p.a_row0 = a_row0; p.sa_nblk = m->nblk;
  p.epi = epi;
  if (m->GWS) { p.workspace = m->GWS; p.workspace_bytes = dk_gemm_split_workspace_bytes(); }
  return p;
}
static void f8_out_bf16(GemmF8Params& p, Rows C) {
  p.C = C.p; p.ldc = C.ld; p.c_seg_len = C.seg_len > 0 ? C.seg_len : p.M; p.c_seg_stride = C.seg_stride; p.c_mx8 = 0;
  p.r_seg_len = p.M; p.gate_seg_len = p.M;
}
// the MX-fp8 output of fc1: rows [c_row0, c_row0 + M) of HC8 (pitch ldh8), scales in SHID
static void f8_out_hid8(GemmF8Params& p, const dk_mmdit* m, int c_row0) {
  p.C = m->HC8 + (size_t)c_row0 * m->ldh8; p.ldc = m->ldh8; p.c_seg_len = p.M; p.c_mx8 = 1;
  p.SC = m->SHID; p.sc_nblk = m->nblk; p.c_row0 = c_row0; p.sc_kb0 = 0;
  p.r_seg_len = p.M; p.gate_seg_len = p.M;
}

// MultiModalTransformerBlock i on the fp8 GEMM: the streams' Linears as pairs of one launch (dk_launch_gemm256f8)
static int double_block_fp8(dk_mmdit* m, const BlockCtx& c, int i, const bf16_t* mod_step, const LaunchCtx& L) {
  const hipStream_t st = L.st;
  const dk_mmdit_config& cf = m->cfg;
  const int h = c.h, S = c.S, S_t = c.S_t, S_i = c.S_i, Mi = c.Mi, Mt = c.Mt, T0 = c.T0, r = cf.mlp_ratio, ldh8 = m->ldh8, mod_stride = c.mod_stride;
  const bf16_t *mod_img = block_mod(m, mod_step, 0, i), *mod_txt = block_mod(m, mod_step, 1, i);
  const StreamW &wi = m->dimg[i], &wt = m->dtxt[i];
  const bool txt_post = !m->txt_skipped(i);
  const Rows X_img = c.X_img, X_txt = c.X_txt;
  // pre_sdpa (mmdit.py:440-519): LN-modulate -> MX-fp8, q/k/v projection, QK-norm (+ RoPE)
  DK_TRY(dk_launch_ln_modulate2_mx8(X_img.p, Mi, mod_img, mod_img + h, S_i, c.xn_img, X_txt.p, Mt, mod_txt, mod_txt + h, S_t, c.xn_txt, h, h, mod_stride,
                                    S, cf.layer_norm_eps, st));
  const bool kf = keys_in_tail(wi, &wt);
  {
    GemmF8Params qi = f8_params(m, m->XN8, m->SXN, h, 0, Mi, 0, wi.qkv_w8, h, wi.qkv_ws, wi.qkv_b, Mi, 3 * h, h, DK_EPI_BIAS);
    GemmF8Params qt = f8_params(m, m->XN8, m->SXN, h, T0, Mt, 0, wt.qkv_w8, h, wt.qkv_ws, wt.qkv_b, Mt, 3 * h, h, DK_EPI_BIAS);
    f8_out_bf16(qi, m->img(m->QKV, 3 * h));
    f8_out_bf16(qt, m->txt(m->QKV, 3 * h));
    if (kf) {
      set_key_norm(qi, wi.kn, wi.qn, h, m->D(), c.rope, S_t, S_i);
      set_key_norm(qt, wt.kn, wt.qn, h, m->D(), c.rope, 0, S_t);
    }
    DK_TRY(dk_launch_gemm256f8(qi, &qt, st));
  }
  if (!kf)
    DK_TRY(dk_launch_qk_norm_rope2(m->QKV + (size_t)S_t * 3 * h, Mi, wi.qn, wi.kn, S_i, S_t, m->QKV, Mt, wt.qn, wt.kn, S_t, 0, 3 * h, 0, h,
                                   cf.num_heads, m->D(), 1e-6f, c.rope, S, st, fuse_q()));
  AttnParams ap = joint_attention(m, c, m->ATT, h, wt, &wi, m->ATT8, m->SATT, h);  // (ATT8: the o-projection's operand)
  if (c.att_split) { ap.o8_split = S_t; ap.o8_txt_row0 = T0; }
  DK_TRY(dk_launch_attention(ap, L.aws, st));
  // post_sdpa (mmdit.py:537-548): residual += gate_attn * o_proj(attn)
  {
    GemmF8Params oi = c.att_split ? f8_params(m, m->ATT8, m->SATT, h, 0, Mi, 0, wi.o_w8, h, wi.o_ws, wi.o_b, Mi, h, h, DK_EPI_GATE_RES)
                                  : f8_params(m, m->ATT8, m->SATT, h, S_t, S_i, S, wi.o_w8, h, wi.o_ws, wi.o_b, Mi, h, h, DK_EPI_GATE_RES);
    f8_out_bf16(oi, X_img);
    set_gate_res(oi, mod_img + 2 * h, S_i, mod_stride, X_img);
    GemmF8Params ot = c.att_split ? f8_params(m, m->ATT8, m->SATT, h, T0, Mt, 0, wt.o_w8, h, wt.o_ws, wt.o_b, Mt, h, h, DK_EPI_GATE_RES)
                                  : f8_params(m, m->ATT8, m->SATT, h, 0, S_t, S, wt.o_w8, h, wt.o_ws, wt.o_b, Mt, h, h, DK_EPI_GATE_RES);
    f8_out_bf16(ot, X_txt);
    set_gate_res(ot, mod_txt + 2 * h, S_t, mod_stride, X_txt);
    DK_TRY(dk_launch_gemm256f8(oi, txt_post ? &ot : nullptr, st));
  }
  // residual += gate_mlp * fc2(gelu(fc1(LN-mod(residual)))); the MLP hidden leaves fc1 as MX-fp8
  if (txt_post)
    DK_TRY(dk_launch_ln_modulate2_mx8(X_img.p, Mi, mod_img + 3 * h, mod_img + 4 * h, S_i, c.xn_img, X_txt.p, Mt, mod_txt + 3 * h, mod_txt + 4 * h, S_t,
                                      c.xn_txt, h, h, mod_stride, S, cf.layer_norm_eps, st));
  else
    DK_TRY(dk_launch_ln_modulate_mx8(X_img.p, h, Mi, h, mod_img + 3 * h, mod_img + 4 * h, mod_stride, S_i, S_i, S, cf.layer_norm_eps, c.xn_img, st));
  GemmF8Params f1i = f8_params(m, m->XN8, m->SXN, h, 0, Mi, 0, wi.fc1_w8, h, wi.fc1_ws, wi.fc1_b, Mi, r * h, h, DK_EPI_BIAS_GELU);
  f8_out_hid8(f1i, m, 0);
  GemmF8Params f2i = f8_params(m, m->HC8, m->SHID, ldh8, 0, Mi, 0, wi.fc2_w8, ldh8, wi.fc2_ws, wi.fc2_b, Mi, h, r * h, DK_EPI_GATE_RES);
  f8_out_bf16(f2i, X_img);
  set_gate_res(f2i, mod_img + 5 * h, S_i, mod_stride, X_img);
  GemmF8Params f1t = f8_params(m, m->XN8, m->SXN, h, T0, Mt, 0, wt.fc1_w8, h, wt.fc1_ws, wt.fc1_b, Mt, r * h, h, DK_EPI_BIAS_GELU);
  f8_out_hid8(f1t, m, T0);
  GemmF8Params f2t = f8_params(m, m->HC8, m->SHID, ldh8, T0, Mt, 0, wt.fc2_w8, ldh8, wt.fc2_ws, wt.fc2_b, Mt, h, r * h, DK_EPI_GATE_RES);
  f8_out_bf16(f2t, X_txt);
  set_gate_res(f2t, mod_txt + 5 * h, S_t, mod_stride, X_txt);
  DK_TRY(dk_launch_gemm256f8(f1i, txt_post ? &f1t : nullptr, st));
  return dk_launch_gemm256f8(f2i, txt_post ? &f2t : nullptr, st);
}

// UnifiedTransformerBlock i on the fp8 GEMM
static int single_block_fp8(dk_mmdit* m, const BlockCtx& c, int i, const bf16_t* mod_step, const LaunchCtx& L) {
  const hipStream_t st = L.st;
  const dk_mmdit_config& cf = m->cfg;
  const int h = c.h, S = c.S, M = c.B * c.S, r = cf.mlp_ratio, ldcat8 = m->ldcat8;
  const StreamW& w = m->single[i];
  const bf16_t* mod = block_mod(m, mod_step, 2, i);
  const Rows X = dense(m->X, h);
  DK_TRY(dk_launch_ln_modulate_mx8(m->X, h, M, h, mod, mod + h, c.mod_stride, S, M, 0, cf.layer_norm_eps, c.xn_all, st));
  {  // linear1: [q|k|v] -> QKV (bf16), gelu(fc1) -> CAT8[:, h:] (MX-fp8), one pass over the modulated activations
    GemmF8Params l1 = f8_params(m, m->XN8, m->SXN, h, 0, M, 0, w.qkv_w8, h, w.qkv_ws, w.qkv_b, M, (3 + r) * h, h, DK_EPI_BIAS);
    f8_out_bf16(l1, dense(m->QKV, 3 * h));
    l1.n_split = 3 * h; l1.C2 = m->HC8 + h; l1.ldc2 = ldcat8; l1.epi2 = DK_EPI_BIAS_GELU; l1.c2_mx8 = 1;
    l1.SC = m->SCAT; l1.sc_nblk = m->nblk; l1.c_row0 = 0; l1.sc_kb0 = h / 32;
    if (keys_in_tail(w, nullptr)) set_key_norm(l1, w.kn, w.qn, h, m->D(), c.rope, 0, S);
    DK_TRY(dk_launch_gemm256f8(l1, nullptr, st));
  }
  if (!keys_in_tail(w, nullptr))
    DK_TRY(dk_launch_qk_norm_rope(m->QKV, 3 * h, 0, h, M, cf.num_heads, m->D(), w.qn, w.kn, 1e-6f, c.rope, S, S, 0, S, st, fuse_q()));
  // (the MX-fp8 copy: the [attn | gelu] operand of linear2, columns [0, h))
  DK_TRY(dk_launch_attention(joint_attention(m, c, m->ATT, h, w, nullptr, m->HC8, m->SCAT, ldcat8), L.aws, st));
  // x += gate * ([attn | gelu] @ [o_proj | fc2]^T + bias)   (one bias: quirk Q8)
  GemmF8Params l2 = f8_params(m, m->HC8, m->SCAT, ldcat8, 0, M, 0, w.l2_w8, ldcat8, w.l2_ws, w.l2_b, M, h, (1 + r) * h, DK_EPI_GATE_RES);
  f8_out_bf16(l2, X);
  set_gate_res(l2, mod + 2 * h, S, c.mod_stride, X);
  return dk_launch_gemm256f8(l2, nullptr, st);
}

// Blocks [first, first + count) of the global order (double blocks 0 .. depth_multimodal - 1, then single blocks) on the joint residual
// stream m->X: the bf16 double blocks of the precision policy on the bf16 path, everything else on the model's own.  rows: the batch rows
// [0, rows) they run on, the launches of a batch of that size on the same buffers (0: the prepared batch)
static int mmdit_blocks(dk_mmdit* m, const bf16_t* mod_step, int first, int count, const LaunchCtx& L, int rows = 0) {
  const BlockCtx c = block_ctx(m, rows > 0 ? rows : m->B);
  const int n_double = m->cfg.depth_multimodal;
  for (int g = first; g < first + count; ++g) {
    const bool f8 = m->fp8() && g >= m->n_bf16();
    if (g < n_double)
      DK_TRY((f8 ? double_block_fp8 : double_block_bf16)(m, c, g, mod_step, L));
    else
      DK_TRY((f8 ? single_block_fp8 : single_block_bf16)(m, c, g - n_double, mod_step, L));
  }
  return 0;
}

// the embedders of a forward call: text rows and image rows of the joint stream m->X (rows: as in mmdit_blocks -- the operands' rows behind
// them are not read)
static int mmdit_embed(dk_mmdit* m, const void* tokens_in, const void* text, const LaunchCtx& L, int rows = 0) {
  const hipStream_t st = L.st;
  const dk_mmdit_config& c = m->cfg;
  const int h = m->h(), B = rows > 0 ? rows : m->B, S = m->S, S_t = m->S_t, S_i = m->S_i, F = m->F();
  DK_TRY(need_reference(m));
  DK_TRY(need_condition(m));
  // context_embedder (mmdit.py:195): text rows of the joint stream -- recomputed from `text`, or copied from the
  // step-invariant result of dk_mmdit_cache_context when `text` is null
  if (text != nullptr) {
    const int T = c.token_level_text_embed_dim;  // (no split workspace)
    DK_TRY(dk_launch_gemm(Linear(L.dtype, dense((const bf16_t*)text, T), m->ctx_w, m->ctx_b, m->txt(m->X, h), B * S_t, h, T, DK_EPI_BIAS), st));
  } else {
    DK_REQUIRE(m->ctx_ready, "forward without text needs dk_mmdit_cache_context first");
    DK_CHECK_HIP(hipMemcpy2DAsync(m->X, (size_t)S * h * 2, m->CTXE, (size_t)S_t * h * 2, (size_t)S_t * h * 2, B, hipMemcpyDeviceToDevice, st));
  }
  // x_embedder (+ learned positional embedding) (mmdit.py:197-206): image rows
  // (no split workspace; the positional rows repeat per image: one segment of S_i rows, stride 0)
  // (with a condition width: the latent columns of the [h, F + cond_f] weight, and the condition's step-invariant share, CONDE, in the
  // residual slot the positional table leaves free -- one segment per batch row)
  // (a control-net engine: CONDE = POS + pos_embed_input(control tokens) in the slot of POS -- x_embedder's own [h, F] weight, pitch F; of FLUX
  // geometry: CONDE = controlnet_x_embedder(control tokens), in the slot that a model without a positional table leaves free)
  const bool cond = m->cond_f > 0;
  DK_REQUIRE(!m->control_net || m->ctrl_ready, "a control-net engine needs dk_mmdit_cache_control_image after dk_mmdit_prepare");
  const Rows res = cond || m->control_net ? Rows{m->CONDE, h, S_i, S_i} : Rows{c.use_pos_embed ? m->POS : nullptr, h, S_i, 0};
  DK_TRY(dk_launch_gemm(Linear(L.dtype, dense((const bf16_t*)tokens_in, F), m->xemb_w, m->xemb_b, m->own(m->X, h), B * S_i, h, F,
                               cond || m->control_net || c.use_pos_embed ? DK_EPI_RES : DK_EPI_BIAS, cond ? F + m->cond_f : 0)
                            .gate_res(nullptr, 0, 0, res),
                        st));
  // the reference image's rows behind them: the step-invariant result of dk_mmdit_cache_reference
  if (m->S_r > 0)
    DK_CHECK_HIP(hipMemcpy2DAsync(m->X + (size_t)(S_t + S_i) * h, (size_t)S * h * 2, m->REFE, (size_t)m->S_r * h * 2, (size_t)m->S_r * h * 2, B,
                                  hipMemcpyDeviceToDevice, st));
  return 0;
}

// ---- skip-layer guidance (include/dk_hip.h) -----------------------------------------------------------------------------------------
extern "C" int dk_mmdit_set_skip_layers(dk_mmdit* m, const int32_t* blocks, int32_t n_blocks, int32_t fork_rows) {
  DK_REQUIRE(m != nullptr, "null handle");
  DK_REQUIRE(n_blocks >= 0 && fork_rows >= 0, "skip layers: n_blocks and fork_rows must not be negative");
  DK_REQUIRE((n_blocks == 0) == (fork_rows == 0), "skip layers: n_blocks and fork_rows are both zero (off) or both positive");
  if (n_blocks == 0) {
    m->skip.clear();
    if (!m->perturbed()) m->fork_rows = 0;  // (the fork is shared: switching this feature off leaves the other's rows alone)
    return 0;
  }
  DK_REQUIRE(blocks != nullptr, "null argument");
  DK_REQUIRE(m->cfg.depth_unified == 0, "skip layers are the SD3 family's: depth_unified must be 0");
  DK_REQUIRE(m->cfg.fp8_linears == 0, "skip layers cannot be set on an engine with fp8_linears");
  DK_REQUIRE(m->ref_h == 0 && m->ref_w == 0 && m->cond_f == 0, "skip layers cannot be set while a reference grid or a condition width is set");
  DK_REQUIRE(m->ip_n == 0, "skip layers cannot be set on an engine with an IP-Adapter (dk_mmdit_set_ip_adapter)");
  DK_REQUIRE(!m->perturbed(), "skip layers cannot be set while perturbed attention is set (dk_mmdit_set_perturbed_attention): there is one fork");
  DK_REQUIRE(!m->control_net && !m->tapped(), "skip layers cannot be set on a control-net engine or while control taps are set: the fork rows would need taps of their own");
  std::vector<int32_t> v(blocks, blocks + n_blocks);
  std::sort(v.begin(), v.end());
  DK_REQUIRE(v.front() >= 0 && v.back() < m->cfg.depth_multimodal, "skip layers: every block must lie in [0, depth_multimodal)");
  DK_REQUIRE(std::adjacent_find(v.begin(), v.end()) == v.end(), "skip layers: a block is named twice (duplicate)");
  m->skip = v;
  m->fork_rows = fork_rows;
  return 0;
}
extern "C" int dk_mmdit_set_perturbed_attention(dk_mmdit* m, const int32_t* blocks, int32_t n_blocks, int32_t fork_rows) {
  DK_REQUIRE(m != nullptr, "null handle");
  DK_REQUIRE(n_blocks >= 0 && fork_rows >= 0, "perturbed attention: n_blocks and fork_rows must not be negative");
  DK_REQUIRE((n_blocks == 0) == (fork_rows == 0), "perturbed attention: n_blocks and fork_rows are both zero (off) or both positive");
  if (n_blocks == 0) {
    if (m->perturbed()) m->fork_rows = 0;
    m->pag.clear();
    return 0;
  }
  DK_REQUIRE(blocks != nullptr, "null argument");
  DK_REQUIRE(m->cfg.depth_unified == 0, "perturbed attention is the SD3 family's: depth_unified must be 0");
  DK_REQUIRE(m->cfg.fp8_linears == 0, "perturbed attention cannot be set on an engine with fp8_linears");
  DK_REQUIRE(m->ref_h == 0 && m->ref_w == 0 && m->cond_f == 0, "perturbed attention cannot be set while a reference grid or a condition width is set");
  DK_REQUIRE(m->ip_n == 0, "perturbed attention cannot be set on an engine with an IP-Adapter (dk_mmdit_set_ip_adapter)");
  DK_REQUIRE(!m->slg(), "perturbed attention cannot be set while skip layers are set (dk_mmdit_set_skip_layers): there is one fork");
  DK_REQUIRE(!m->control_net && !m->tapped(), "perturbed attention cannot be set on a control-net engine or while control taps are set: the fork rows would need taps of their own");
  std::vector<int32_t> v(blocks, blocks + n_blocks);
  std::sort(v.begin(), v.end());
  DK_REQUIRE(v.front() >= 0 && v.back() < m->cfg.depth_multimodal, "perturbed attention: every block must lie in [0, depth_multimodal)");
  DK_REQUIRE(std::adjacent_find(v.begin(), v.end()) == v.end(), "perturbed attention: a block is named twice (duplicate)");
  m->pag = v;
  m->fork_rows = fork_rows;
  return 0;
}
static int no_skip_layers(const dk_mmdit* m, const char* entry) {
  if (!m->slg() && !m->perturbed()) return 0;
  dk_set_error(std::string(entry) + (m->slg() ? " cannot run while skip layers are set (dk_mmdit_set_skip_layers)" :
                                                " cannot run while perturbed attention is set (dk_mmdit_set_perturbed_attention)") +
               ": only dk_mmdit_forward forks the row group");
  return -1;
}

// ---- SD3 ControlNet (include/dk_hip.h) --------------------------------------------------------------------------------------------------
static bool sd3_geometry(const dk_mmdit* m) { return m->cfg.use_pos_embed != 0 && m->cfg.depth_unified == 0 && m->cfg.fp8_linears == 0; }
extern "C" int dk_mmdit_set_control_net(dk_mmdit* m, int32_t on) {
  DK_REQUIRE(m != nullptr, "null handle");
  DK_REQUIRE(m->named.empty() && !m->prepared, "dk_mmdit_set_control_net must precede the first dk_mmdit_bind");
  if (on) {
    DK_REQUIRE(sd3_geometry(m), "a control-net engine is the SD3 family's: use_pos_embed != 0, depth_unified == 0 and fp8_linears == 0");
    DK_REQUIRE(m->n_dual == 0 && m->ref_h == 0 && m->ref_w == 0 && m->cond_f == 0,
               "a control-net engine cannot have dual attention blocks, a reference grid or a condition width");
    DK_REQUIRE(!m->bc_on && !m->slg() && !m->perturbed() && !m->tapped(),
               "a control-net engine cannot have a block cache, skip layers, perturbed attention or control taps of its own");
  }
  m->control_net = on != 0;
  m->control_flux = false;
  m->ctrl_ready = false;
  return 0;
}
// the ControlNet of FLUX geometry (diffusers' FluxControlNetModel): double and single blocks, RoPE, no positional table
extern "C" int dk_mmdit_set_flux_control_net(dk_mmdit* m, int32_t on) {
  DK_REQUIRE(m != nullptr, "null handle");
  DK_REQUIRE(m->named.empty() && !m->prepared, "dk_mmdit_set_flux_control_net must precede the first dk_mmdit_bind");
  if (on) {
    DK_REQUIRE(m->cfg.use_rope != 0 && m->cfg.use_pos_embed == 0, "a FLUX control-net engine is the FLUX family's: use_rope != 0 and use_pos_embed == 0");
    DK_REQUIRE(m->cfg.fp8_linears == 0, "a FLUX control-net engine cannot have fp8 Linears");
    DK_REQUIRE(m->dtype == DK_DTYPE_BF16, "a FLUX control-net engine needs bf16 activations");
    DK_REQUIRE(m->cfg.depth_multimodal >= 1 && m->cfg.depth_unified >= 0, "a FLUX control-net engine needs at least one double block");
    DK_REQUIRE(m->ip_n == 0, "a FLUX control-net engine cannot have an IP-Adapter (dk_mmdit_set_ip_adapter)");
    DK_REQUIRE(m->n_dual == 0 && m->ref_h == 0 && m->ref_w == 0 && m->cond_f == 0,
               "a control-net engine cannot have dual attention blocks, a reference grid or a condition width");
    DK_REQUIRE(!m->bc_on && !m->slg() && !m->perturbed() && !m->tapped(),
               "a control-net engine cannot have a block cache, skip layers, perturbed attention or control taps of its own");
  }
  m->control_net = m->control_flux = on != 0;
  m->ctrl_ready = false;
  return 0;
}
extern "C" int dk_mmdit_cache_control_image(dk_mmdit* m, const void* ctrl_tokens, int32_t per_image, void* stream) {
  DK_REQUIRE(m && m->prepared && ctrl_tokens, "prepare must precede cache_control_image");
  DK_REQUIRE(m->control_net, "cache_control_image needs a control-net engine: dk_mmdit_set_control_net before the first dk_mmdit_bind");
  const int h = m->h(), F = m->F(), S_i = m->S_i;
  // pos_embed_input as x_embedder in mmdit_embed (no split workspace) with the positional rows as residual, one launch per batch row: a shared
  // control image gives every batch row the bits a per-image copy of it would
  // (FLUX geometry: CONDE[b] = controlnet_x_embedder(ctrl_tokens[b]) -- there is no positional table, so no residual operand)
  for (int b = 0; b < m->B; ++b) {
    const bf16_t* src = (const bf16_t*)ctrl_tokens + (per_image ? (size_t)b * S_i * F : 0);
    const Rows out = dense(m->CONDE + (size_t)b * S_i * h, h);
    if (m->control_flux)
      DK_TRY(dk_launch_gemm(Linear(m->dtype, dense(src, F), m->cxe_w, m->cxe_b, out, S_i, h, F, DK_EPI_BIAS), S_(stream)));
    else
      DK_TRY(dk_launch_gemm(Linear(m->dtype, dense(src, F), m->cin_w, m->cin_b, out, S_i, h, F, DK_EPI_RES).gate_res(nullptr, 0, 0, Rows{m->POS, h, S_i, 0}),
                            S_(stream)));
  }
  m->ctrl_ready = true;
  return 0;
}
extern "C" int dk_mmdit_set_control_taps(dk_mmdit* m, const void* taps, int32_t n_taps, float scale) {
  DK_REQUIRE(m != nullptr, "null handle");
  if (taps == nullptr || n_taps == 0) {
    m->taps = nullptr; m->n_taps = m->n_dtaps = m->n_staps = 0; m->tap_scale = 0.f;  // (off: taps of either kind)
    return 0;
  }
  DK_REQUIRE(sd3_geometry(m), "control taps are the SD3 family's: use_pos_embed != 0, depth_unified == 0 and fp8_linears == 0");
  DK_REQUIRE(!m->control_net, "control taps cannot be set on a control-net engine (dk_mmdit_set_control_net): it writes taps, the main engine reads them");
  DK_REQUIRE(n_taps >= 1 && n_taps <= m->cfg.depth_multimodal, "control taps: n_taps must lie in [1, depth_multimodal]");
  DK_REQUIRE(((uintptr_t)taps & 15) == 0, "control taps must be 16-byte aligned");
  DK_REQUIRE(m->n_dual == 0, "control taps cannot be set on an engine with dual attention blocks");
  DK_REQUIRE(!m->bc_on, "control taps cannot be set while the block cache is on (dk_mmdit_set_block_cache)");
  DK_REQUIRE(!m->slg() && !m->perturbed(), "control taps cannot be set while skip layers or perturbed attention are set: the fork rows would need taps of their own");
  DK_REQUIRE(m->ref_h == 0 && m->ref_w == 0 && m->cond_f == 0, "control taps cannot be set while a reference grid or a condition width is set");
  // diffusers' rule in integers: floor(g n / depth) must be int(g / (depth / n)) in double for every block that takes a tap
  const int depth = m->cfg.depth_multimodal;
  const double interval = (double)depth / (double)n_taps;
  for (int g = 0; g + 1 < depth; ++g)
    DK_REQUIRE((int)((long)g * n_taps / depth) == (int)((double)g / interval), "control taps: the integer tap index disagrees with int(g / (depth / n_taps))");
  m->taps = (const bf16_t*)taps; m->n_taps = n_taps; m->tap_scale = scale;
  return 0;
}
// FLUX taps on the MAIN engine: taps [n_double_taps + n_single_taps, B, S_i, h], the double blocks' first
extern "C" int dk_mmdit_set_flux_control_taps(dk_mmdit* m, const void* taps, int32_t n_double_taps, int32_t n_single_taps, float scale) {
  DK_REQUIRE(m != nullptr, "null handle");
  if (taps == nullptr || (n_double_taps == 0 && n_single_taps == 0)) {
    m->taps = nullptr; m->n_taps = m->n_dtaps = m->n_staps = 0; m->tap_scale = 0.f;  // (off: taps of either kind)
    return 0;
  }
  const int nd = m->cfg.depth_multimodal, ns = m->cfg.depth_unified;
  DK_REQUIRE(m->cfg.use_rope != 0 && m->cfg.use_pos_embed == 0, "FLUX control taps are the FLUX family's: use_rope != 0 and use_pos_embed == 0");
  DK_REQUIRE(m->cfg.fp8_linears == 0, "FLUX control taps cannot be set on an engine with fp8 Linears: the fp8 LayerNorm kernels take no tap");
  DK_REQUIRE(m->dtype == DK_DTYPE_BF16, "FLUX control taps need bf16 activations");
  DK_REQUIRE(!m->control_net, "control taps cannot be set on a control-net engine: it writes taps, the main engine reads them");
  DK_REQUIRE(m->n_taps == 0, "FLUX control taps cannot be set while SD3 control taps are set (dk_mmdit_set_control_taps)");
  DK_REQUIRE(m->ip_n == 0, "FLUX control taps cannot be set on an engine with an IP-Adapter (dk_mmdit_set_ip_adapter): the LayerNorm launch has one tap operand");
  DK_REQUIRE(n_double_taps >= 0 && n_double_taps <= nd, "FLUX control taps: n_double_taps must lie in [0, depth_multimodal]");
  DK_REQUIRE(n_single_taps >= 0 && n_single_taps <= ns, "FLUX control taps: n_single_taps must lie in [0, depth_unified]");
  DK_REQUIRE(((uintptr_t)taps & 15) == 0, "control taps must be 16-byte aligned");
  DK_REQUIRE(m->n_dual == 0, "control taps cannot be set on an engine with dual attention blocks");
  DK_REQUIRE(!m->bc_on, "FLUX control taps cannot be set while the block cache is on (dk_mmdit_set_block_cache)");
  DK_REQUIRE(!m->slg() && !m->perturbed(), "control taps cannot be set while skip layers or perturbed attention are set: the fork rows would need taps of their own");
  DK_REQUIRE(m->ref_h == 0 && m->ref_w == 0, "FLUX control taps cannot be set while a reference grid is set");
  DK_REQUIRE(m->cond_f == 0, "FLUX control taps cannot be set while a condition width is set");
  // diffusers' rule in integers: g / ceil(depth / n) must be int(g // np.ceil(depth / n)) in double for every block of the kind
  for (int kind = 0; kind < 2; ++kind) {
    const int depth = kind == 0 ? nd : ns, n = kind == 0 ? n_double_taps : n_single_taps;
    if (n == 0) continue;
    const double interval = std::ceil((double)depth / (double)n);
    for (int g = 0; g < depth; ++g) {
      const int idx = dk_mmdit::flux_tap_of(g, n, depth);
      DK_REQUIRE(idx == (int)std::floor((double)g / interval) && idx >= 0 && idx < n,
                 "FLUX control taps: the integer tap index disagrees with int(g // ceil(depth / n))");
    }
  }
  m->taps = (const bf16_t*)taps; m->n_dtaps = n_double_taps; m->n_staps = n_single_taps; m->tap_scale = scale;
  return 0;
}
// what the entries other than dk_mmdit_forward answer while taps are set, and the forward entries on a control-net engine
static int no_control_taps(const dk_mmdit* m, const char* entry) {
  if (!m->tapped()) return 0;
  dk_set_error(std::string(entry) + " cannot run while control taps are set (" + (m->flux_tapped() ? "dk_mmdit_set_flux_control_taps" : "dk_mmdit_set_control_taps") +
               "): only dk_mmdit_forward adds them");
  return -1;
}
static int no_control_net(const dk_mmdit* m, const char* entry) {
  if (!m->control_net) return 0;
  dk_set_error(std::string(entry) + " cannot run on a control-net engine (dk_mmdit_set_control_net): it has no final layer, use dk_mmdit_control_forward");
  return -1;
}
extern "C" int dk_mmdit_control_forward(dk_mmdit* m, const void* tokens_in, const void* text, int32_t step_index, void* taps_out, void* stream) {
  DK_REQUIRE(m && m->prepared && m->mod_ready, "prepare + cache_modulation_params must precede control_forward");
  DK_REQUIRE(m->control_net, "control_forward needs a control-net engine: dk_mmdit_set_control_net before the first dk_mmdit_bind");
  DK_REQUIRE(tokens_in && taps_out, "null argument");
  DK_REQUIRE(step_index >= 0 && step_index < m->n_t, "step index out of range");
  const LaunchCtx L = m->ctx(stream);
  const int h = m->h(), Mi = m->B * m->S_i;
  const bf16_t* mod_step = m->MOD + (size_t)step_index * m->B * m->mod_rows() * h;
  DK_TRY(mmdit_embed(m, tokens_in, text, L, 0));
  // (FLUX geometry: the single blocks follow in the global order, and behind single block j - depth_multimodal the tap Linear reads the image
  // rows of the joint stream -- the same segmented rows)
  for (int j = 0; j < (int)m->tap_w.size(); ++j) {
    DK_TRY(mmdit_blocks(m, mod_step, j, 1, L));
    // taps_out[j] = controlnet_blocks.j(image rows): the segmented rows of the stream in, dense [B S_i, h] out
    DK_TRY(dk_launch_gemm(Linear(L.dtype, m->own(m->X, h), m->tap_w[j], m->tap_b[j], dense((bf16_t*)taps_out + (size_t)j * Mi * h, h), Mi, h, h, DK_EPI_BIAS)
                              .split_ws(L.kws), L.st));
  }
  return 0;
}

// ---- FLUX IP-Adapter (include/dk_hip.h) -------------------------------------------------------------------------------------------------
extern "C" int dk_mmdit_set_ip_adapter(dk_mmdit* m, int32_t n_tokens, int32_t token_dim) {
  DK_REQUIRE(m != nullptr, "null handle");
  DK_REQUIRE(!m->resolved && !m->prepared, "dk_mmdit_set_ip_adapter is legal only before the weights are resolved (the first dk_mmdit_prepare)");
  if (n_tokens != 0 || token_dim != 0) {
    DK_REQUIRE(m->cfg.use_rope != 0 && m->cfg.use_pos_embed == 0 && m->cfg.depth_multimodal >= 1,
               "an IP-Adapter is the FLUX family's: use_rope != 0, use_pos_embed == 0 and at least one double block (SD3 geometry is refused)");
    DK_REQUIRE(m->cfg.fp8_linears == 0, "an IP-Adapter cannot be set on an engine with fp8 Linears: the fp8 LayerNorm kernels take no tap");
    DK_REQUIRE(m->dtype == DK_DTYPE_BF16, "an IP-Adapter needs bf16 activations");
    DK_REQUIRE(m->D() == 128 && m->cfg.use_qk_norm != 0, "an IP-Adapter needs head_dim 128 and QK-norm weights (its queries are the block's QK-normed image queries)");
    DK_REQUIRE(!m->control_net, "an IP-Adapter cannot be set on a control-net engine");
    DK_REQUIRE(!m->tapped(), "an IP-Adapter cannot be set while control taps are set: the LayerNorm launch has one tap operand");
    DK_REQUIRE(!m->bc_on, "an IP-Adapter cannot be set while the block cache is on (dk_mmdit_set_block_cache)");
    DK_REQUIRE(m->ref_h == 0 && m->ref_w == 0, "an IP-Adapter cannot be set while a reference grid is set");
    DK_REQUIRE(m->cond_f == 0, "an IP-Adapter cannot be set while a condition width is set");
    DK_REQUIRE(!m->slg() && !m->perturbed() && m->n_dual == 0, "an IP-Adapter cannot be set with skip layers, perturbed attention or dual attention blocks");
    DK_REQUIRE(n_tokens >= 1 && n_tokens <= 16, "an IP-Adapter has between 1 and 16 image-prompt tokens per image");
    DK_REQUIRE(token_dim > 0 && token_dim % 64 == 0 && token_dim <= (1 << 16), "the IP-Adapter's token width must be a positive multiple of 64");
  }
  m->ip_n = n_tokens; m->ip_c = token_dim;
  m->ip_ready = false;
  return 0;
}
extern "C" int dk_mmdit_cache_ip_tokens(dk_mmdit* m, const void* tokens, int32_t per_image, void* stream) {
  DK_REQUIRE(m && m->prepared && tokens, "prepare must precede cache_ip_tokens");
  DK_REQUIRE(m->ip_n > 0, "cache_ip_tokens needs an IP-Adapter: dk_mmdit_set_ip_adapter before the first dk_mmdit_prepare");
  const int N = m->ip_n, Ck = m->ip_c, ldkv = m->cfg.depth_multimodal * 2 * m->h();
  // every block's keys and values from ONE matrix; one launch per batch row (M = N rows), as the other hoists do: a shared prompt gives every
  // batch row the bits a per-image copy of it would.  No split workspace.  A previous cache is overwritten
  for (int b = 0; b < m->B; ++b) {
    const bf16_t* src = (const bf16_t*)tokens + (per_image ? (size_t)b * N * Ck : 0);
    DK_TRY(dk_launch_gemm(Linear(m->dtype, dense(src, Ck), m->ipkv_w, m->ipkv_b, dense(m->IPKV + (size_t)b * N * ldkv, ldkv), N, ldkv, Ck, DK_EPI_BIAS), S_(stream)));
  }
  m->ip_ready = true;
  return 0;
}
extern "C" int dk_mmdit_set_ip_scale(dk_mmdit* m, float scale) {
  DK_REQUIRE(m != nullptr, "null handle");
  if (scale != 0.f) {
    DK_REQUIRE(m->ip_n > 0, "set_ip_scale needs an IP-Adapter: dk_mmdit_set_ip_adapter before the first dk_mmdit_prepare");
    DK_REQUIRE(std::isfinite(scale), "the IP-Adapter's scale must be finite");
    DK_REQUIRE(!m->tapped(), "the IP-Adapter cannot be switched on while control taps are set: the LayerNorm launch has one tap operand");
  }
  m->ip_scale = scale;
  return 0;
}
// what the entries other than dk_mmdit_forward answer while the adapter is active (set, with a scale other than 0)
static int no_ip_adapter(const dk_mmdit* m, const char* entry) {
  if (!m->ip_active()) return 0;
  dk_set_error(std::string(entry) + " cannot run while the IP-Adapter is active (dk_mmdit_set_ip_adapter with a scale other than 0): only dk_mmdit_forward runs it");
  return -1;
}
// ... and what dk_mmdit_forward asks before its first launch: the cache, and image queries that stay raw in QKV behind the q / k / v projection
static int need_ip_adapter(const dk_mmdit* m) {
  if (!m->ip_active()) return 0;
  DK_REQUIRE(m->ip_ready, "an engine with an active IP-Adapter needs dk_mmdit_cache_ip_tokens after dk_mmdit_prepare");
  DK_REQUIRE(fuse_q() != 0, "the IP-Adapter reads the image queries raw from QKV: dk_tune_set(\"attn_fuse_q\", 0) norms and rotates them there in a pass of its own");
  // (queries_in_tail is what double_block_bf16's launches follow: with the keys' fused tail off -- "gemm_fuse_k" 0 -- "gemm_fuse_q" 1 finishes nothing
  // and the queries stay raw)
  for (int i = 0; i < m->cfg.depth_multimodal; ++i)
    DK_REQUIRE(!queries_in_tail(m->dimg[i], &m->dtxt[i], false),
               "the IP-Adapter reads the image queries raw from QKV: dk_tune_set(\"gemm_fuse_q\", 1) norms and rotates them in the projection's tail");
  DK_REQUIRE(!m->tapped() && !m->bc_on && m->S_r == 0 && m->cond_f == 0 && !m->slg() && !m->perturbed() && m->n_dual == 0,
             "the IP-Adapter cannot run with control taps, a block cache, a reference grid, a condition width, skip layers, perturbed attention or dual attention blocks");
  return 0;
}

// The fork of both features: rows [0, live) alone up to block `first`, there the fork rows become a copy of rows [0, fork_rows), and from there on
// block g runs on the rows [0, rows_of(g)) -- each group of launches is the driver's for its row count
template <class RowsOf>
static int mmdit_forward_fork(dk_mmdit* m, const void* tokens_in, const void* text, const bf16_t* mod_step, bf16_t* tokens_out, const LaunchCtx& L,
                              int first, RowsOf rows_of) {
  const int fork = m->fork_rows, live = m->B - fork, depth = m->cfg.depth_multimodal;
  DK_TRY(mmdit_embed(m, tokens_in, text, L, live));
  if (first > 0) DK_TRY(mmdit_blocks(m, mod_step, 0, first, L, live));
  const size_t row = (size_t)m->S * m->h() * 2;
  DK_CHECK_HIP(hipMemcpyAsync(m->X + (size_t)live * m->S * m->h(), m->X, (size_t)fork * row, hipMemcpyDeviceToDevice, L.st));
  for (int g = first; g < depth; ++g) DK_TRY(mmdit_blocks(m, mod_step, g, 1, L, rows_of(g)));
  return mmdit_final_layer(m, mod_step, tokens_out, L);
}
// dk_mmdit_forward with skip layers set: the fork in front of the first skipped block; the fork rows run every block behind it but the skipped ones
static int mmdit_forward_forked(dk_mmdit* m, const void* tokens_in, const void* text, const bf16_t* mod_step, bf16_t* tokens_out, const LaunchCtx& L) {
  const int B = m->B, live = B - m->fork_rows;
  DK_REQUIRE(2 * m->fork_rows <= B, "skip layers: 2 * fork_rows must not exceed the prepared batch (the fork rows copy rows [0, fork_rows))");
  DK_REQUIRE(m->S_r == 0 && m->cond_f == 0 && m->cfg.depth_unified == 0 && !m->fp8(),
             "skip layers cannot run with a reference grid, a condition width, single blocks or fp8_linears");
  return mmdit_forward_fork(m, tokens_in, text, mod_step, tokens_out, L, m->skip.front(), [&](int g) { return m->skipped(g) ? live : B; });
}
// ... with perturbed attention set: the fork in front of the first block of the set; every block behind it runs on all rows, and the blocks of the
// set give the fork rows the identity launch (double_block_bf16)
static int mmdit_forward_perturbed(dk_mmdit* m, const void* tokens_in, const void* text, const bf16_t* mod_step, bf16_t* tokens_out, const LaunchCtx& L) {
  const int B = m->B;
  DK_REQUIRE(2 * m->fork_rows <= B, "perturbed attention: 2 * fork_rows must not exceed the prepared batch (the fork rows copy rows [0, fork_rows))");
  DK_REQUIRE(m->S_r == 0 && m->cond_f == 0 && m->cfg.depth_unified == 0 && !m->fp8(),
             "perturbed attention cannot run with a reference grid, a condition width, single blocks or fp8_linears");
  DK_REQUIRE(m->D() == 64, "perturbed attention: the identity attention kernel is built for head_dim 64");
  return mmdit_forward_fork(m, tokens_in, text, mod_step, tokens_out, L, m->pag.front(), [&](int) { return B; });
}

extern "C" int dk_mmdit_forward(dk_mmdit* m, const void* tokens_in, const void* text, int32_t step_index, void* tokens_out,
                                void* stream) {
  DK_REQUIRE(m && m->prepared && m->mod_ready, "prepare + cache_modulation_params must precede forward");
  DK_REQUIRE(step_index >= 0 && step_index < m->n_t, "step index out of range");
  const LaunchCtx L = m->ctx(stream);
  const bf16_t* mod_step = m->MOD + (size_t)step_index * m->B * m->mod_rows() * m->h();
  DK_TRY(no_control_net(m, "dk_mmdit_forward"));
  DK_TRY(need_ip_adapter(m));
  m->bc_pending = -1;  // (a head without its tail is dropped: this call overwrites the stream it left; R / D_ref stay)
  if (m->slg()) return mmdit_forward_forked(m, tokens_in, text, mod_step, (bf16_t*)tokens_out, L);
  if (m->perturbed()) return mmdit_forward_perturbed(m, tokens_in, text, mod_step, (bf16_t*)tokens_out, L);
  DK_TRY(mmdit_embed(m, tokens_in, text, L));
  DK_TRY(mmdit_blocks(m, mod_step, 0, m->cfg.depth_multimodal + m->cfg.depth_unified, L));
  return mmdit_final_layer(m, mod_step, (bf16_t*)tokens_out, L);
}

// ---- first-block cache (include/dk_hip.h) -----------------------------------------------------------------------------------------
extern "C" int dk_mmdit_set_block_cache(dk_mmdit* m, int32_t on) {
  DK_REQUIRE(m != nullptr, "null handle");
  if (on) DK_REQUIRE(!m->control_net && !m->tapped(), "the block cache cannot be switched on on a control-net engine or while control taps are set");
  if (on) DK_REQUIRE(m->ip_n == 0, "the block cache cannot be switched on on an engine with an IP-Adapter (dk_mmdit_set_ip_adapter)");
  if (m->bc_on != (on != 0)) m->prepared = false;  // (another carve: dk_mmdit_prepare must follow)
  m->bc_on = on != 0;
  m->bc_reset();
  return 0;
}
extern "C" int dk_mmdit_reset_block_cache(dk_mmdit* m) {
  DK_REQUIRE(m != nullptr, "null handle");
  m->bc_reset();
  return 0;
}
// image rows of the stream <-> a dense [B * S_i, h] buffer
static int bc_save_img(const dk_mmdit* m, bf16_t* dst, hipStream_t st) {
  const size_t row = (size_t)m->S_i * m->h() * 2;
  DK_CHECK_HIP(hipMemcpy2DAsync(dst, row, m->X + (size_t)m->S_t * m->h(), (size_t)m->S * m->h() * 2, row, m->B, hipMemcpyDeviceToDevice, st));
  return 0;
}
extern "C" int dk_mmdit_forward_head(dk_mmdit* m, const void* tokens_in, const void* text, int32_t step_index, float* probe_out, void* stream) {
  DK_REQUIRE(m && m->prepared && m->mod_ready, "prepare + cache_modulation_params must precede forward_head");
  DK_TRY(no_ip_adapter(m, "dk_mmdit_forward_head"));  // (in front of the block cache's rule: an engine with an adapter can have no block cache)
  DK_REQUIRE(m->bc_on, "forward_head needs the block cache: dk_mmdit_set_block_cache(m, 1) before dk_mmdit_prepare");
  DK_REQUIRE(probe_out != nullptr, "null argument");
  DK_TRY(no_skip_layers(m, "dk_mmdit_forward_head"));
  DK_TRY(no_control_net(m, "dk_mmdit_forward_head"));
  DK_TRY(no_control_taps(m, "dk_mmdit_forward_head"));
  DK_REQUIRE(step_index >= 0 && step_index < m->n_t, "step index out of range");
  const LaunchCtx L = m->ctx(stream);
  const int h = m->h();
  const bf16_t* mod_step = m->MOD + (size_t)step_index * m->B * m->mod_rows() * h;
  m->bc_pending = -1;
  DK_TRY(mmdit_embed(m, tokens_in, text, L));
  bf16_t* dcur = m->BC_D[m->bc_cur];
  DK_TRY(bc_save_img(m, dcur, L.st));  // X0
  DK_TRY(mmdit_blocks(m, mod_step, 0, 1, L));
  DK_TRY(DK_EL(L.dtype, dk_launch_block_probe)(m->X + (size_t)m->S_t * h, h, m->S_i, m->S, dcur, m->bc_valid ? m->BC_D[1 - m->bc_cur] : nullptr,
                                               m->BC_ROWS, probe_out, m->B * m->S_i, h, m->S_i, L.st));
  m->bc_pending = step_index;
  return 0;
}
extern "C" int dk_mmdit_forward_tail(dk_mmdit* m, int32_t step_index, int32_t reuse, void* tokens_out, void* stream) {
  DK_REQUIRE(m && m->prepared && m->mod_ready, "prepare + cache_modulation_params must precede forward_tail");
  DK_TRY(no_ip_adapter(m, "dk_mmdit_forward_tail"));  // (in front of the block cache's rule, as in dk_mmdit_forward_head)
  DK_REQUIRE(m->bc_on && tokens_out != nullptr, "forward_tail needs the block cache and an output");
  DK_TRY(no_skip_layers(m, "dk_mmdit_forward_tail"));
  DK_TRY(no_control_net(m, "dk_mmdit_forward_tail"));
  DK_TRY(no_control_taps(m, "dk_mmdit_forward_tail"));
  DK_REQUIRE(m->bc_pending >= 0, "forward_tail needs a pending head: dk_mmdit_forward_head of this step must run first");
  DK_REQUIRE(m->bc_pending == step_index, "forward_tail must be of the same step as the pending head");
  if (reuse) DK_REQUIRE(m->bc_valid, "forward_tail(reuse = 1) needs a valid cache: a computed step since the last prepare / cache_modulation_params / reset");
  const LaunchCtx L = m->ctx(stream);
  const int h = m->h(), Mi = m->B * m->S_i;
  const bf16_t* mod_step = m->MOD + (size_t)step_index * m->B * m->mod_rows() * h;
  bf16_t* x_img = m->X + (size_t)m->S_t * h;
  m->bc_pending = -1;
  if (reuse) {
    DK_TRY(DK_EL(L.dtype, dk_launch_block_residual)(x_img, h, m->S_i, m->S, m->BC_R, Mi, h, true, L.st));
    return mmdit_final_layer(m, mod_step, (bf16_t*)tokens_out, L);
  }
  m->bc_valid = false;  // (R is being rewritten; valid again once every launch of this tail is queued)
  DK_TRY(bc_save_img(m, m->BC_R, L.st));  // X1
  DK_TRY(mmdit_blocks(m, mod_step, 1, m->cfg.depth_multimodal + m->cfg.depth_unified - 1, L));
  DK_TRY(mmdit_final_layer(m, mod_step, (bf16_t*)tokens_out, L));
  DK_TRY(DK_EL(L.dtype, dk_launch_block_residual)(x_img, h, m->S_i, m->S, m->BC_R, Mi, h, false, L.st));
  m->bc_cur = 1 - m->bc_cur;  // D_ref <- D_cur
  m->bc_valid = true;
  return 0;
}

// Teacher-forced block range (include/dk_hip.h): x_in -> m->X, blocks [first, first + count), m->X -> x_out
extern "C" int dk_mmdit_run_blocks(dk_mmdit* m, const void* x_in, void* x_out, int32_t step_index, int32_t first_block, int32_t n_blocks,
                                   void* stream) {
  DK_REQUIRE(m && m->prepared && m->mod_ready, "prepare + cache_modulation_params must precede run_blocks");
  DK_REQUIRE(x_in && x_out, "null argument");
  DK_TRY(no_skip_layers(m, "dk_mmdit_run_blocks"));
  DK_TRY(no_control_taps(m, "dk_mmdit_run_blocks"));
  DK_TRY(no_ip_adapter(m, "dk_mmdit_run_blocks"));
  DK_REQUIRE(step_index >= 0 && step_index < m->n_t, "step index out of range");
  const int total = m->cfg.depth_multimodal + m->cfg.depth_unified;
  DK_REQUIRE(first_block >= 0 && n_blocks >= 1 && first_block + n_blocks <= total, "block range outside the model");
  DK_TRY(need_reference(m));
  DK_TRY(need_condition(m));
  const LaunchCtx L = m->ctx(stream);
  const hipStream_t st = L.st;
  const size_t bytes = (size_t)m->B * m->S * m->h() * 2;
  const bf16_t* mod_step = m->MOD + (size_t)step_index * m->B * m->mod_rows() * m->h();
  DK_CHECK_HIP(hipMemcpyAsync(m->X, x_in, bytes, hipMemcpyDeviceToDevice, st));
  DK_TRY(mmdit_blocks(m, mod_step, first_block, n_blocks, L));
  DK_CHECK_HIP(hipMemcpyAsync(x_out, m->X, bytes, hipMemcpyDeviceToDevice, st));
  return 0;
}

extern "C" const void* dk_mmdit_debug_buffer(const dk_mmdit* m, int32_t which) {
  if (!m || !m->prepared) return nullptr;
  if (which >= 3 && which <= 5)  // R, D_ref, D_cur (5: the probe's output between a head and its tail; a compute tail makes that buffer D_ref)
    return !m->bc_on ? nullptr : which == 3 ? (const void*)m->BC_R : (const void*)m->BC_D[which == 4 ? 1 - m->bc_cur : m->bc_cur];
  if (which == 6) return (const void*)m->CONDE;  // x_embedder's condition share [B, S_i, h] (null with the width off)
  return which == 0 ? (const void*)m->X : which == 1 ? (const void*)m->MOD : which == 2 ? (const void*)m->GWS : nullptr;
}

