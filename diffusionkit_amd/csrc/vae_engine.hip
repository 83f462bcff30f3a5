// C-ABI layer (include/dk_hip.h), part 3: the VAE decoder (vae.py:336-401) and encoder engines (dk_vae_*) and the latent sampler.
// Host code only: no kernels are defined here.
#include <cmath>
#include <utility>

#include "dk_engine.h"

// dk_tune_set("conv_halo", v): the VAE's norm -> silu -> conv stages on the halo-staged kernel with the GroupNorm applied on load
// (conv_halo.hip): -1 (default) / 1 wherever the shape allows (measured: decode 15.1 -> 12.5 ms, against 13.0 ms when only the
// stages with fewer than 256 output channels use it -- the 256 / 512-channel convs are ~7 % slower than on the 256 x 256 implicit-GEMM
// kernel, but lose their GroupNorm-apply passes), 2 only below 256 output channels, 3 like 1 but the upsampling convs stay on the
// implicit-GEMM kernel, 0 never
int g_dk_conv_halo = -1;

struct dk_vae {
  dk_vae_config cfg;
  std::unordered_map<std::string, const void*> named;
  // workspace views
  bf16_t *bufA, *bufB, *T1, *Y, *SC, *LAT, *ZERO, *Qb, *Kb, *Vb, *Vt, *SCORES;
  float* gn;
  float *ss0, *ss1;  // GroupNorm (scale | shift) tables [B][2][C] of the fused norm -> silu -> conv stages
  void* GWS = nullptr;  // GEMM split workspace of this engine's launches (fp32 slabs + flags)
  // element type of every bound tensor, activation buffer, of `raw` (decode) and of the 16-bit moments (encode): dk_vae_set_dtype; sizes are the same
  int dtype = DK_DTYPE_BF16;
  bool dtype_set = false;
};

extern "C" int dk_vae_create(const dk_vae_config* cfg, dk_vae** out) {
  DK_REQUIRE(cfg && out, "null argument");
  DK_REQUIRE(cfg->n_blocks >= 1 && cfg->n_blocks <= 4, "1..4 resolution levels");
  for (int i = 0; i < cfg->n_blocks; ++i)
    DK_REQUIRE(cfg->block_out_channels[i] % 64 == 0, "VAE channel counts must be multiples of 64");
  DK_REQUIRE(cfg->in_channels >= 1 && cfg->in_channels <= 64 && cfg->out_channels >= 1 && cfg->out_channels <= 64,
             "input / output channels of the VAE halves: 1..64");
  dk_vae* v = new dk_vae();
  v->cfg = *cfg;
  *out = v;
  return 0;
}
extern "C" int dk_vae_set_dtype(dk_vae* v, int32_t dtype) {
  DK_REQUIRE(v != nullptr, "null handle");
  DK_REQUIRE(dtype == DK_DTYPE_BF16 || dtype == DK_DTYPE_F16, "VAE dtype: 0 bf16, 1 fp16");
  if (v->dtype_set || !v->named.empty())
    DK_REQUIRE(dtype == v->dtype, "dk_vae_set_dtype must precede the first dk_vae_bind; afterwards only the type already set is accepted");
  v->dtype = dtype;
  v->dtype_set = true;
  return 0;
}
extern "C" void dk_vae_destroy(dk_vae* v) { delete v; }
extern "C" int dk_vae_bind(dk_vae* v, const char* name, const void* dev_ptr) {
  DK_REQUIRE(v && name && dev_ptr, "null argument");
  v->named[name] = dev_ptr;
  return 0;
}

// The four numbers in which the workspaces of the two halves differ
struct VaeExtents {
  size_t maxel;   // largest activation, elements
  size_t in_px;   // pixels of the channel-padded input (LAT)
  size_t tok;     // tokens of one image in the mid block's attention
  size_t tiles;   // 16 x 16 output tiles of the largest stage of one image (statistics partials of the fused convs)
};
static VaeExtents decoder_extents(const dk_vae_config& cf, int B, int h, int w) {
  // largest activation: walk the decoder (vae.py:386-401) and take max(B * H * W * C)
  size_t H = h, W = w;
  int Cprev = cf.block_out_channels[cf.n_blocks - 1];
  size_t maxel = (size_t)B * H * W * Cprev;
  for (int j = cf.n_blocks - 1; j >= 0; --j) {
    const int Cout = cf.block_out_channels[j];
    const size_t e = (size_t)B * H * W * (size_t)(Cprev > Cout ? Cprev : Cout);
    if (e > maxel) maxel = e;
    if (j > 0) {
      H *= 2;
      W *= 2;
      if ((size_t)B * H * W * Cout > maxel) maxel = (size_t)B * H * W * Cout;
    }
    Cprev = Cout;
  }
  return {maxel, (size_t)B * h * w, (size_t)h * w, ((size_t)h << (cf.n_blocks - 1)) / 16 * (((size_t)w << (cf.n_blocks - 1)) / 16)};
}
static VaeExtents encoder_extents(const dk_vae_config& cf, int B, int H, int W) {
  size_t maxel = (size_t)B * H * W * 64;  // channel-padded input image
  size_t h = H, w = W;
  int Cprev = cf.block_out_channels[0];
  for (int i = 0; i < cf.n_blocks; ++i) {
    const int Cout = cf.block_out_channels[i];
    const size_t e = (size_t)B * h * w * (size_t)(Cprev > Cout ? Cprev : Cout);
    if (e > maxel) maxel = e;
    if (i < cf.n_blocks - 1) { h /= 2; w /= 2; }
    Cprev = Cout;
  }
  return {maxel, (size_t)B * H * W, ((size_t)H >> (cf.n_blocks - 1)) * ((size_t)W >> (cf.n_blocks - 1)), ((size_t)H / 16) * ((size_t)W / 16)};
}
// (the order and the sizes of the buffers are the layout dk_vae_workspace_bytes / dk_vae_encoder_workspace_bytes report)
static size_t vae_carve(dk_vae* v, Carver& c, int B, const VaeExtents& e) {
  const dk_vae_config& cf = v->cfg;
  const size_t act = e.maxel * 2;
  v->bufA = (bf16_t*)c.take(act);
  v->bufB = (bf16_t*)c.take(act);
  v->T1 = (bf16_t*)c.take(act);
  v->Y = (bf16_t*)c.take(act);
  v->SC = (bf16_t*)c.take(act);
  v->LAT = (bf16_t*)c.take(e.in_px * 64 * 2);
  v->ZERO = (bf16_t*)c.take(256);
  const int Cm = cf.block_out_channels[cf.n_blocks - 1];
  const size_t tok = e.tok;
  v->Qb = (bf16_t*)c.take((size_t)B * tok * Cm * 2);
  v->Kb = (bf16_t*)c.take((size_t)B * tok * Cm * 2);
  v->Vb = (bf16_t*)c.take((size_t)B * tok * Cm * 2);
  v->Vt = (bf16_t*)c.take((size_t)B * align_up(tok, 64) * Cm * 2);  // (the flash form transposes every image's V up front)
  // the materialised score matrix of the general path; a 512-channel mid block runs the flash kernel (attention512.hip) and needs none
  v->SCORES = (bf16_t*)c.take(Cm == 512 ? 0 : tok * align_up(tok, 64) * 2);
  {
    // statistics scratch: up to 1024 chunk partials per batch row from the stand-alone pass, or one per 16 x 16 output tile of the
    // largest stage from the fused convs, + mean / rstd
    const size_t npart = e.tiles > 1024 ? e.tiles : 1024;
    v->gn = (float*)c.take(((size_t)B * npart * 2 * cf.resnet_groups + (size_t)B * cf.resnet_groups * 2) * 4);
    int cmax = 0;
    for (int j = 0; j < cf.n_blocks; ++j) cmax = cf.block_out_channels[j] > cmax ? cf.block_out_channels[j] : cmax;
    v->ss0 = (float*)c.take((size_t)B * 2 * cmax * 4);
    v->ss1 = (float*)c.take((size_t)B * 2 * cmax * 4);
  }
  v->GWS = c.take(dk_gemm_split_workspace_bytes());
  return c.off;
}
extern "C" size_t dk_vae_workspace_bytes(const dk_vae* v, int32_t batch, int32_t latent_h, int32_t latent_w) {
  dk_vae tmp = *v;
  Carver c(nullptr, 0);
  return vae_carve(&tmp, c, batch, decoder_extents(tmp.cfg, batch, latent_h, latent_w)) + 256;
}

struct VaeRun : LaunchCtx {  // (st, dtype; kws: the 3x3 convs' split region; no attention region)
  dk_vae* v;
  int B;
  int rc = 0;
  const bf16_t* W(const std::string& name) {
    const bf16_t* p = nullptr;
    if (rc == 0) rc = need(v->named, name, &p);
    return p;
  }
  bool has(const std::string& name) const { return v->named.count(name) != 0; }
  int gn(const bf16_t* x, bf16_t* y, long HW, int C, const std::string& name, int silu) {
    const bf16_t *g = W(name + ".weight"), *b = W(name + ".bias");
    if (rc) return rc;
    return groupnorm_launch(dtype, x, y, B, HW, C, v->cfg.resnet_groups, g, b, v->cfg.group_norm_eps, silu, v->gn, st);
  }
  int conv(const bf16_t* x, bf16_t* y, int H, int Wd, int C, int O, const std::string& name, int ups, const bf16_t* res, int ldy) {
    dk_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.x = x; d.w = W(name + ".weight"); d.bias = W(name + ".bias"); d.y = y; d.res = res; d.zeros = v->ZERO;
    if (rc) return rc;
    d.B = B; d.H = H; d.W = Wd; d.C = C; d.O = O; d.ldy = ldy; d.ldr = O; d.upsample = ups;
    d.epilogue = res ? DK_EPI_RES : DK_EPI_BIAS;
    return conv3x3_launch(dtype, &d, kws, st);
  }
  // ---- fused norm -> silu -> conv stages (conv_halo.hip) ----
  int n_part = 0;  // > 0: v->gn holds the output-statistics partials [B][n_part][G][2] of the tensor the last fused conv wrote
  bool halo_stage(int H, int Wd, int Cin, int Cout) const {
    if (g_dk_conv_halo == 0 || H % 16 != 0 || Wd % 16 != 0 || Cin % 64 != 0 || Cout % 128 != 0) return false;
    if ((size_t)H * Wd * (Cin > Cout ? Cin : Cout) * 2 >= (1ull << 31)) return false;
    // the fused stages always ask their conv for the output statistics of the next GroupNorm (dk_conv_halo_eligible: a channel
    // group must divide the 128-channel workgroup tile and span at most 64 channels) -- other group plans take gn() + conv()
    const int G = v->cfg.resnet_groups;
    if (G <= 0 || Cout % G != 0 || 128 % (Cout / G) != 0 || Cout / G > 64) return false;
    return g_dk_conv_halo != 2 || Cout < 256;
  }
  // the (scale | shift) table of GroupNorm `name` over tensor x: from the partials the producing conv left, or a statistics pass
  int gn_table(const bf16_t* x, long HW, int C, const std::string& name, float* ss) {
    const bf16_t *g = W(name + ".weight"), *b = W(name + ".bias");
    if (rc) return rc;
    const int np = n_part;
    n_part = 0;
    return groupnorm_table_launch(dtype, np > 0 ? nullptr : x, B, HW, C, v->cfg.resnet_groups, g, b, v->cfg.group_norm_eps, v->gn, np, ss, st);
  }
  // a conv_halo.hip launch of this run: the fields all of them set (ldw: row pitch of the weight, ldy: of y -- 0 for the image tail);
  // operands, norm table, statistics and outputs stay at the call site
  ConvHaloParams halo_conv(int H, int Wd, int C, int O, int ldw, int ldy) const {
    ConvHaloParams c;
    memset(&c, 0, sizeof(c));
    c.dtype = dtype;
    c.B = B; c.H = H; c.W = Wd; c.C = C; c.O = O; c.ldw = ldw; c.ldy = ldy;
    return c;
  }
  // ResnetBlock2D (vae.py:60-101) in two launches + two statistics finalisations: x stays raw, both GroupNorm + SiLU are applied
  // on the way into the convs' LDS halo tiles, conv1 / conv2 leave the statistics of their outputs behind (stats_next: somebody
  // normalises `out` next), the 1x1 shortcut rides in conv2's reduction
  int resnet_fused(const bf16_t* x, bf16_t* out, int H, int Wd, int Cin, int Cout, const std::string& p, bool stats_next) {
    const long HW = (long)H * Wd;
    const int tiles = (H / 16) * (Wd / 16), G = v->cfg.resnet_groups;
    DK_TRY(gn_table(x, HW, Cin, p + ".norm1", v->ss0));
    ConvHaloParams c = halo_conv(H, Wd, Cin, Cout, 9 * Cin, Cout);
    c.x = x; c.w = W(p + ".conv1.weight"); c.bias = W(p + ".conv1.bias"); c.y = v->Y; c.gn_ss = v->ss0; c.gn_silu = 1;
    c.stats_out = v->gn; c.G_out = G;
    if (rc) return rc;
    DK_TRY(dk_launch_conv_halo(c, st));
    n_part = tiles;
    DK_TRY(gn_table(v->Y, HW, Cout, p + ".norm2", v->ss1));
    const bool shortcut = has(p + ".conv_shortcut.weight");
    c = halo_conv(H, Wd, Cout, Cout, shortcut ? 9 * Cout + Cin : 9 * Cout, Cout);
    c.x = v->Y; c.bias = W(p + ".conv2.bias"); c.y = out; c.gn_ss = v->ss1; c.gn_silu = 1; c.ldr = Cout;
    if (shortcut) {
      c.w = W(p + ".conv2_sc.weight");  // [conv2 | conv_shortcut] along the reduction (weights.pack_vae)
      c.x2 = x; c.C2 = Cin; c.bias2 = W(p + ".conv_shortcut.bias");
    } else {
      DK_REQUIRE(Cin == Cout, "resnet without shortcut must keep the channel count");
      c.w = W(p + ".conv2.weight"); c.res = x;
    }
    if (stats_next) { c.stats_out = v->gn; c.G_out = G; }
    if (rc) return rc;
    DK_TRY(dk_launch_conv_halo(c, st));
    n_part = stats_next ? tiles : 0;
    return 0;
  }
  // ResnetBlock2D (vae.py:60-101): x [B,H,W,Cin] -> out [B,H,W,Cout]
  int resnet(const bf16_t* x, bf16_t* out, int H, int Wd, int Cin, int Cout, const std::string& p, bool stats_next = false) {
    if (halo_stage(H, Wd, Cin, Cout) && (Cin == Cout || has(p + ".conv2_sc.weight"))) return resnet_fused(x, out, H, Wd, Cin, Cout, p, stats_next);
    n_part = 0;
    const long HW = (long)H * Wd;
    DK_TRY(gn(x, v->T1, HW, Cin, p + ".norm1", 1));
    DK_TRY(conv(v->T1, v->Y, H, Wd, Cin, Cout, p + ".conv1", 0, nullptr, Cout));
    DK_TRY(gn(v->Y, v->T1, HW, Cout, p + ".norm2", 1));
    const bf16_t* res = x;
    if (has(p + ".conv_shortcut.weight")) {
      const bf16_t *sw = W(p + ".conv_shortcut.weight"), *sb = W(p + ".conv_shortcut.bias");
      if (rc) return rc;
      DK_TRY(dk_launch_gemm(Linear(dtype, dense(x, Cin), sw, sb, dense(v->SC, Cout), (int)(B * HW), Cout, Cin, DK_EPI_BIAS), st));
      res = v->SC;
    } else {
      DK_REQUIRE(Cin == Cout, "resnet without shortcut must keep the channel count");
    }
    return conv(v->T1, out, H, Wd, Cout, Cout, p + ".conv2", 0, res, Cout);
  }
  // single-head attention (vae.py:28-57).  None of its Linears carries the split workspace (nor does the resnets' 1x1 shortcut): of this
  // engine's launches only the 3x3 convs (conv) do
  int attention(const bf16_t* x, bf16_t* out, int H, int Wd, int C, const std::string& p) {
    const long HW = (long)H * Wd;
    const int T = (int)HW;
    DK_REQUIRE(T % 4 == 0, "VAE attention: even latent sides");
    const int Tp = (int)align_up((size_t)T, 64);  // K of the P.V product: zero-padded probability columns / V^T rows
    DK_TRY(gn(x, v->T1, HW, C, p + ".group_norm", 0));
    const bf16_t *qw = W(p + ".query_proj.weight"), *qb = W(p + ".query_proj.bias");
    const bf16_t *kw = W(p + ".key_proj.weight"), *kb = W(p + ".key_proj.bias");
    const bf16_t *vw = W(p + ".value_proj.weight"), *vb = W(p + ".value_proj.bias");
    const bf16_t *ow = W(p + ".out_proj.weight"), *ob = W(p + ".out_proj.bias");
    if (rc) return rc;
    DK_TRY(dk_launch_gemm(Linear(dtype, dense(v->T1, C), qw, qb, dense(v->Qb, C), B * T, C, C, DK_EPI_BIAS), st));
    DK_TRY(dk_launch_gemm(Linear(dtype, dense(v->T1, C), kw, kb, dense(v->Kb, C), B * T, C, C, DK_EPI_BIAS), st));
    DK_TRY(dk_launch_gemm(Linear(dtype, dense(v->T1, C), vw, vb, dense(v->Vb, C), B * T, C, C, DK_EPI_BIAS), st));
    const float scale = 1.0f / sqrtf((float)C);
    // flash form (attention512.hip): no [T, T] score matrix
    if (C == 512) DK_TRY(attention_d512(dtype, v->Qb, v->Kb, v->Vb, v->Y, B, T, C, C, scale, v->Vt, st));
    else
      for (int b = 0; b < B; ++b) {
        Linear g(dtype, dense(v->Qb + (size_t)b * T * C, C), v->Kb + (size_t)b * T * C, nullptr, dense(v->SCORES, Tp), T, T, C, DK_EPI_BIAS);
        g.alpha = scale;  // scores = scale * q @ k^T
        DK_TRY(dk_launch_gemm(g, st));
        DK_TRY(DK_EL(dtype, dk_launch_softmax_rows)(v->SCORES, T, T, Tp, st));  // columns [T, Tp) come out as zeros
        DK_TRY(DK_EL(dtype, dk_launch_transpose)(v->Vb + (size_t)b * T * C, v->Vt, T, C, st, Tp));
        // attn @ V: A = probs [T, Tp], W = V^T [C, Tp]; result into Y rows of this batch
        DK_TRY(dk_launch_gemm(Linear(dtype, dense(v->SCORES, Tp), v->Vt, nullptr, dense(v->Y + (size_t)b * T * C, C), T, C, Tp, DK_EPI_BIAS), st));
      }
    // out_proj + residual
    return dk_launch_gemm(Linear(dtype, dense(v->Y, C), ow, ob, dense(out, C), B * T, C, C, DK_EPI_RES).gate_res(nullptr, 0, 0, dense(x, C)), st);
  }
};

extern "C" int dk_vae_decode(dk_vae* v, const float* latent, int32_t batch, int32_t latent_h, int32_t latent_w, float* image_f32,
                             uint8_t* image_u8, void* raw_bf16, void* workspace, size_t workspace_bytes, void* stream) {
  DK_REQUIRE(v && latent && workspace, "null argument");
  DK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  Carver c(workspace, workspace_bytes);
  const size_t need_bytes = vae_carve(v, c, batch, decoder_extents(v->cfg, batch, latent_h, latent_w));
  DK_REQUIRE(need_bytes <= workspace_bytes, "workspace too small");
  const dk_vae_config& cf = v->cfg;
  VaeRun R{{S_(stream), v->dtype, v->GWS}, v, batch};
  hipStream_t st = R.st;
  // the flag region of the GEMM split workspace must be zero before the first launch (the kernels leave it zero)
  DK_CHECK_HIP(hipMemsetAsync((char*)v->GWS + DK_KSPLIT_FLAGS_OFF, 0, DK_KSPLIT_FLAG_BYTES, st));
  DK_CHECK_HIP(hipMemsetAsync(v->ZERO, 0, 256, st));
  int H = latent_h, W = latent_w;
  const int Cm = cf.block_out_channels[cf.n_blocks - 1];
  DK_TRY(DK_EL(v->dtype, dk_launch_pad_channels)(latent, v->LAT, (long)batch * H * W, cf.in_channels, 64, st));
  bf16_t *cur = v->bufA, *nxt = v->bufB;
  DK_TRY(R.conv(v->LAT, cur, H, W, 64, Cm, "conv_in", 0, nullptr, Cm));
  DK_TRY(R.resnet(cur, nxt, H, W, Cm, Cm, "mid_blocks.0")); std::swap(cur, nxt);
  DK_TRY(R.attention(cur, nxt, H, W, Cm, "mid_blocks.1")); std::swap(cur, nxt);
  DK_TRY(R.resnet(cur, nxt, H, W, Cm, Cm, "mid_blocks.2", true)); std::swap(cur, nxt);  // (the first up-block's norm1 reads its partials)
  int C = Cm;
  // up_blocks list index n-1 runs first (vae.py:379,393); index 0 has no upsample conv
  for (int j = cf.n_blocks - 1; j >= 0; --j) {
    const int Cout = cf.block_out_channels[j];
    for (int r = 0; r < cf.layers_per_block; ++r) {
      const std::string p = "up_blocks." + std::to_string(j) + ".resnets." + std::to_string(r);
      // (somebody normalises the output next: the following resnet, or conv_norm_out behind the last block)
      const bool gn_next = r + 1 < cf.layers_per_block || j == 0;
      DK_TRY(R.resnet(cur, nxt, H, W, r == 0 ? C : Cout, Cout, p, gn_next)); std::swap(cur, nxt);
    }
    C = Cout;
    if (j > 0) {
      H *= 2; W *= 2;
      R.n_part = 0;
      const std::string up = "up_blocks." + std::to_string(j) + ".upsample";
      if (g_dk_conv_halo != 3 && R.halo_stage(H, W, C, C)) {  // (3: the upsampling convs stay on the implicit-GEMM kernel)
        // the upsampling conv (vae.py:20-25,146) on the halo kernel too: nearest-x2 folded into the halo addressing, no norm in
        // front of it, and the statistics of its output for the next block's first GroupNorm
        ConvHaloParams c = R.halo_conv(H, W, C, C, 9 * C, C);
        c.x = cur; c.w = R.W(up + ".weight"); c.bias = R.W(up + ".bias"); c.y = nxt; c.stats_out = v->gn; c.G_out = cf.resnet_groups;
        c.ups = 1;
        if (R.rc) return R.rc;
        DK_TRY(dk_launch_conv_halo(c, st));
        R.n_part = (H / 16) * (W / 16);
      } else {
        DK_TRY(R.conv(cur, nxt, H, W, C, C, up, 1, nullptr, C));
      }
      std::swap(cur, nxt);
    }
  }
  if (g_dk_conv_halo != 0 && H % 16 == 0 && W % 16 == 0 && C % 64 == 0 && cf.out_channels <= 4 && (size_t)H * W * C * 2 < (1ull << 31)) {
    // conv_norm_out -> silu -> conv_out -> clip / uint8 (vae.py:381,384,397-399; __init__.py:581-584,525-526) in one launch
    DK_TRY(R.gn_table(cur, (long)H * W, C, "conv_norm_out", v->ss0));
    ConvHaloParams c = R.halo_conv(H, W, C, cf.out_channels, 9 * C, 0);
    c.x = cur; c.w = R.W("conv_out.weight"); c.bias = R.W("conv_out.bias"); c.gn_ss = v->ss0; c.gn_silu = 1;
    c.img = image_f32; c.u8 = image_u8; c.raw = raw_bf16 ? (bf16_t*)raw_bf16 : v->Y; c.out_channels = cf.out_channels;
    if (R.rc) return R.rc;
    DK_TRY(dk_launch_conv_halo(c, st));
    return R.rc;
  }
  DK_TRY(R.gn(cur, v->T1, (long)H * W, C, "conv_norm_out", 1));
  bf16_t* raw = raw_bf16 ? (bf16_t*)raw_bf16 : v->Y;
  // (the conv writes out_channels of the 4 columns per pixel; the fused tail above stores zeros in the rest, so does this one)
  if (raw_bf16 && cf.out_channels < 4) DK_CHECK_HIP(hipMemsetAsync(raw, 0, (size_t)batch * H * W * 4 * sizeof(bf16_t), st));
  DK_TRY(R.conv(v->T1, raw, H, W, C, cf.out_channels, "conv_out", 0, nullptr, 4));
  DK_TRY(DK_EL(v->dtype, dk_launch_image_post)(raw, 4, image_f32, image_u8, (long)batch * H * W, st));
  return R.rc;
}

// ---------------------------------------------------------------------------------------------
// VAE encoder engine (vae.py:404-467; img2img entry mlx/__init__.py:586-594).  Same handle type as the
// decoder: a dk_vae created with the encoder's config (in 3, out 32, layers_per_block 2) and bound to
// the encoder's module names (conv_in, down_blocks.{i}.resnets.{r}, down_blocks.{i}.downsample,
// mid_blocks.{0,1,2}, conv_norm_out, conv_out).
// ---------------------------------------------------------------------------------------------
extern "C" size_t dk_vae_encoder_workspace_bytes(const dk_vae* v, int32_t batch, int32_t image_h, int32_t image_w) {
  dk_vae tmp = *v;
  Carver c(nullptr, 0);
  return vae_carve(&tmp, c, batch, encoder_extents(tmp.cfg, batch, image_h, image_w)) + 256;
}

extern "C" int dk_vae_encode(dk_vae* v, const float* image, int32_t batch, int32_t image_h, int32_t image_w, void* moments_bf16,
                             int32_t ldm, float* moments_f32, void* workspace, size_t workspace_bytes, void* stream) {
  DK_REQUIRE(v && image && workspace && (moments_bf16 || moments_f32), "null argument");
  DK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  const dk_vae_config& cf = v->cfg;
  const int down = 1 << (cf.n_blocks - 1);
  DK_REQUIRE(image_h % down == 0 && image_w % down == 0, "image size must be a multiple of the VAE down-scaling factor");
  const int ldo = (cf.out_channels + 3) / 4 * 4;
  DK_REQUIRE(moments_bf16 == nullptr || ldm >= ldo, "moments leading dimension too small (multiple of 4 >= out_channels)");
  Carver c(workspace, workspace_bytes);
  const size_t need_bytes = vae_carve(v, c, batch, encoder_extents(v->cfg, batch, image_h, image_w));
  DK_REQUIRE(need_bytes <= workspace_bytes, "workspace too small");
  VaeRun R{{S_(stream), v->dtype, v->GWS}, v, batch};
  hipStream_t st = R.st;
  DK_CHECK_HIP(hipMemsetAsync((char*)v->GWS + DK_KSPLIT_FLAGS_OFF, 0, DK_KSPLIT_FLAG_BYTES, st));
  DK_CHECK_HIP(hipMemsetAsync(v->ZERO, 0, 256, st));
  int H = image_h, W = image_w;
  DK_TRY(DK_EL(v->dtype, dk_launch_pad_channels)(image, v->LAT, (long)batch * H * W, cf.in_channels, 64, st));
  bf16_t *cur = v->bufA, *nxt = v->bufB;
  int C = cf.block_out_channels[0];
  DK_TRY(R.conv(v->LAT, cur, H, W, 64, C, "conv_in", 0, nullptr, C));
  for (int i = 0; i < cf.n_blocks; ++i) {
    const int Cout = cf.block_out_channels[i];
    for (int r = 0; r < cf.layers_per_block; ++r) {
      const std::string p = "down_blocks." + std::to_string(i) + ".resnets." + std::to_string(r);
      DK_TRY(R.resnet(cur, nxt, H, W, r == 0 ? C : Cout, Cout, p)); std::swap(cur, nxt);
    }
    C = Cout;
    if (i < cf.n_blocks - 1) {  // pad (0,1),(0,1) + conv k3 s2 p0 (vae.py:141-143)
      H /= 2; W /= 2;
      DK_TRY(R.conv(cur, nxt, H, W, C, C, "down_blocks." + std::to_string(i) + ".downsample", 2, nullptr, C)); std::swap(cur, nxt);
    }
  }
  DK_TRY(R.resnet(cur, nxt, H, W, C, C, "mid_blocks.0")); std::swap(cur, nxt);
  DK_TRY(R.attention(cur, nxt, H, W, C, "mid_blocks.1")); std::swap(cur, nxt);
  DK_TRY(R.resnet(cur, nxt, H, W, C, C, "mid_blocks.2")); std::swap(cur, nxt);
  DK_TRY(R.gn(cur, v->T1, (long)H * W, C, "conv_norm_out", 1));
  bf16_t* mom = moments_bf16 ? (bf16_t*)moments_bf16 : v->Y;
  const int ld = moments_bf16 ? ldm : ldo;
  DK_TRY(R.conv(v->T1, mom, H, W, C, cf.out_channels, "conv_out", 0, nullptr, ld));
  if (moments_f32) DK_TRY(DK_EL(v->dtype, dk_launch_bf16_rows_to_f32)(mom, ld, moments_f32, (long)batch * H * W, cf.out_channels, st));
  return R.rc;
}

static int latent_sample(int dtype, const void* moments, int ldm, const float* noise, float* latent, long n_pixels, int latent_channels, void* stream) {
  DK_REQUIRE(moments && noise && latent && n_pixels > 0 && latent_channels > 0 && ldm >= 2 * latent_channels, "bad argument");
  return DK_EL(dtype, dk_launch_latent_sample)((const bf16_t*)moments, ldm, noise, latent, n_pixels, latent_channels, S_(stream));
}
extern "C" int dk_latent_sample_f32(const void* moments_bf16, int32_t ldm, const float* noise, float* latent, int64_t n_pixels,
                                    int32_t latent_channels, void* stream) {
  return latent_sample(DK_DTYPE_BF16, moments_bf16, ldm, noise, latent, (long)n_pixels, latent_channels, stream);
}
extern "C" int dk_latent_sample_f16(const void* moments_f16, int32_t ldm, const float* noise, float* latent, int64_t n_pixels,
                                    int32_t latent_channels, void* stream) {
  return latent_sample(DK_DTYPE_F16, moments_f16, ldm, noise, latent, (long)n_pixels, latent_channels, stream);
}
