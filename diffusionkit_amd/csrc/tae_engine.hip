// C-ABI layer (include/dk_hip.h), part 4: the tiny latent decoder (dk_tae_*) and its two stand-alone operators.
// Host code only: the kernels are in tae.hip.
#include "dk_engine.h"
#include "dk_tae.h"

// dk_tune_set("tae_block", v): the decoder's residual Blocks as the three-launch chain of single convs (-1 default / 0) or as one fused launch
// each (1).  The same bits either way.  Measured (profiles/tiny_decoder.md): the chain is the faster form -- 0.446 against 0.628 ms per call at 1024 x 1024,
// level at 128 x 128, and the whole decode is 1.05 - 1.35 x slower with fused Blocks -- so the engine takes it for every stage; the fused kernel stays reachable here
// and as ops.tae_block.  The chain needs the workspace's third buffer, which is always carved.
int g_dk_tae_block = -1;

struct dk_tae {
  std::unordered_map<std::string, const void*> named;
};

extern "C" int dk_tae_create(dk_tae** out) {
  DK_REQUIRE(out, "null argument");
  *out = new dk_tae();
  return 0;
}
extern "C" void dk_tae_destroy(dk_tae* t) { delete t; }
extern "C" int dk_tae_bind(dk_tae* t, const char* name, const void* dev_ptr) {
  DK_REQUIRE(t && name && dev_ptr, "null argument");
  t->named[name] = dev_ptr;
  return 0;
}

// two ping-pong activations at the largest stage [B, 8h, 8w, 64] + the chain form's intermediate
static size_t tae_act_bytes(int B, int h, int w) { return align_up((size_t)B * (8 * (size_t)h) * (8 * (size_t)w) * 64 * 2, 256); }
extern "C" size_t dk_tae_workspace_bytes(int32_t batch, int32_t latent_h, int32_t latent_w) {
  if (batch < 1 || latent_h < 1 || latent_w < 1) return 0;
  return 3 * tae_act_bytes(batch, latent_h, latent_w);
}

struct TaeRun {
  dk_tae* t;
  hipStream_t st;
  int B;
  bf16_t *cur, *nxt, *tmp;
  int rc = 0;
  const bf16_t* Wt(const std::string& name) {
    const bf16_t* p = nullptr;
    if (rc == 0) rc = need(t->named, name, &p);
    return p;
  }
  void swap() { bf16_t* s = cur; cur = nxt; nxt = s; }
  int block(int i, int H, int W) {
    const std::string p = std::to_string(i) + ".conv.";
    TaeBlockParams b;
    b.x = cur; b.y = nxt; b.B = B; b.H = H; b.W = W;
    for (int j = 0; j < 3; ++j) {
      b.w[j] = Wt(p + std::to_string(2 * j) + ".weight");
      b.b[j] = Wt(p + std::to_string(2 * j) + ".bias");
    }
    if (rc) return rc;
    if (g_dk_tae_block == 1) {
      DK_TRY(dk_launch_tae_block(b, st));
    } else {
      TaeConvParams c;
      memset(&c, 0, sizeof(c));
      c.B = B; c.H = H; c.W = W; c.relu = 1;
      c.x = cur; c.w = b.w[0]; c.bias = b.b[0]; c.y = nxt;
      DK_TRY(dk_launch_tae_conv(DK_TAE_MID, c, st));
      c.x = nxt; c.w = b.w[1]; c.bias = b.b[1]; c.y = tmp;
      DK_TRY(dk_launch_tae_conv(DK_TAE_MID, c, st));
      c.x = tmp; c.w = b.w[2]; c.bias = b.b[2]; c.y = nxt; c.skip = cur;
      DK_TRY(dk_launch_tae_conv(DK_TAE_MID, c, st));
    }
    swap();
    return 0;
  }
};

extern "C" int dk_tae_decode(dk_tae* t, const float* latent, int32_t batch, int32_t latent_h, int32_t latent_w, float scale, float shift,
                             float* image_f32, uint8_t* image_u8, void* workspace, size_t workspace_bytes, void* stream) {
  DK_REQUIRE(t && latent && workspace && (image_f32 || image_u8), "null argument");
  DK_REQUIRE(batch >= 1 && latent_h >= 1 && latent_w >= 1, "tae: batch, latent height and width must be positive");
  DK_REQUIRE(latent_h <= (1 << 24) && latent_w <= (1 << 24), "tae: latent side beyond 2^24");
  DK_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  DK_REQUIRE(dk_tae_workspace_bytes(batch, latent_h, latent_w) <= workspace_bytes, "workspace too small");
  const size_t act = tae_act_bytes(batch, latent_h, latent_w);
  TaeRun R{t, S_(stream), batch, (bf16_t*)workspace, (bf16_t*)((char*)workspace + act), (bf16_t*)((char*)workspace + 2 * act)};
  int H = latent_h, W = latent_w;
  TaeConvParams c;
  memset(&c, 0, sizeof(c));
  c.B = batch; c.H = H; c.W = W; c.xf = latent; c.scale = scale; c.shift = shift; c.relu = 1;
  c.w = R.Wt("1.weight"); c.bias = R.Wt("1.bias"); c.y = R.cur;
  if (R.rc) return R.rc;
  DK_TRY(dk_launch_tae_conv(DK_TAE_FIRST, c, R.st));
  int layer = 3;
  for (int stage = 0; stage < 3; ++stage) {
    for (int j = 0; j < 3; ++j) DK_TRY(R.block(layer++, H, W));
    ++layer;  // nearest x 2: a view of the next conv's tile load
    H *= 2; W *= 2;
    memset(&c, 0, sizeof(c));
    c.B = batch; c.H = H; c.W = W; c.ups = 1; c.x = R.cur; c.y = R.nxt;
    c.w = R.Wt(std::to_string(layer++) + ".weight");
    if (R.rc) return R.rc;
    DK_TRY(dk_launch_tae_conv(DK_TAE_MID, c, R.st));
    R.swap();
  }
  DK_TRY(R.block(layer++, H, W));  // 18
  memset(&c, 0, sizeof(c));
  c.B = batch; c.H = H; c.W = W; c.x = R.cur; c.img = image_f32; c.u8 = image_u8;
  c.w = R.Wt("19.weight"); c.bias = R.Wt("19.bias");
  if (R.rc) return R.rc;
  return dk_launch_tae_conv(DK_TAE_LAST, c, R.st);
}

extern "C" int dk_tae_block_bf16(const void* x, const void* const* weights, const void* const* biases, void* y, int32_t B, int32_t H, int32_t W,
                                 void* stream) {
  DK_REQUIRE(x && weights && biases && y, "null argument");
  TaeBlockParams p;
  p.x = (const bf16_t*)x; p.y = (bf16_t*)y; p.B = B; p.H = H; p.W = W;
  for (int j = 0; j < 3; ++j) { p.w[j] = (const bf16_t*)weights[j]; p.b[j] = (const bf16_t*)biases[j]; }
  return dk_launch_tae_block(p, S_(stream));
}

extern "C" int dk_tae_conv_bf16(const dk_tae_conv_desc* d, void* stream) {
  DK_REQUIRE(d != nullptr, "null argument");
  TaeConvParams c;
  memset(&c, 0, sizeof(c));
  if (d->kind == DK_TAE_FIRST) c.xf = (const float*)d->x;
  else c.x = (const bf16_t*)d->x;
  c.w = (const bf16_t*)d->w; c.bias = (const bf16_t*)d->bias; c.skip = (const bf16_t*)d->skip; c.y = (bf16_t*)d->y;
  c.img = d->image_f32; c.u8 = d->image_u8;
  c.B = d->B; c.H = d->H; c.W = d->W; c.ups = d->upsample; c.relu = d->relu; c.scale = d->scale; c.shift = d->shift;
  return dk_launch_tae_conv(d->kind, c, S_(stream));
}
