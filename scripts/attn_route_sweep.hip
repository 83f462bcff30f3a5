// dk_attention_route over the shapes of tests/test_dispatch_plan.py plus edge inputs, one line per call.  Host only: built with the host
// sanitizers and run on the CPU by scripts/attn_route_sweep.py, which also compares the lines with dk_attention_plan.
#include <cstdio>

#include "../diffusionkit_amd/csrc/dk_kernels.h"

struct Shape {
  int B, H, S, D, dtype, bias, o8, o8_split, qn;
};

static void one(const Shape& s, int n_cu, size_t ws) {
  AttnParams p;
  const int h = s.H * s.D;
  p.Q = (const bf16_t*)0x10000000; p.K = p.Q + h; p.V = p.K + h; p.O = (bf16_t*)0x20000000;
  p.B = s.B; p.H = s.H; p.S = s.S; p.D = s.D; p.ld = 3 * h; p.ldo = h; p.scale = 1.0f; p.dtype = s.dtype;
  if (s.bias) { p.bias = (const bf16_t*)0x30000000; p.ldb = (s.S + 63) / 64 * 64; p.bias_head_stride = (long)p.ldb * s.S; }
  if (s.qn) p.qn_a = p.qn_b = (const bf16_t*)0x40000000;
  if (s.o8) { p.O8 = (unsigned char*)0x50000000; p.O8_scales = (unsigned char*)0x60000000; p.o8_ld = h; p.o8_nblk = (s.B * s.S + 127) / 128 + 1; }
  p.o8_split = s.o8_split; p.o8_txt_row0 = s.B * (s.S - s.o8_split);
  printf("attn=%d attn_split=%d n_cu=%d ws=%zu dtype=%d B=%d H=%d S=%d D=%d bias=%d o8=%d o8_split=%d qn=%d -> ", g_dk_attn_mode, g_dk_attn5_split, n_cu, ws,
         s.dtype, s.B, s.H, s.S, s.D, s.bias, s.o8, s.o8_split, s.qn);
  AttnRoute r;
  if (dk_attention_route(p, ws, n_cu, r) != 0) { printf("refused: %s\n", dk_last_error()); return; }
  printf("kernel=%d qfuse=%d blocks=%d whole=%d split=%d jobs=%d quantize=%d launches=%d\n", r.kernel, (int)r.qfuse, r.blocks, r.whole, r.split, r.jobs,
         r.quantize, r.launches);
}

int main() {
  const Shape shapes[] = {
      // FLUX (H = 24, D = 128): 1024 x 1024 with 1 / 2 / 4 images, FLUX-dev, 768 x 768, 512 x 512, a ragged sequence, the MX-fp8 copy in both row orders
      {1, 24, 4352, 128}, {2, 24, 4352, 128}, {4, 24, 4352, 128}, {1, 24, 4608, 128}, {1, 24, 2560, 128}, {1, 24, 1280, 128}, {2, 24, 1280, 128},
      {1, 24, 4225, 128}, {1, 24, 4352, 128, 0, 0, 1, 256}, {1, 24, 4352, 128, 0, 0, 1, 0}, {1, 24, 1280, 128, 0, 0, 1, 256}, {1, 24, 4352, 128, 0, 0, 0, 0, 1},
      // head_dim 64 (SD3-medium, SD3.5-large) in both element types, a score bias, what the fp16 route refuses, bad arguments
      {2, 24, 1613, 64}, {2, 38, 4429, 64}, {2, 24, 1613, 64, 1}, {2, 38, 4429, 64, 1, 0, 0, 0, 1}, {1, 12, 77, 64, 0, 1}, {1, 24, 4352, 128, 0, 1},
      {1, 24, 4352, 128, 1}, {1, 24, 1613, 64, 1, 1}, {1, 24, 1280, 96}, {0, 24, 1280, 128}, {1, 24, 1280, 128, 0, 0, 1, 1280},
      // the edges of the one-wave-per-SIMD kernel's shape rule, and last rounds of 0, 1 and 255 blocks on 256 CUs (S = 768: 3 blocks per head)
      {1, 24, 1, 128}, {1, 24, 255, 128}, {1, 24, 256, 128}, {1, 24, 767, 128}, {1, 24, 768, 128}, {1, 256, 768, 128}, {1, 171, 768, 128}, {1, 85, 768, 128},
      {1, 171, 1536, 128}, {1, 85, 3072, 128}};
  const int knobs[][2] = {{-1, -1}, {10, -1}, {10, 4}, {10, 0}, {9, -1}, {4, -1}, {7, -1}};
  const int cus[] = {1, 16, 256, 304};
  for (const auto& k : knobs)
    for (const int n_cu : cus)
      for (const Shape& s : shapes) {
        g_dk_attn_mode = k[0]; g_dk_attn5_split = k[1];
        one(s, n_cu, 0);
        one(s, n_cu, (size_t)1020 * DK_ATTN5_JOB_BYTES);
        AttnParams probe;  // the region the launch wants: one job short, and exact
        AttnRoute r;
        probe.Q = probe.K = probe.V = nullptr; probe.B = s.B; probe.H = s.H; probe.S = s.S; probe.D = s.D; probe.ld = 3 * s.H * s.D; probe.ldo = s.H * s.D;
        if (s.bias || s.o8 || s.dtype || dk_attention_route(probe, ~(size_t)0, n_cu, r) != 0 || r.jobs == 0) continue;
        one(s, n_cu, (size_t)(r.jobs - 1) * DK_ATTN5_JOB_BYTES);
        one(s, n_cu, (size_t)r.jobs * DK_ATTN5_JOB_BYTES);
      }
  return 0;
}
