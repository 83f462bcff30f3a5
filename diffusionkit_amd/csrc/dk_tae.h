// The tiny latent decoder's kernels (tae.hip) as the host units see them (tae_engine.hip).
#pragma once
#include "dk_common.h"

#define DK_TAE_TILE 16      // output tile of every tae.hip kernel: 16 x 16 pixels of one image, all channels
#define DK_TAE_K64 576      // reduction of a 64-channel conv: 9 taps x 64 channels, 18 MFMA steps
#define DK_TAE_K16 160      // ... of the first conv: 9 taps x 16 channels = 144, zero-padded to 5 MFMA steps

enum { DK_TAE_FIRST = 0, DK_TAE_MID = 1, DK_TAE_LAST = 2 };

// One Block: y = ReLU(conv3(ReLU(conv2(ReLU(conv1(x))))) + x), x, y bf16 [B, H, W, 64], w[i] bf16 [64, 576] (tap-major), b[i] bf16 [64]
struct TaeBlockParams {
  const bf16_t* x;
  bf16_t* y;
  const bf16_t* w[3];
  const bf16_t* b[3];
  int B, H, W;
};

// One 3x3 conv, zero-padded by 1, on an output grid of [B, H, W]:
//   FIRST  xf f32 [B, H, W, 16] -> 3 tanh(((x - shift) scale) / 3) -> bf16; w [64, 160]; bias, ReLU                 -> y bf16 [B, H, W, 64]
//   MID    x bf16 [B, H >> ups, W >> ups, 64] (ups = 1: nearest x 2 as a view, H and W even); w [64, 576]; bias (or null), ReLU (or not),
//          skip bf16 [B, H, W, 64] (or null): out = ReLU?((acc + bias) + skip)                                        -> y bf16 [B, H, W, 64]
//   ups and skip belong to MID alone: the launcher refuses them for the other two.
//   LAST   x bf16 [B, H, W, 64]; w [16, 576] (rows 3.. zero); bias [16]                                               -> img f32 / u8 [B, H, W, 3]
struct TaeConvParams {
  const bf16_t* x;
  const float* xf;
  const bf16_t* w;
  const bf16_t* bias;
  const bf16_t* skip;
  bf16_t* y;
  float* img;
  unsigned char* u8;
  int B, H, W;
  int ups, relu;
  float scale, shift;
};

int dk_launch_tae_block(const TaeBlockParams& p, hipStream_t stream);
int dk_launch_tae_conv(int kind, const TaeConvParams& p, hipStream_t stream);
