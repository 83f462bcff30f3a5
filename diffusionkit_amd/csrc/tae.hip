// The tiny latent decoder (TAESD family: taesd3 / taef1): 3x3 convolutions on 64 channels, ReLU, nearest x 2 -- no GroupNorm, no attention.
// bf16 only, NHWC with 64 channels: a pixel is one 128-byte row.
//
// Why kernels of their own: conv_halo.hip / conv256v4.hip are built around GroupNorm-apply + SiLU, 128- / 256-channel tiles and one launch per
// conv.  A tiny decoder's widest activation is 128 MiB at 1024 x 1024 against 0.5 TFLOP of arithmetic: one launch per conv is bound by HBM and by
// the launch count.  dk_tae_block_kernel runs a whole residual Block (three convs, skip, ReLUs) per launch and keeps both intermediates in LDS.
//
// Frame shared by both kernels.  A workgroup owns a 16 x 16 output tile of one image over all 64 output channels.  The input pixels it needs lie
// in LDS as rows of 144 bytes (128 B of channels + 16 B pad: the 16 lanes of a fragment read 16 consecutive rows, 36 dwords apart, and cover the
// 64 banks exactly once).  A conv is an implicit GEMM: M = pixels, N = 64, K = 9 taps x 64 channels = 18 steps of v_mfma_f32_16x16x32_bf16,
// walked tap by tap, low 32 channels first -- in EVERY kernel of this file, so that the fused Block and a chain of single convs accumulate in the
// same order and agree bit for bit.  The taps read shifted windows of the LDS tile; there is no im2col buffer.
//
// Weights never enter LDS (22 x 22 + 20 x 20 pixel rows and one conv's 72 KB do not fit in 160 KB): a wave owns 32 output channels and holds
// that slice of the weight operand in registers for the whole conv -- 2 fragments x 18 steps x 4 = 144 VGPRs, loaded straight from global
// memory (a Block's 216 KB stay in L2 for every workgroup).  The weight fragment is the MFMA's A operand, the pixel fragment its B operand, so a
// lane ends up with 4 consecutive channels of one pixel: 8-byte packed stores into the next ring's LDS rows.
//
// dk_tae_block_kernel, 512 threads = 2 channel halves x 4 fragment groups:
//   input halo 22 x 22 (region A) -> conv1 -> ring 20 x 20 (region B) -> conv2 -> ring 18 x 18 (region A again: the input is dead, the skip
//   operand is read again from global in the last tail) -> conv3 (+ bias + x, ReLU in the accumulators) -> staged in region B -> whole 128-byte
//   pixel rows to global.  Recompute factor of the rings: (400 + 324 + 256) / 768 = 1.28.
//   Every conv pads ITS OWN input with zeros: a ring position outside the image is stored as zero, not as the value the conv in front would
//   compute there from the halo; positions past the right / bottom edge of a partial tile fall under the same rule.
//   Per tile: 25 + 21 + 16 = 62 pixel fragments; each is read by the 2 channel halves (18 ds_read_b128 of 1 KiB each) and multiplied by
//   2 x 36 MFMAs: 2232 LDS reads = 17.9 k LDS clocks against 4464 MFMAs x 16 clocks / 4 SIMDs = 17.9 k clocks -- a paper tie (four waves of
//   16 channels would read every fragment four times: LDS-bound by 2 x; a wave of 64 channels needs 288 weight registers).
// dk_tae_conv_kernel<KIND>, 256 threads, two workgroups per CU: one conv in the same frame (18 x 18 halo) --
//   FIRST  fp32 latent [.., 16] with (x - shift) * scale -> 3 tanh(. / 3) -> bf16 on the load; K = 144 padded to 160 (5 steps: a step spans two
//          taps of 16 channels, the tenth tap is a zero fragment); bias, ReLU
//   MID    64 -> 64; optional nearest x 2 (source pixel (y >> 1, x >> 1) at tile load: the upsampled image is never materialised), optional
//          bias / ReLU / skip: the chain form of a Block and the three upsampling convs
//   LAST   64 -> 3 (one 16-row weight fragment, rows 3.. zero) with the image tail in the accumulators.
// Rounding points: every conv's ReLU(acc + bias) is rounded to bf16 once (what a chain would have stored); a Block's output is
// round(ReLU((acc + bias) + x)).  Image tail, restated from conv_halo.hip's IMG case (which decodes clip(x / 2 + 0.5)): v = round_bf16(acc + bias),
// image = min(max(v, 0), 1) in fp32, byte = (unsigned char) round_bf16(image * 255) -- the product rounded to bf16, then truncated.
// Measured (profiles/tiny_decoder.md): the fused Block takes 0.628 ms at a 1024 x 1024 grid against 0.446 ms for its chain of three single convs
// (one workgroup of 8 waves per CU: weight loads, tile load, barriers and row stores are exposed), so the engine runs chains; the fused kernel is
// reachable as dk_tae_block_bf16 and through dk_tune_set("tae_block", 1).
// Addresses: every global offset is formed in size_t (no extent guard needed below the grid's 2^31 tiles).
#include "dk_kernels.h"
#include "dk_tae.h"

typedef __attribute__((address_space(3))) char lds_c;
#define TAE_LDS(T, OFF) (*(__attribute__((address_space(3))) T*)(lds + (OFF)))

#define TAE_P64 144  // LDS bytes of a 64-channel pixel row
#define TAE_P16 48   // ... of a 16-channel one (32 B + 16 B pad: 12 dwords apart, conflict-free as well)

// the tail every 64-column conv of this file shares (the fused Block's inner convs pass skip = 0)
__device__ __forceinline__ float tae_tail(float acc, float bias, float skip, bool relu) {
  const float v = (acc + bias) + skip;
  return relu ? fmaxf(v, 0.f) : v;
}

// this wave's slice of a weight matrix [.., K] -> registers: fragment nf = rows n0 + 16 nf .. + 15, step ks = columns 32 ks .. + 31
template <int NF, int KS>
__device__ __forceinline__ void tae_load_w(ex8 (&wf)[NF][KS], const bf16_t* w, int n0, int l15, int q) {
#pragma unroll
  for (int nf = 0; nf < NF; ++nf)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) wf[nf][ks] = *(const ex8*)(w + (size_t)(n0 + nf * 16 + l15) * (KS * 32) + ks * 32 + q * 8);
}
__device__ __forceinline__ void tae_load_bias(float (&b4)[4], const bf16_t* bias, int col) {
  if (bias) {
    const u32x2 v = *(const u32x2*)(bias + col);
    unpack2(v[0], b4[0], b4[1]);
    unpack2(v[1], b4[2], b4[3]);
  } else {
    b4[0] = b4[1] = b4[2] = b4[3] = 0.f;
  }
}

// 64-channel halo tile -> LDS: TH x TW pixels from (y0, x0) of the H x W view of an image stored [H >> ups, Ws, 64]; pixels outside the view
// become zeros.  (Loads are unconditional on a clamped pixel and selected afterwards: they issue back to back.)
template <int NT, int TH, int TW>
__device__ __forceinline__ void tae_load_tile64(lds_c* lds, unsigned dst, const bf16_t* xb, int Ws, int ups, int H, int W, int y0, int x0, int tid) {
  constexpr int ITEMS = TH * TW * 8, IT = (ITEMS + NT - 1) / NT;
  u32x4 v[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int id = tid + NT * i, pix = id >> 3, c8 = id & 7;
    const int hy = pix / TW, hx = pix - hy * TW;
    const int y = y0 + hy, x = x0 + hx;
    const bool ok = id < ITEMS && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
    const int yc = ok ? y : 0, xc = ok ? x : 0;
    v[i] = *(const u32x4*)(xb + ((size_t)(yc >> ups) * Ws + (xc >> ups)) * 64 + c8 * 8);
    if (!ok) v[i] = u32x4{0u, 0u, 0u, 0u};
  }
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int id = tid + NT * i;
    if (id < ITEMS) TAE_LDS(u32x4, dst + (id >> 3) * TAE_P64 + (id & 7) * 16) = v[i];
  }
}

// One conv over the RH x RW pixels whose 3x3 windows lie in an LDS tile: fragment f = ring pixels 16 f .. 16 f + 15 in row-major order (the last
// fragment's lanes past the ring compute on the last pixel and are dropped by the tail), fragments f = mg, mg + MG, ...
// frag(a, ks): the lane's B fragment of step ks for a window whose top-left pixel row starts at LDS byte a; tail(idx, ry, rx, acc).
template <int SW, int PITCH, int RW, int RH, int NF, int KS, int MG, class Frag, class Tail>
__device__ __forceinline__ void tae_ring_conv(unsigned src, const ex8 (&wf)[NF][KS], int mg, int l15, Frag&& frag, Tail&& tail) {
  constexpr int NPIX = RW * RH, NFRAG = (NPIX + 15) / 16;
  for (int f = mg; f < NFRAG; f += MG) {
    const int idx = f * 16 + l15;
    const int idc = idx < NPIX ? idx : NPIX - 1;
    const int ry = idc / RW, rx = idc - ry * RW;
    const unsigned a = src + (unsigned)((ry * SW + rx) * PITCH);
    f32x4 acc[NF];
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) acc[nf] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const ex8 b = frag(a, ks);
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) acc[nf] = mfma_16x16x32(wf[nf][ks], b, acc[nf]);
    }
    if (idx < NPIX) tail(idx, ry, rx, acc);
  }
}

// staging image of the output tile: 256 pixel rows of 128 B, the 16-byte chunk c of row r at position c ^ (r & 7)
__device__ __forceinline__ unsigned tae_stage_at(int pix, int col) {  // byte offset of column col (a multiple of 4) of pixel pix
  return (unsigned)(pix * 128 + (((col >> 3) ^ (pix & 7)) << 4) + (col & 7) * 2);
}
// staging image -> whole 128-byte pixel rows of y (the pixels of the tile that lie in the image)
template <int NT>
__device__ __forceinline__ void tae_store_tile(lds_c* lds, unsigned stage, bf16_t* yb, int H, int W, int y0, int x0, int tid) {
#pragma unroll
  for (int i = 0; i < 2048 / NT; ++i) {
    const int id = tid + NT * i, pix = id >> 3, c8 = id & 7;
    const int y = y0 + (pix >> 4), x = x0 + (pix & 15);
    if (y < H && x < W) *(u32x4*)(yb + ((size_t)y * W + x) * 64 + c8 * 8) = TAE_LDS(u32x4, stage + tae_stage_at(pix, c8 * 8));
  }
}

#define TAE_RA 0u
#define TAE_RB (22u * 22u * TAE_P64)
#define TAE_BLOCK_LDS (22 * 22 * TAE_P64 + 20 * 20 * TAE_P64)

__global__ __launch_bounds__(512) void dk_tae_block_kernel(TaeBlockParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_c* const lds = (lds_c*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ng = wave & 1, mg = wave >> 1;
  const int l15 = lane & 15, q = lane >> 4;
  const int n0 = ng * 32;

  const int tiles_x = (p.W + 15) >> 4, tiles_y = (p.H + 15) >> 4;
  const int bid = blockIdx.x;
  const int tx = bid % tiles_x, ty = (bid / tiles_x) % tiles_y, b = bid / (tiles_x * tiles_y);
  const int py0 = ty * 16, px0 = tx * 16;
  const size_t img = (size_t)b * p.H * p.W;  // first pixel of this image
  const int H = p.H, W = p.W;

  ex8 wf[2][18];
  float bias[2][4];
  const unsigned qoff = (unsigned)(q * 16);
  // the lane's B fragment of step ks: tap ks >> 1 = (dy, dx), channels 32 (ks & 1) + 8 q .. + 7
#define TAE_FRAG64(SW) [&](unsigned a, int ks) -> ex8 { \
    return TAE_LDS(ex8, a + qoff + (unsigned)((((ks >> 1) / 3) * (SW) + (ks >> 1) % 3) * TAE_P64 + (ks & 1) * 64)); }
  // ReLU(acc + bias) -> bf16 -> ring row idx at dst; zero where the ring position (origin py0 - ORG, px0 - ORG) lies outside the image
#define TAE_RING_TAIL(DST, ORG) [&](int idx, int ry, int rx, const f32x4 (&acc)[2]) {                                              \
    const bool in = (unsigned)(py0 - (ORG) + ry) < (unsigned)H && (unsigned)(px0 - (ORG) + rx) < (unsigned)W;                      \
    _Pragma("unroll") for (int nf = 0; nf < 2; ++nf) {                                                                             \
      float v[4];                                                                                                                  \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) v[e] = in ? tae_tail(acc[nf][e], bias[nf][e], 0.f, true) : 0.f;                \
      TAE_LDS(u32x2, (DST) + (unsigned)(idx * TAE_P64 + (n0 + nf * 16 + 4 * q) * 2)) = u32x2{pack2(v[0], v[1]), pack2(v[2], v[3])}; \
    }                                                                                                                              \
  }
#define TAE_CONV_SETUP(I)                                                                                     \
  tae_load_w(wf, p.w[I], n0, l15, q);                                                                         \
  _Pragma("unroll") for (int nf = 0; nf < 2; ++nf) tae_load_bias(bias[nf], p.b[I], n0 + nf * 16 + 4 * q)

  TAE_CONV_SETUP(0);
  tae_load_tile64<512, 22, 22>(lds, TAE_RA, p.x + img * 64, W, 0, H, W, py0 - 3, px0 - 3, tid);
  __syncthreads();
  tae_ring_conv<22, TAE_P64, 20, 20, 2, 18, 4>(TAE_RA, wf, mg, l15, TAE_FRAG64(22), TAE_RING_TAIL(TAE_RB, 2));
  TAE_CONV_SETUP(1);  // (in flight across the barrier)
  __syncthreads();    // ring 1 complete; the input tile is dead
  tae_ring_conv<20, TAE_P64, 18, 18, 2, 18, 4>(TAE_RB, wf, mg, l15, TAE_FRAG64(20), TAE_RING_TAIL(TAE_RA, 1));
  TAE_CONV_SETUP(2);
  __syncthreads();    // ring 2 complete; ring 1 is dead: its space takes the staged output
  tae_ring_conv<18, TAE_P64, 16, 16, 2, 18, 4>(TAE_RA, wf, mg, l15, TAE_FRAG64(18), [&](int idx, int ry, int rx, const f32x4 (&acc)[2]) {
    const int y = py0 + ry, x = px0 + rx;
    if (y >= H || x >= W) return;  // (never stored)
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      const int col = n0 + nf * 16 + 4 * q;
      const u32x2 sv = *(const u32x2*)(p.x + (img + (size_t)y * W + x) * 64 + col);
      float s[4], v[4];
      unpack2(sv[0], s[0], s[1]);
      unpack2(sv[1], s[2], s[3]);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = tae_tail(acc[nf][e], bias[nf][e], s[e], true);
      TAE_LDS(u32x2, TAE_RB + tae_stage_at(idx, col)) = u32x2{pack2(v[0], v[1]), pack2(v[2], v[3])};
    }
  });
  __syncthreads();
  tae_store_tile<512>(lds, TAE_RB, p.y + img * 64, H, W, py0, px0, tid);
#undef TAE_RING_TAIL
#undef TAE_CONV_SETUP
}

// LDS of the single convs: the 18 x 18 halo tile, then (64-column outputs) the staging image
constexpr unsigned TAE_CONV_STAGE(int kind) { return kind == DK_TAE_FIRST ? 18u * 18u * TAE_P16 : 18u * 18u * TAE_P64; }
constexpr unsigned TAE_CONV_LDS(int kind) { return TAE_CONV_STAGE(kind) + (kind == DK_TAE_LAST ? 0u : 256u * 128u); }

template <int KIND>
__global__ __launch_bounds__(256, 2) void dk_tae_conv_kernel(TaeConvParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_c* const lds = (lds_c*)smem;
  constexpr int NF = KIND == DK_TAE_LAST ? 1 : 2;     // 16-row weight fragments of a wave
  constexpr int MG = KIND == DK_TAE_LAST ? 4 : 2;     // fragment groups
  constexpr int KS = KIND == DK_TAE_FIRST ? 5 : 18;
  constexpr unsigned STAGE = TAE_CONV_STAGE(KIND);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ng = KIND == DK_TAE_LAST ? 0 : (wave & 1), mg = KIND == DK_TAE_LAST ? wave : (wave >> 1);
  const int l15 = lane & 15, q = lane >> 4;
  const int n0 = ng * 32;

  const int H = p.H, W = p.W;
  const int tiles_x = (W + 15) >> 4, tiles_y = (H + 15) >> 4;
  const int bid = blockIdx.x;
  const int tx = bid % tiles_x, ty = (bid / tiles_x) % tiles_y, b = bid / (tiles_x * tiles_y);
  const int py0 = ty * 16, px0 = tx * 16;
  const size_t img = (size_t)b * H * W;

  ex8 wf[NF][KS];
  float bias[NF][4];
  tae_load_w(wf, p.w, n0, l15, q);
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) tae_load_bias(bias[nf], p.bias, n0 + nf * 16 + 4 * q);

  if constexpr (KIND == DK_TAE_FIRST) {
    // 18 x 18 pixels x 2 halves of 8 channels: fp32 -> (x - shift) * scale -> 3 tanh(. / 3) -> bf16; padding is zero AFTER the transform
    constexpr int ITEMS = 18 * 18 * 2, IT = (ITEMS + 255) / 256;
    f32x4 v[IT][2];
    bool okv[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int id = tid + 256 * i, pix = id >> 1, h8 = id & 1;
      const int hy = pix / 18, hx = pix - hy * 18;
      const int y = py0 - 1 + hy, x = px0 - 1 + hx;
      okv[i] = id < ITEMS && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
      const float* src = p.xf + (img + (okv[i] ? (size_t)y * W + x : 0)) * 16 + h8 * 8;
      v[i][0] = *(const f32x4*)src;
      v[i][1] = *(const f32x4*)(src + 4);
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int id = tid + 256 * i;
      float t[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = okv[i] ? 3.0f * tanhf((v[i][e >> 2][e & 3] - p.shift) * p.scale * (1.0f / 3.0f)) : 0.f;
      if (id < ITEMS)
        TAE_LDS(u32x4, (id >> 1) * TAE_P16 + (id & 1) * 16) = u32x4{pack2(t[0], t[1]), pack2(t[2], t[3]), pack2(t[4], t[5]), pack2(t[6], t[7])};
    }
  } else {
    const int Hs = H >> p.ups, Ws = W >> p.ups;
    tae_load_tile64<256, 18, 18>(lds, 0u, p.x + (size_t)b * Hs * Ws * 64, Ws, p.ups, H, W, py0 - 1, px0 - 1, tid);
  }
  __syncthreads();

  if constexpr (KIND == DK_TAE_FIRST) {
    // step ks spans taps 2 ks and 2 ks + 1 (16 channels each): lane quarter q reads tap 2 ks + (q >> 1), channels 8 (q & 1) .. + 7
    auto frag = [&](unsigned a, int ks) -> ex8 {
      const int tap = 2 * ks + (q >> 1);
      const int tc = tap < 9 ? tap : 8;
      const ex8 v = TAE_LDS(ex8, a + (unsigned)(((tc / 3) * 18 + tc % 3) * TAE_P16 + (q & 1) * 16));
      return tap < 9 ? v : __builtin_bit_cast(ex8, u32x4{0u, 0u, 0u, 0u});
    };
    tae_ring_conv<18, TAE_P16, 16, 16, NF, KS, MG>(0u, wf, mg, l15, frag, [&](int idx, int ry, int rx, const f32x4 (&acc)[NF]) {
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        const int col = n0 + nf * 16 + 4 * q;
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = tae_tail(acc[nf][e], bias[nf][e], 0.f, true);
        TAE_LDS(u32x2, STAGE + tae_stage_at(idx, col)) = u32x2{pack2(o[0], o[1]), pack2(o[2], o[3])};
      }
    });
  } else {
    const unsigned qoff = (unsigned)(q * 16);
    auto frag = TAE_FRAG64(18);
    if constexpr (KIND == DK_TAE_MID) {
      const bool relu = p.relu != 0;
      tae_ring_conv<18, TAE_P64, 16, 16, NF, KS, MG>(0u, wf, mg, l15, frag, [&](int idx, int ry, int rx, const f32x4 (&acc)[NF]) {
        const int y = py0 + ry, x = px0 + rx;
        if (y >= H || x >= W) return;
#pragma unroll
        for (int nf = 0; nf < NF; ++nf) {
          const int col = n0 + nf * 16 + 4 * q;
          float s[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
          if (p.skip) {
            const u32x2 sv = *(const u32x2*)(p.skip + (img + (size_t)y * W + x) * 64 + col);
            unpack2(sv[0], s[0], s[1]);
            unpack2(sv[1], s[2], s[3]);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = tae_tail(acc[nf][e], bias[nf][e], s[e], relu);
          TAE_LDS(u32x2, STAGE + tae_stage_at(idx, col)) = u32x2{pack2(o[0], o[1]), pack2(o[2], o[3])};
        }
      });
    } else {
      // the image tail: channels 0 .. 2 of the one fragment sit in the q == 0 lanes
      tae_ring_conv<18, TAE_P64, 16, 16, NF, KS, MG>(0u, wf, mg, l15, frag, [&](int idx, int ry, int rx, const f32x4 (&acc)[NF]) {
        const int y = py0 + ry, x = px0 + rx;
        if (q != 0 || y >= H || x >= W) return;
        const size_t pix = img + (size_t)y * W + x;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          const float im = fminf(fmaxf(round_act(acc[0][e] + bias[0][e]), 0.f), 1.f);
          if (p.img) p.img[pix * 3 + e] = im;
          if (p.u8) p.u8[pix * 3 + e] = (unsigned char)round_act(im * 255.0f);
        }
      });
    }
  }
  if constexpr (KIND != DK_TAE_LAST) {
    __syncthreads();
    tae_store_tile<256>(lds, STAGE, p.y + img * 64, H, W, py0, px0, tid);
  }
}
#undef TAE_FRAG64

static bool tae_al16(const void* q) { return ((uintptr_t)q & 15) == 0; }

static int tae_grid(int B, int H, int W, unsigned* tiles) {
  DK_REQUIRE(B >= 1 && H >= 1 && W >= 1, "tae: batch, height and width of the output grid must be positive");
  const unsigned long long t = (unsigned long long)B * ((H + 15) / 16) * ((W + 15) / 16);
  DK_REQUIRE(t < (1ull << 31), "tae: more than 2^31 - 1 output tiles of 16 x 16 pixels");
  *tiles = (unsigned)t;
  return 0;
}

int dk_launch_tae_block(const TaeBlockParams& p, hipStream_t stream) {
  DK_REQUIRE(p.x && p.y && p.x != p.y, "tae_block: x and y must be two buffers (a tile reads its neighbours' input)");
  for (int i = 0; i < 3; ++i)
    DK_REQUIRE(p.w[i] && p.b[i] && tae_al16(p.w[i]) && tae_al16(p.b[i]), "tae_block: three weights [64, 576] and biases [64], 16-byte aligned");
  DK_REQUIRE(tae_al16(p.x) && tae_al16(p.y), "tae_block: x / y must be 16-byte aligned");
  unsigned tiles = 0;
  if (const int rc = tae_grid(p.B, p.H, p.W, &tiles)) return rc;
  static DkDeviceOnce attr_once;
  if (attr_once.first()) {
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_tae_block_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, TAE_BLOCK_LDS));
    attr_once.mark();
  }
  dk_prof_begin(1, 3.0 * 2.0 * p.B * p.H * p.W * 576.0 * 64.0, stream);
  hipLaunchKernelGGL(dk_tae_block_kernel, dim3(tiles), dim3(512), TAE_BLOCK_LDS, stream, p);
  dk_prof_end(stream);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}

int dk_launch_tae_conv(int kind, const TaeConvParams& p, hipStream_t stream) {
  DK_REQUIRE(kind == DK_TAE_FIRST || kind == DK_TAE_MID || kind == DK_TAE_LAST, "tae_conv: kind 0 first, 1 64 -> 64, 2 last");
  DK_REQUIRE(p.w && tae_al16(p.w) && tae_al16(p.bias), "tae_conv: weight (and bias) 16-byte aligned");
  unsigned tiles = 0;
  if (const int rc = tae_grid(p.B, p.H, p.W, &tiles)) return rc;
  static DkDeviceOnce attr_once;
  if (attr_once.first()) {
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_tae_conv_kernel<DK_TAE_FIRST>, hipFuncAttributeMaxDynamicSharedMemorySize, TAE_CONV_LDS(DK_TAE_FIRST)));
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_tae_conv_kernel<DK_TAE_MID>, hipFuncAttributeMaxDynamicSharedMemorySize, TAE_CONV_LDS(DK_TAE_MID)));
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_tae_conv_kernel<DK_TAE_LAST>, hipFuncAttributeMaxDynamicSharedMemorySize, TAE_CONV_LDS(DK_TAE_LAST)));
    attr_once.mark();
  }
  const double px = (double)p.B * p.H * p.W;
  if (kind == DK_TAE_FIRST) {
    DK_REQUIRE(p.xf && p.y && p.bias && tae_al16(p.xf) && tae_al16(p.y), "tae_conv first: f32 latent, bias and bf16 output, 16-byte aligned");
    DK_REQUIRE(p.ups == 0 && p.skip == nullptr, "tae_conv first: upsample and skip belong to the 64 -> 64 form (kind 1)");
    dk_prof_begin(1, 2.0 * px * 144.0 * 64.0, stream);
    hipLaunchKernelGGL(dk_tae_conv_kernel<DK_TAE_FIRST>, dim3(tiles), dim3(256), TAE_CONV_LDS(DK_TAE_FIRST), stream, p);
  } else if (kind == DK_TAE_MID) {
    DK_REQUIRE(p.x && p.y && p.x != p.y && tae_al16(p.x) && tae_al16(p.y) && tae_al16(p.skip), "tae_conv: x and y two buffers, 16-byte aligned");
    DK_REQUIRE(p.ups == 0 || (p.ups == 1 && p.H % 2 == 0 && p.W % 2 == 0), "tae_conv: upsample 0, or 1 with an even output grid");
    dk_prof_begin(1, 2.0 * px * 576.0 * 64.0, stream);
    hipLaunchKernelGGL(dk_tae_conv_kernel<DK_TAE_MID>, dim3(tiles), dim3(256), TAE_CONV_LDS(DK_TAE_MID), stream, p);
  } else {
    DK_REQUIRE(p.x && p.bias && (p.img || p.u8) && tae_al16(p.x), "tae_conv last: bf16 input, bias, and an f32 or u8 image");
    DK_REQUIRE(p.ups == 0 && p.skip == nullptr, "tae_conv last: upsample and skip belong to the 64 -> 64 form (kind 1)");
    dk_prof_begin(1, 2.0 * px * 576.0 * 3.0, stream);
    hipLaunchKernelGGL(dk_tae_conv_kernel<DK_TAE_LAST>, dim3(tiles), dim3(256), TAE_CONV_LDS(DK_TAE_LAST), stream, p);
  }
  dk_prof_end(stream);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}
