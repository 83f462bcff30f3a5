// bf16 MFMA GEMM for gfx950: C = epi(alpha * A . W^T + bias), fp32 accumulate.
//
// Replaces every nn.Linear / nn.Conv2d call site of the reference hot path
// (python/src/diffusionkit/mlx/mmdit.py:56,285,358-360,373-375,432,771,777,821-832;
//  python/src/diffusionkit/mlx/vae.py:36-39,73,79,84,134,349,384).
//
// Tile: 128(M) x 128(N) x 64(K) per 256-thread workgroup (4 waves as 2x2, 64x64 per wave,
// v_mfma_f32_32x32x16_bf16).  Both operands are K-major, staged HBM -> LDS with
// global_load_lds_dwordx4 (no VGPR round trip) into a double-buffered 2 x 32 KiB image.
// The LDS image is lane-linear (a DMA constraint); bank conflicts on the ds_read_b128
// fragment reads are removed by XOR-ing the 16-byte chunk index with (row>>1)&7 on the
// *source* address and again on the read (same involution both sides).
// The MFMA is issued with operands swapped (W-fragment as A, X-fragment as B) so each lane
// ends up owning one output row and 4-element runs of consecutive columns: the epilogue
// (bias, GELU, gate*x+residual) then works on 8-byte vectors.
// AMODE=1 turns the A loader into an im2col gather for 3x3 convolution over NHWC: pad 1 / stride 1
// (optionally reading a nearest-x2-upsampled view), or stride 2 over the input padded by one row and
// column at the bottom / right (the VAE encoder's downsample, vae.py:141-143); padding taps read a zero page.
#include "dk_kernels.h"

#define BM 128
#define BN 128
#define BK 64
#define A_TILE_BYTES (BM * BK * 2)
#define B_TILE_BYTES (BN * BK * 2)
#define STAGE_BYTES (A_TILE_BYTES + B_TILE_BYTES)

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;

__device__ __forceinline__ int lds_row_off(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

template <int AMODE>
__global__ __launch_bounds__(256) void dk_gemm_bf16_kernel(GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int hi = lane >> 5, l31 = lane & 31;

  // ---- workgroup -> tile: XCD-contiguous chunks, then 8-row groups (A/W panels shared in L2) ----
  const int nbm = (p.M + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
  const int nwg = nbm * nbn;
  int t;
  {
    const int bid = blockIdx.x;
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int GROUP = 8;
  const int tpg = GROUP * nbn;
  const int g = t / tpg;
  const int first_m = g * GROUP;
  const int gsz = min(nbm - first_m, GROUP);
  const int tm = first_m + (t % tpg) % gsz;
  const int tn = (t % tpg) / gsz;
  const int m0 = tm * BM, n0 = tn * BN;

  // ---- per-lane source pointers for the DMA loads (4 A + 4 W row-instructions per wave) ----
  const bf16_t* a_src[4];
  const bf16_t* w_src[4];
  int cy[4], cx[4];       // conv: output pixel coordinates of this lane's rows
  long cimg[4];           // conv: image base (elements)
  const int srow = lane >> 3;  // row within an 8-row instruction
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = wave * 32 + i * 8 + srow;  // tile-local row
    const int chunk = (lane & 7) ^ ((r >> 1) & 7);
    int n = min(n0 + r, p.N - 1);
    w_src[i] = p.W + (size_t)n * p.ldw + chunk * 8;
    int m = min(m0 + r, p.M - 1);
    if (AMODE == 0) {
      const int phys = (m / p.a_seg_len) * p.a_seg_stride + (m % p.a_seg_len);
      a_src[i] = p.A + (size_t)phys * p.lda + chunk * 8;
    } else {
      const int hw = p.cH * p.cW;
      const int b = m / hw, rem = m - b * hw;
      cy[i] = rem / p.cW;
      cx[i] = rem - cy[i] * p.cW;
      // stored input size: ups 1 = nearest-x2 view of a half-size tensor, ups 2 = stride-2 conv over a double-size one
      const int Hs = p.ups == 1 ? (p.cH >> 1) : p.ups == 2 ? (p.cH << 1) : p.cH;
      const int Ws = p.ups == 1 ? (p.cW >> 1) : p.ups == 2 ? (p.cW << 1) : p.cW;
      cimg[i] = (long)b * Hs * Ws * p.cC + chunk * 8;
      a_src[i] = p.zeros + chunk * 8;
    }
  }

  const int nk = p.K / BK;
  const int cpt = (AMODE == 1) ? (p.cC / BK) : 1;  // K-tiles per conv tap

  auto issue = [&](int kt, int buf) {
    char* abase = smem + buf * STAGE_BYTES + (wave * 32) * 128;
    char* bbase = abase + A_TILE_BYTES;
    if (AMODE == 1) {
      const int tap = kt / cpt, cb = (kt - tap * cpt) * BK;
      const int ky = tap / 3 - 1, kx = tap - (tap / 3) * 3 - 1;
      const int Ws = p.ups == 1 ? (p.cW >> 1) : p.ups == 2 ? (p.cW << 1) : p.cW;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int iy = cy[i] + ky, ix = cx[i] + kx;
        bool ok = (iy >= 0) && (iy < p.cH) && (ix >= 0) && (ix < p.cW);
        int sy = p.ups == 1 ? (iy >> 1) : iy, sx = p.ups == 1 ? (ix >> 1) : ix;
        if (p.ups == 2) {  // stride 2 over the input padded by one row / column at the bottom / right (vae.py:141-143)
          sy = 2 * cy[i] + ky + 1, sx = 2 * cx[i] + kx + 1;
          ok = sy < 2 * p.cH && sx < 2 * p.cW;
        }
        const bf16_t* src = ok ? (p.A + cimg[i] + ((long)sy * Ws + sx) * p.cC + cb) : a_src[i];
        __builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(abase + i * 1024), 16, 0, 0);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_global_load_lds((gbl_ptr_t)(a_src[i] + kt * BK), (lds_ptr_t)(abase + i * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_global_load_lds((gbl_ptr_t)(w_src[i] + kt * BK), (lds_ptr_t)(bbase + i * 1024), 16, 0, 0);
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  issue(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < nk) issue(kt + 1, buf ^ 1);
    const char* As = smem + buf * STAGE_BYTES;
    const char* Bs = As + A_TILE_BYTES;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int c = kk * 2 + hi;
      ex8 wf[2], xf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        wf[i] = *(const ex8*)(Bs + lds_row_off(wn * 64 + i * 32 + l31, c));
        xf[i] = *(const ex8*)(As + lds_row_off(wm * 64 + i * 32 + l31, c));
      }
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
          acc[ni][mi] = mfma_32x32x16(wf[ni], xf[mi], acc[ni][mi]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- epilogue: lane owns row m (per mi) and columns nb + {0..3} per (ni, g) ----
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int m = m0 + wm * 64 + mi * 32 + l31;
    if (m >= p.M) continue;
    const size_t crow = (size_t)((m / p.c_seg_len) * p.c_seg_stride + (m % p.c_seg_len)) * p.ldc;
    size_t rrow = 0;
    const bf16_t* gate = nullptr;
    if (p.epi == DK_EPI_GATE_RES || p.epi == DK_EPI_RES)
      rrow = (size_t)((m / p.r_seg_len) * p.r_seg_stride + (m % p.r_seg_len)) * p.ldr;
    if (p.epi == DK_EPI_GATE_RES) gate = p.gate + (size_t)(m / p.gate_seg_len) * p.gate_stride;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int nb = n0 + wn * 64 + ni * 32 + 8 * g4 + 4 * hi;
        if (nb >= p.N) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[ni][mi][4 * g4 + e] * p.alpha;
        const bool full = (nb + 3 < p.N);
        if (full) {
          if (p.bias) {
            const uint2 bb = *(const uint2*)(p.bias + nb);
            float b0, b1, b2, b3;
            unpack2(bb.x, b0, b1);
            unpack2(bb.y, b2, b3);
            v[0] += b0; v[1] += b1; v[2] += b2; v[3] += b3;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = round_act(v[e]);
          if (p.epi == DK_EPI_BIAS_GELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = gelu_erf_f(v[e]);
          } else if (p.epi == DK_EPI_BIAS_SILU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = silu_f(v[e]);
          } else if (p.epi == DK_EPI_GATE_RES || p.epi == DK_EPI_RES) {
            const uint2 rr = *(const uint2*)(p.res + rrow + nb);
            float r0, r1, r2, r3;
            unpack2(rr.x, r0, r1);
            unpack2(rr.y, r2, r3);
            if (p.epi == DK_EPI_GATE_RES) {
              const uint2 gg = *(const uint2*)(gate + nb);
              float g0, g1, g2, g3;
              unpack2(gg.x, g0, g1);
              unpack2(gg.y, g2, g3);
              v[0] = r0 + round_act(g0 * v[0]);
              v[1] = r1 + round_act(g1 * v[1]);
              v[2] = r2 + round_act(g2 * v[2]);
              v[3] = r3 + round_act(g3 * v[3]);
            } else {
              v[0] += r0; v[1] += r1; v[2] += r2; v[3] += r3;
            }
          }
          uint2 o;
          o.x = pack2(v[0], v[1]);
          o.y = pack2(v[2], v[3]);
          *(uint2*)(p.C + crow + nb) = o;
        } else {
          for (int e = 0; e < 4 && nb + e < p.N; ++e) {
            float x = v[e];
            if (p.bias) x += to_f32(p.bias[nb + e]);
            x = round_act(x);
            if (p.epi == DK_EPI_BIAS_GELU) x = gelu_erf_f(x);
            else if (p.epi == DK_EPI_BIAS_SILU) x = silu_f(x);
            else if (p.epi == DK_EPI_GATE_RES) x = to_f32(p.res[rrow + nb + e]) + round_act(to_f32(gate[nb + e]) * x);
            else if (p.epi == DK_EPI_RES) x += to_f32(p.res[rrow + nb + e]);
            p.C[crow + nb + e] = from_f32(x);
          }
        }
      }
    }
  }
}

#ifndef DK_ELEM_F16  // (gemm_f16.hip compiles the kernel above and its launcher below a second time, inside namespace dk_f16)
// ---------------- routing: kernel, tile height and K split of one call (dk_gemm_route), read by the launches and by dk_gemm_plan ----------------

// tuning knob (dk_tune_set("gemm", v)): -1 = automatic choice, 128 = always the 128^2-tile kernel of this file, 9 = the 256^2 kernel
// (gemm256v3.hip) on every shape it accepts, 10 = the one-wave-per-SIMD 256^2 kernel (gemm256v4.hip) on every shape IT accepts (others: 9)
int g_dk_gemm_mode = -1;
int g_dk_pair_split_nk = -1;  // dk_tune_set("gemm_pair_nk", v): K-tile steps from which an image + text pair whose extra round is a small remainder is grouped and cut along K; -1: 24 (32 until the raw-accumulator exchange of round 6: profiles/r06_gemm_pair_nk.log)
int g_dk_v4_auto = -1;  // dk_tune_set("gemm_v4", v): -1 (default) the rule in use_v4, 0 never in the automatic choice (A/B runs)
// dk_tune_set("gemm_split", v): -1 (default) split a remainder wave of at most half the CUs into equal pieces when the
// cost model below says it pays, 0 never, 1 whenever possible.  Kernel lab (profiles/archive/r01_gemm_lab.md): every workgroup
// carries ~18 us of fixed cost (launch, first DMA, tail) and a CU runs its K-tiles ~20 % slower when all 256 CUs are busy
// than when 192 are, so a remainder of MORE than half the CUs (finisher + several producer pieces in turn on the
// spare CUs) loses on every shape but the longest-K one and is only taken when forced.
int g_dk_v3_split = -1;
int g_dk_v3_split_min = -1;  // dk_tune_set("gemm_split_min", v): saved K-tile steps below which a Linear that is ALL remainder stays whole; -1: 32 (see dk_plan_split)
// dk_tune_set("gemm_mf", v): wave-tile height in 16-row fragments; -1 (default) = the height with the fewest rounds x height, 8 / 7 forced
int g_dk_v3_mf = -1;

SplitPlan dk_plan_split(int tiles, int nk, bool have_ws, int n_cu, bool linear) {
  SplitPlan none{tiles, 0, 1, nk};
  if (!have_ws || g_dk_v3_split == 0 || n_cu < 16) return none;
  const int G = n_cu & ~7;
  const int T = tiles % G;
  if (T == 0) return none;
  const int E = G - T;
  int S, ks, t_steps;  // t_steps: K-tile steps until the split wave is done
  if (T > G / 2) {  // one producer piece per tile, c = ceil(T / E) of them in turn on each of the E spare CUs
    if (g_dk_v3_split < 0) return none;
    S = 2;
    const int c = (T + E - 1) / E;
    ks = (nk * c + c) / (c + 1);  // ~ nk * c / (c + 1), rounded up: the finishers must not end before the producers
    if (ks > nk - 1) ks = nk - 1;
    t_steps = ks > c * (nk - ks) ? ks : c * (nk - ks);
  } else {  // S equal pieces per tile, one CU each
    S = G / T < 4 ? G / T : 4;
    ks = (nk + S - 1) / S;
    t_steps = ks;
  }
  if (S < 2 || ks < 1 || nk - ks < S - 1 || T * (S - 1) > DK_KSPLIT_SLABS) return none;
  // a K-tile step costs about 1.45 us; splitting costs a slab write + read and a flag round trip per tile
  if (g_dk_v3_split < 0 && (nk - t_steps) * 1.45 < 25.0) return none;
  // a Linear that is ALL remainder (round 6: FLUX / SD3 below 1024 x 1024, 60 - 120 tiles): every tile pays S - 1 slab round trips at once, and the few
  // busy CUs run their K-tiles in ~1 us.  Measured (profiles/r06_gemm_small_m.log, r06_res_sweep.md): with the fp32-image exchange of rounds 1-5 FLUX's o_proj at
  // 512 x 512 (K = 3072, four ranges: 36 steps saved) lost 16 us with the split and fc2 / linear2 (144 / 180 saved) gained 60 - 90; with the raw-accumulator
  // exchange (gemm256v3.hip, round 6) the in-model sweep is flat from 0 to 48 saved steps and 1 % better at 24 - 36 than at 48: the rule cuts from 32
  if (g_dk_v3_split < 0 && linear && tiles < G && nk - t_steps < (g_dk_v3_split_min >= 0 ? g_dk_v3_split_min : 32)) return none;
  return SplitPlan{tiles - T, T, S, ks};
}

// a launch of `kernel` with bm x bn tiles over p (and p2), not split
static GemmRoute tile_route(int kernel, int bm, int bn, const GemmParams& p, const GemmParams* p2, int n_cu) {
  GemmRoute r;
  r.kernel = kernel;
  r.tile_rows = bm;
  r.tiles_a = ((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn);
  r.tiles_b = p2 ? ((p2->M + bm - 1) / bm) * ((p2->N + bn - 1) / bn) : 0;
  r.n_cu = n_cu;
  r.split = SplitPlan{r.tiles_a + r.tiles_b, 0, 1, p.K / BK};
  return r;
}
static long tiles256(const GemmParams& p, const GemmParams* p2, int bm) {
  long tiles = (long)((p.M + bm - 1) / bm) * ((p.N + 255) / 256);
  if (p2) tiles += (long)((p2->M + bm - 1) / bm) * ((p2->N + 255) / 256);
  return tiles;
}

// Tile height of the 256-column kernels.  Model: rounds of the CUs x rows per tile, over both problems of a grouped launch (same N).  Measured
// (profiles/r02_gemm_tile_height.log): on the FLUX shapes 224-row tiles save 2.7 % of the GEMM time -- far less than the 12.5 %
// the model promises, because a K-tile runs slower the more CUs are busy (the chip is power / fabric bound) -- and on
// the short-K SD3 shapes the 15 % extra tiles (each with its fixed prologue + tail) cost more than the fuller round gives back.
// So: 224-row tiles only for long reductions, and only when the model predicts at least 10 %.
static int fewest_rounds_mf(const GemmParams& p, const GemmParams* p2, int n_cu) {
  long cost[2];
  for (int mf = 7; mf <= 8; ++mf) {
    const int bm = 32 * mf;
    cost[mf - 7] = ((tiles256(p, p2, bm) + n_cu - 1) / n_cu) * bm;
  }
  return cost[0] * 10 <= cost[1] * 9 ? 7 : 8;
}

// gemm256v3.hip: the tile height, then the K split of the remainder wave
static GemmRoute route_v3(const GemmParams& p, const GemmParams* p2, int n_cu) {
  const bool have_ws = dk_ksplit_ws_ok(p, p2);
  const int nk = p.K / BK;
  int mf = 8;
  if (g_dk_v3_mf == 7 || g_dk_v3_mf == 8) {
    mf = g_dk_v3_mf;
  } else if (p.K >= 2048) {
    // Small launches (round 6; the reference CLI's 512 x 512 default: FLUX's o_proj / fc2 / linear2 are 60 - 84 tiles for 256 CUs): when both
    // heights leave at least half the CUs idle the launch is one split "remainder", and what a CU runs is the finisher piece: ks K-tiles of bm rows
    const long t7 = tiles256(p, p2, 224), t8 = tiles256(p, p2, 256);
    SplitPlan s7{}, s8{};
    if (have_ws && !p.conv && (t7 < t8 ? t7 : t8) * 2 <= n_cu && t7 <= n_cu && t8 <= n_cu) {
      s7 = dk_plan_split((int)t7, nk, true, n_cu, true);
      s8 = dk_plan_split((int)t8, nk, true, n_cu, true);
    }
    if (s7.n_rem > 0 || s8.n_rem > 0)
      mf = 224L * (s7.n_rem > 0 ? s7.ks : nk) < 256L * (s8.n_rem > 0 ? s8.ks : nk) ? 7 : 8;
    else
      mf = fewest_rounds_mf(p, p2, n_cu);
  }
  GemmRoute r = tile_route(3, 32 * mf, 256, p, p2, n_cu);
  r.split = dk_plan_split(r.tiles_a + r.tiles_b, nk, have_ws, n_cu, !p.conv);
  return r;
}

// gemm256v4.hip: every row tile of height bm lies inside one segment of every row map (its tile-uniform tail paths: FAST, or CUT for the last one)
static bool uniform_tiles(const GemmParams& p, int bm) {
  auto ok = [&](int len) { return len >= p.M || len % bm == 0; };
  const bool res = p.epi == DK_EPI_GATE_RES || p.epi == DK_EPI_RES || (p.n_split > 0 && (p.epi2 == DK_EPI_GATE_RES || p.epi2 == DK_EPI_RES));
  const bool gate = p.epi == DK_EPI_GATE_RES || (p.n_split > 0 && p.epi2 == DK_EPI_GATE_RES);
  return ok(p.a_seg_len) && ok(p.c_seg_len) && (!res || ok(p.r_seg_len)) && (!gate || ok(p.gate_seg_len)) && (p.kn_w == nullptr || ok(p.kn_seg_len));
}
// gemm256v4.hip (both problems eligible): gemm256v3.hip's height rule without the K split, 256-row tiles where a 224-row tile would straddle a segment
static GemmRoute route_v4(const GemmParams& p, const GemmParams* p2, int n_cu) {
  int mf = 8;
  if (g_dk_v3_mf == 7 || g_dk_v3_mf == 8)
    mf = g_dk_v3_mf;
  else if (p.K >= 2048 && uniform_tiles(p, 224) && (p2 == nullptr || uniform_tiles(*p2, 224)))  // (the per-row tail path is slow there)
    mf = fewest_rounds_mf(p, p2, n_cu);
  return tile_route(4, 32 * mf, 256, p, p2, n_cu);
}

// gemm256v4.hip is a bf16 kernel (generated asm body): an fp16 launch never goes there, whatever dk_tune_set("gemm", 10) / ("gemm_v4", v) say
static bool v4_ok(const GemmParams& p) { return p.dtype == DK_DTYPE_BF16 && dk_gemm256v4_eligible(p); }

// Which of the two 256^2 kernels takes a launch both accept (v3 / v4: its route on each).  gemm256v4.hip (one wave per SIMD, asm body) runs its K loop
// 5-7 % faster (profiles/r05_gemm_v4_*.log: 8192^3 1587 against 1488 TF with cold weights, the model's linear1 / linear2 / fc1 / fc2 +4-5 %), but has no
// remainder handling: gemm256v3.hip keeps the launches whose last round of the CUs is a small remainder (its 224-row tiles and the
// remainder-wave K split fill those: the q / k / v projections at 2.25-2.4 rounds, the grouped image + text fc1 at 3.2).
static bool use_v4(const GemmParams& p, const GemmParams* p2, const GemmRoute& v3, const GemmRoute& v4) {
  if (g_dk_gemm_mode != 10 && (g_dk_gemm_mode != -1 || g_dk_v4_auto == 0)) return false;
  if (g_dk_gemm_mode == 10) return true;
  const int n_cu = v3.n_cu;
  // Small launches (round 6): at most half a round of tiles, and gemm256v3.hip would cut every one of them along K -- FLUX at the reference CLI's
  // 512 x 512 default: o_proj / fc2 / linear2 are 60 - 84 tiles on 256 CUs, linear2 229 us on this kernel (profiles/r06_flux_512_kernel_stats_before.md)
  // (the one-wave-per-SIMD kernel has no K split, and 60 tiles on 256 CUs waste three quarters of the chip)
  const bool v3_cuts_all = (long)(v3.tiles_a + v3.tiles_b) * 2 <= n_cu && v3.split.n_rem > 0 && v3.split.n_dp == 0;
  if (g_dk_v4_auto != 2 && v3_cuts_all) return false;
  // launches with tiles that straddle row segments or short reductions with ragged rows stay on gemm256v3.hip: this kernel's per-row tail path
  // is slow (the lab's 1178 x 6144 x 1536 text fc1: 80 us here against 49 there) and its fixed cost per tile ~ 1 us higher (SD3-medium in the
  // model: every eligible launch 22.0 against 21.5 ms per step, whole-tile launches only 21.2; profiles/r05_gemm_v4_in_model.log).
  // ("gemm_v4" 2: lab, no such restriction)
  const int bm = v4.tile_rows;
  const bool uniform = uniform_tiles(p, bm) && (p2 == nullptr || uniform_tiles(*p2, bm));
  // (K < 2048: the image stream's fc1 of SD3 alone on this kernel measured +1.1 % per step on one box and -0.9 % on another: short reductions stay
  //  on gemm256v3.hip)
  if ((!uniform || p.K < 2048) && g_dk_v4_auto != 2) return false;
  const long tiles = (long)v4.tiles_a + v4.tiles_b;
  // (the rounds test in units of the device's CUs: the constants were fitted on 256 CUs -- a last round more than 56 % full, or 8 rounds and more)
  const long frac = tiles % n_cu;
  return tiles <= n_cu || tiles >= 8L * n_cu || frac == 0 || frac * 16 > 9L * n_cu;
}

// the grouped launch of an image + text pair (same N, K, epilogue), or PAIR: two launches
static int route_pair(const GemmParams& a, const GemmParams& b, int n_cu, GemmRoute& r) {
  r.kernel = GemmRoute::PAIR;
  const bool same = a.N == b.N && a.K == b.K && a.epi == b.epi && a.alpha == b.alpha && a.n_split == 0 && b.n_split == 0 && a.dtype == b.dtype;
  if (!((g_dk_gemm_mode == -1 || g_dk_gemm_mode == 10) && same && (a.M >= 1024 || b.M >= 1024) && (a.N % 256 == 0 || a.N >= 1024) &&
        dk_gemm256v3_eligible(a) && dk_gemm256v3_eligible(b)))
    return 0;
  // group only when the extra tiles do not open another wave of the CUs (kernel lab: a partial extra wave costs more
  // than the small separate launch) ...
  const long ta = (long)((a.M + 255) / 256) * ((a.N + 255) / 256), tb = (long)((b.M + 255) / 256) * ((b.N + 255) / 256);
  const long nc = n_cu;  // (rounds in units of THIS device's CUs; the fractions below were fitted on 256)
  // ... unless the kernel can cut that extra, small wave along K (remainder-wave split, needs the workspace)
  const bool split_ok = g_dk_v3_split != 0 && a.workspace != nullptr && (ta + tb) % nc <= nc / 4 && a.K / 64 >= (g_dk_pair_split_nk >= 0 ? g_dk_pair_split_nk : 24);
  const GemmRoute v3 = route_v3(a, &b, n_cu);
  // (gemm256v4.hip: the same test at ITS tile height -- with 224-row tiles the image + text fc1 of FLUX is 912 + 96 tiles: both 4 rounds)
  if (v4_ok(a) && v4_ok(b)) {
    const GemmRoute v4 = route_v4(a, &b, n_cu);
    const long ta4 = v4.tiles_a, tb4 = v4.tiles_b;
    if ((ta4 + nc - 1) / nc == (ta4 + tb4 + nc - 1) / nc && use_v4(a, &b, v3, v4)) {
      r = v4;
      return 0;
    }
  }
  if ((ta + nc - 1) / nc == (ta + tb + nc - 1) / nc || split_ok) {
    DK_REQUIRE(!a.conv && !b.conv, "gemm256v3: no grouped convolutions");
    r = v3;
  }
  return 0;
}

int dk_gemm_route(const GemmParams& p, const GemmParams* p2, int n_cu, GemmRoute& r) {
  if (p2 != nullptr) return route_pair(p, *p2, n_cu, r);
  DK_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0, "empty GEMM");
  DK_REQUIRE(p.dtype == DK_DTYPE_BF16 || p.dtype == DK_DTYPE_F16, "element type: 0 bf16, 1 fp16");
  DK_REQUIRE(p.ldw >= p.K && p.ldw % 8 == 0, "ldw must be >= K and a multiple of 8 elements");
  // the 256^2 kernel (16x16x32 MFMA, LDS-DMA ring, any M and any row-segment map) takes every large-M shape it accepts; small M
  // (modulation tables, embedders, a lone text stream) and N % 256 != 0 stay on the 128^2 tiles
  // (mode 10 forces gemm256v4.hip on what IT accepts and leaves every other launch to the automatic choice: usable around a whole model)
  // (N % 256 == 128 -- the half column tile -- only where the wasted half tile is a small fraction: SD3.5-large's N = 2432 / 7296; a small
  //  N such as the VAE's 128-channel shortcut Linear stays on the 128^2 tiles: ADVICE r4)
  const bool half_ok = p.N % 256 == 0 || p.N >= 1024 || g_dk_gemm_mode == 9;
  const bool big = !p.conv && g_dk_gemm_mode != 128 && half_ok && dk_gemm256v3_eligible(p) &&
                   (p.M >= 1024 || g_dk_gemm_mode == 9 || (g_dk_gemm_mode == 10 && v4_ok(p)));
  if (g_dk_gemm_mode == 9 && !p.conv) DK_REQUIRE(big, "gemm256v3 forced but the shape does not allow it");
  if (big) {
    r = route_v3(p, nullptr, n_cu);
    if (v4_ok(p)) {
      const GemmRoute v4 = route_v4(p, nullptr, n_cu);
      if (use_v4(p, nullptr, r, v4)) r = v4;
    }
    return 0;
  }
  // the fused key QKNorm + RoPE lives in the 256^2 kernel's tail: any other route runs the projection plain and the
  // stand-alone pass over its key columns afterwards
  if (p.kn_w != nullptr) {
    r.kernel = GemmRoute::KNORM;
    return 0;
  }
  if (p.n_split > 0) {
    // column-split GEMM on the kernel without split support: two GEMMs over the two column ranges
    DK_REQUIRE(p.n_split < p.N && p.C2 != nullptr, "bad column split");
    r.kernel = GemmRoute::COLUMNS;
    return 0;
  }
  if (p.conv && g_dk_gemm_mode != 128 && dk_gemm256v3_eligible(p)) {
    // implicit-GEMM convolutions with O % 256 == 0 ride the 256^2 kernel once their tiles fill most of the CUs (the VAE's 256^2-pixel
    // and larger stages); the 128^2-tile kernel below keeps the small stages and O = 128
    const long t256 = (long)((p.M + 255) / 256) * ((p.N + 255) / 256);
    // (with the K-split workspace a stage of about half the CUs' worth of tiles goes there too: its tiles are cut in two along K)
    if (g_dk_gemm_mode == 9 || t256 >= 192 || (p.workspace != nullptr && t256 >= 96 && t256 <= 128)) {
      r = route_v3(p, nullptr, n_cu);
      return 0;
    }
  }
  DK_REQUIRE(p.K % BK == 0, "K must be a multiple of 64");
  DK_REQUIRE(p.ldc % 4 == 0, "ldc must be a multiple of 4 elements");
  DK_REQUIRE(p.conv || (p.lda % 8 == 0), "lda must be a multiple of 8 elements");
  if (p.conv) {
    DK_REQUIRE(p.cC % BK == 0 && p.K == 9 * p.cC, "conv: C must be a multiple of 64 and K = 9*C");
    DK_REQUIRE(p.M == p.cB * p.cH * p.cW, "conv: M must equal B*H*W");
    DK_REQUIRE(p.zeros != nullptr, "conv: zero page missing");
  }
  if (p.epi == DK_EPI_GATE_RES) DK_REQUIRE(p.gate && p.res, "gate/res missing");
  if (p.epi == DK_EPI_RES) DK_REQUIRE(p.res, "res missing");
  r = tile_route(128, BM, BN, p, nullptr, n_cu);
  return 0;
}

#endif  // !DK_ELEM_F16

// the 128^2-tile kernel in this unit's element type (Linears and the conv form)
int dk_launch_gemm128(const GemmParams& p, const GemmRoute& r, hipStream_t stream) {
#ifndef DK_ELEM_F16
  if (p.dtype == DK_DTYPE_F16) return dk_f16::dk_launch_gemm128(p, r, stream);
#endif
  static DkDeviceOnce attr_once;
  if (attr_once.first()) {
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_gemm_bf16_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * STAGE_BYTES));
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_gemm_bf16_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * STAGE_BYTES));
    attr_once.mark();
  }
  dim3 grid(r.tiles_a), block(256);
  dk_prof_begin(p.conv ? 1 : 0, 2.0 * (double)p.M * (double)p.N * (double)p.K, stream);
  if (p.conv)
    hipLaunchKernelGGL(dk_gemm_bf16_kernel<1>, grid, block, 2 * STAGE_BYTES, stream, p);
  else
    hipLaunchKernelGGL(dk_gemm_bf16_kernel<0>, grid, block, 2 * STAGE_BYTES, stream, p);
  dk_prof_end(stream);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}

#ifndef DK_ELEM_F16

// One call: its route, then the launch -- or the calls an expansion is made of.  With `rec` (dk_gemm_plan) every launch is recorded instead:
// `launches` counts them, the other fields describe the last GEMM launch.
static int gemm_call(const GemmParams& p_in, const GemmParams* p2_in, hipStream_t stream, dk_gemm_plan_t* rec) {
  GemmParams p = p_in, p2 = p2_in ? *p2_in : p_in;
  if (p.ldw <= 0) p.ldw = p.K;
  if (p2.ldw <= 0) p2.ldw = p2.K;
  const GemmParams* second = p2_in ? &p2 : nullptr;
  GemmRoute r;
  const int rc = dk_gemm_route(p, second, dk_device_cu_count(), r);
  if (rc) return rc;
  if (r.kernel == GemmRoute::PAIR) {
    const int rc1 = gemm_call(p, nullptr, stream, rec);
    return rc1 ? rc1 : gemm_call(p2, nullptr, stream, rec);
  }
  if (r.kernel == GemmRoute::COLUMNS) {
    GemmParams a = p, b = p;
    a.N = p.n_split; a.n_split = 0;
    b.N = p.N - p.n_split; b.n_split = 0; b.W = p.W + (size_t)p.n_split * p.ldw; b.bias = p.bias ? p.bias + p.n_split : nullptr;
    b.C = p.C2; b.ldc = p.ldc2; b.epi = p.epi2;
    const int rc1 = gemm_call(a, nullptr, stream, rec);
    return rc1 ? rc1 : gemm_call(b, nullptr, stream, rec);
  }
  if (r.kernel == GemmRoute::KNORM) {
    GemmParams plain = p;
    plain.kn_w = nullptr;
    plain.qn_w = nullptr;
    const int rc1 = gemm_call(plain, nullptr, stream, rec);
    if (rc1) return rc1;
    DK_REQUIRE(p.c_seg_len == p.kn_seg_len || p.c_seg_len >= p.M, "fused key QKNorm: the output's row segments must be the sequences");
    // (with the query side asked for as well -- qn_w -- the pass covers both column ranges: they hold the same number of heads)
    DK_REQUIRE(p.qn_w == nullptr || p.qn_col1 - p.qn_col0 == p.kn_col1 - p.kn_col0, "fused QKNorm: query and key ranges must hold the same heads");
    if (rec) {
      rec->launches += 1;  // (the stand-alone pass)
      return 0;
    }
    return (p.dtype == DK_DTYPE_F16 ? dk_f16::dk_launch_qk_norm_rope : dk_launch_qk_norm_rope)(p.C, p.ldc, p.qn_w ? p.qn_col0 : 0, p.kn_col0, p.M, (p.kn_col1 - p.kn_col0) / p.kn_D, p.kn_D, p.qn_w ? p.qn_w : p.kn_w, p.kn_w,
                                  p.kn_eps, p.kn_rope, p.kn_seg_len, p.c_seg_len == p.kn_seg_len ? p.c_seg_stride : p.kn_seg_len, p.kn_pos_off, 0,
                                  stream, p.qn_w ? 0 : 1);
  }
  if (rec) {
    rec->kernel = r.kernel; rec->tile_rows = r.tile_rows; rec->tiles = r.tiles_a + r.tiles_b;
    rec->workgroups = r.split.n_dp + r.split.n_rem * r.split.S; rec->split_tiles = r.split.n_rem; rec->k_pieces = r.split.S; rec->ks = r.split.ks;
    rec->n_cu = r.n_cu; rec->launches += 1;
    return 0;
  }
  if (r.kernel == 3) return dk_launch_gemm256v3(p, second, r, stream);
  if (r.kernel == 4) return dk_launch_gemm256v4(p, second, r, stream);
  return dk_launch_gemm128(p, r, stream);
}

int dk_launch_gemm(const GemmParams& p, hipStream_t stream) { return gemm_call(p, nullptr, stream, nullptr); }
int dk_launch_gemm_pair(const GemmParams& a, const GemmParams& b, hipStream_t stream) { return gemm_call(a, &b, stream, nullptr); }
int dk_gemm_plan_call(const GemmParams& p, const GemmParams* p2, dk_gemm_plan_t& rec) {
  rec = dk_gemm_plan_t{};
  return gemm_call(p, p2, nullptr, &rec);
}
#endif  // !DK_ELEM_F16
