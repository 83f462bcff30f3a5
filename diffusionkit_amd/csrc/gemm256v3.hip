// 256 x 256 x 64 bf16 MFMA GEMM, third generation: the second-generation kernel (gemm256sk.hip, tile-parallel
// form) with the K loop rebuilt on v_mfma_f32_16x16x32_bf16.  Same contract, same grouped (two-problem) launch and
// column split; nn.Linear call sites python/src/diffusionkit/mlx/mmdit.py:821-832 and the fused linear1 / linear2
// of the single-stream blocks (:693-751).
//
// Shapes: N % 128 == 0 and K % 64 == 0; M is free.  (N % 256 == 128 -- SD3.5-large's h = 38 * 64 = 2432, config.py:72-74: the last
// column tile is half a tile: its upper 128 weight rows are fetched as a second copy of the lower 128, so that every DMA piece stays
// inside W, and the two waves columns that own them skip the tail.)  Rows go through the segment maps per lane on the load side
// (clamped to the last row when M is ragged) and, in the tail, per tile when the tile lies inside one segment
// (the common case) or per row when it straddles a segment boundary or the end of M -- the text stream of the
// SD3 double blocks (B = 2 segments of 589 rows, mmdit.py:608-625) rides in the image stream's launch that way.
//
// Why: the chip is power-limited on real (random) bf16 data, and the 16x16x32 instruction does the same FLOPs
// for less power than 32x32x16 -- scripts/mfma_probe.hip measures 2.21-2.24 PFLOP/s against 1.90-1.93 PFLOP/s
// for the same operand fragments (both reach 2.49 PFLOP/s on zeros).
//
// K loop: 8 waves (2 x 4), wave tile 128 (m) x 64 (n); per K = 32 slice the wave needs 4 W fragments and
// 8 A fragments (ds_read_b128 each: row = base + (lane & 15), 16-byte chunk = 4 * kk + (lane >> 4)) for
// 32 MFMAs.  A K-tile is 4 steps of 16 MFMAs:  (kk0, m 0-63), (kk0, m 64-127), (kk1, m 0-63), (kk1, m 64-127),
// with two W register sets and two A register sets reloaded one step ahead (inline-asm ds_read_b128,
// hand-counted s_waitcnt lgkmcnt), the tile barrier between steps 2 and 3, and the 8 LDS-DMA instructions
// (buffer_load_dwordx4 ... lds: SGPR resource + 32-bit lane offset) of a K-tile spread over steps 3 and 0, one in
// front of every fourth MFMA, on opposite slots for the two wave groups of a SIMD.  The second wave of each SIMD issues
// its fragment reads in the middle of a step instead of in front of it (DK_ITER_SKEW), and the steady state carries no
// branches: the last two K-tiles, which issue less DMA, are peeled (DK_DRIVE).
//
// Tail: accumulators -> wave-private LDS image (fp32, XOR-swizzled) -> row-major read-back, 8 columns per lane, one
// 16-byte store per lane and row; bias / GELU (erfc polynomial) / SiLU / gate * x + residual on the way.
// Remainder waves can be cut along K (SplitArgs, dk_plan_split): finisher + producer pieces through fp32 slabs (dk_ksplit.h).
//
// Tile height: template parameter MF = 16-row fragments per wave along m, 8 (256-row tiles) or 7 (224-row tiles).  The hot
// shapes have M = 4352 / 4608 / 8192 rows and N / 256 = 12 .. 48 column tiles: with 256-row tiles the last round of the 256 CUs is
// 20 % empty (N = 3072: 204 tiles, one round), with 224-row tiles the same work is 240 / 252 tiles of 7/8 the size -- one round
// of 0.875 tile-times instead of 1.0.  The route (dk_gemm_route) takes the height that minimises rounds x height (dk_tune_set
// ("gemm_mf", 7 | 8) forces one).  The LDS image keeps its two 128-row A slots; a 224-row tile uses 112 rows of each.
//
// C / D layout of the swapped-operand MFMA (A-operand = W fragment, B-operand = activation fragment):
// lane holds output row m = mf*16 + (lane & 15), columns n = nf*16 + 4*(lane >> 4) + {0..3}.
#include <cstring>
#include <type_traits>

#include "dk_kernels.h"
#include "dk_gemm_tail.h"

#ifndef DK_V3_ABL
#define DK_V3_ABL 0  // lab only (scripts/build_lab.sh ABL=n), bit mask: 1 no DMA inside the K loop, 2 no fragment reads inside it, 4 no tile
                     // barrier, 8 producers do not store, 16 finishers neither wait nor read, 32 no C stores, 64 no tail (run-time false),
                     // 128 every K-tile's DMA re-reads K-tile 0 (same bytes into the LDS, all of them L2 hits)
#endif

// placement of the 4 DMA pieces inside a 16-MFMA step: in front of MFMA slots PH, PH + STR, ... (PH0 / PH1 for the
// two wave groups of a SIMD)
#ifndef DK_V3_PH0
#define DK_V3_PH0 0
#define DK_V3_PH1 2
#define DK_V3_STR 4
#endif
#ifndef DK_V3_NT_STORE
#define DK_V3_NT_STORE 0  // lab: C leaves through non-temporal stores
#endif
#ifndef DK_V3_SKEW
#define DK_V3_SKEW 1
#endif
#ifndef DK_V3_SKEW_R
#define DK_V3_SKEW_R 8  // MFMA slot of a step behind which the skewed wave group issues its fragment reads
#endif

#define T256 256
#define BK 64
#define HALF_BYTES (128 * BK * 2)
#define OP_BYTES (2 * HALF_BYTES)  // one operand of one K-tile: rows 0-127, rows 128-255
// LDS ring: two slots of the activation operand, THREE of the weight operand (all 160 KiB).  Weights stream from HBM (every
// block of the model has its own, 5-38 GB per step in total), activations come out of L2 / Infinity Cache: the four weight
// pieces of K-tile i+2 are issued in the first step of K-tile i, 1.75 K-tiles ahead of their first read (a 2-slot ring gave
// them 0.5-1.0), the activation pieces behind the tile barrier, 1.0 ahead; the in-order vmcnt lets the newest four -- the
// weight pieces -- stay in flight across the barrier.  Cold-weight launches: within 1-6 % of warm ones (2-slot ring: 10-24 %).
#define W_BASE (2 * OP_BYTES)
#define LDS_BYTES (5 * OP_BYTES)

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;
typedef __attribute__((address_space(3))) char lds_char;

// Remainder split (SplitPlan, dk_plan_split in gemm.hip): the tiles beyond the last full wave of the CUs -- n_rem < #CU of them --
// are cut along K into S pieces with the SAME cut points for every tile (so that the workgroups that run at the
// same time still walk K in step and share A / W panels in L2): piece 0 = [0, ks) is the tile's finisher, pieces
// 1 .. S-1 share [ks, nk) and are producers (partial tile -> slab, flag; dk_ksplit.h).  Block order = dispatch order:
// full tiles, then the n_rem finishers, then the producers; a finisher only waits at its very end, and at least
// #CU - n_rem CUs are never held by finishers, so producers always get to run.
struct SplitArgs {
  float* slabs;     // [n_rem * (S - 1)][256 * 256] fp32: raw accumulators (Linears) / row-major tile images (convolutions)
  unsigned* flags;  // [n_rem * (S - 1)], zero between launches (reset by the finisher)
  unsigned* error_word;
  int n_dp;         // full tiles (multiple of 8); 0 <= n_dp <= tiles
  int n_rem;        // split tiles = tiles - n_dp (0: no split)
  int S;            // pieces per split tile
  int ks;           // K-tiles of the finisher piece
};

// position of block `bid` inside the XCD-contiguous order of the `count` blocks that start at block `base`
// (hardware places block b on XCD b & 7): neighbouring positions share an XCD, hence an L2
__device__ __forceinline__ int xcd_contiguous(int bid, int base, int count) {
  const int x = bid & 7;
  int start = 0;
  for (int y = 0; y < x; ++y) {
    const int first = (y - base) & 7;  // offset of XCD y's first block inside the group
    start += first < count ? (count - first + 7) >> 3 : 0;
  }
  return start + ((bid - base) >> 3);
}

// CONV: the activation operand is the im2col view of an NHWC tensor (3x3, pad 1, stride 1, optionally over the nearest-x2
// upsampling of the stored tensor -- vae.py:20-25,73,79,134): GEMM row m = output pixel (b, y, x), K-tile = 64 channels of one
// tap.  Per DMA piece the lane offset is recomputed from the pixel and the tap (a dozen VALU instructions); padding taps take
// an offset beyond the buffer descriptor's range, for which the LDS-DMA writes zeros (scripts/oob_probe.hip).
template <int MF, bool CONV>
__global__ __launch_bounds__(512, 2) void dk_gemm256v3_kernel(GemmParams pa, GemmParams pb, int tiles_a, int tiles_b, SplitArgs sp) {
  static_assert(MF == 8 || MF == 7, "wave tile: 8 or 7 fragments of 16 rows");
  constexpr int BM = 32 * MF;     // tile rows (two wave rows)
  constexpr int HROWS = 16 * MF;  // rows of one wave row = rows used of a 128-row LDS slot
  constexpr int NHI = MF - 4;     // fragments of the second ("hi") m-group of a wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if ((unsigned)(size_t)(lds_char*)smem != 0u) __builtin_trap();  // the LDS image is addressed from 0
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int l15 = lane & 15, q = lane >> 4;

  const int nk_full = pa.K / BK;
  int tile;       // XCD-contiguous tile index: neighbouring tiles share an L2
  int k0 = 0, nk = nk_full;  // this workgroup's K-tile range [k0, k0 + nk)
  int piece = -1;            // -1 full tile, 0 finisher of a split tile, >= 1 producer
  int rt = 0;                // index of the split tile
  {
    const int bid = blockIdx.x;
    if (bid < sp.n_dp || sp.n_rem == 0) {
      tile = xcd_contiguous(bid, 0, sp.n_rem == 0 ? tiles_a + tiles_b : sp.n_dp);
    } else {
      const int j = bid - sp.n_dp;
      piece = j / sp.n_rem;
      const int base = sp.n_dp + piece * sp.n_rem;
      rt = xcd_contiguous(bid, base, sp.n_rem);
      tile = sp.n_dp + rt;
      if (piece == 0) {
        nk = sp.ks;
      } else {
        const int rest = nk_full - sp.ks, np = sp.S - 1;
        k0 = sp.ks + rest * (piece - 1) / np;
        nk = sp.ks + rest * piece / np - k0;
      }
    }
  }
  const bool second = tile >= tiles_a;
  // ONE scalar base into the kernel-argument segment for this tile's parameter block (round 4).  Written as `second ? pb : pa` the compiler
  // loads BOTH blocks and s_cselects field by field (36 selects and 30 SGPRs spilled to VGPR lanes in the prologue, 2039 v_readlane over the
  // tail's code paths); with a base pointer every field is one s_load at its use: 100-104 -> 82-104 SGPRs, no lane spills, +0.5 % in the model
  // (profiles/r04_gemm_kernarg_pointer.log).  Layout: by-value struct arguments sit back to back from offset 0 of the segment.
  static_assert(sizeof(GemmParams) % 8 == 0 && alignof(GemmParams) == 8, "pb follows pa without padding");
  typedef const __attribute__((address_space(4))) GemmParams karg_params_t;
  const __attribute__((address_space(4))) char* kbase = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
  karg_params_t& p = *(karg_params_t*)(kbase + (second ? sizeof(GemmParams) : 0));
  const int tl = second ? tile - tiles_a : tile;  // tile index inside its problem
  const int nbm = (p.M + BM - 1) / BM, nbn = (p.N + T256 - 1) / T256;

  // ---- lane-constant parts of the LDS fragment addresses: row l15 (+ 16 * fragment), chunk 4*kk + q ----
  unsigned offk[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) offk[kk] = (unsigned)(l15 * 128 + (((kk * 4 + q) ^ (l15 >> 1)) << 4));
  const unsigned sA = wm * HALF_BYTES;
  const unsigned sW = W_BASE + (wn >> 1) * HALF_BYTES + (wn & 1) * 64 * 128;

  const int srow = lane >> 3;
  const int GROUP = 4;
  const int tpg = GROUP * nbn;
  const int g = tl / tpg;
  const int first_m = g * GROUP;
  const int gsz = min(nbm - first_m, GROUP);
  const int tm = first_m + (tl % tpg) % gsz;
  const int tn = (tl % tpg) / gsz;
  const int m0 = tm * BM, n0 = tn * T256;

  // DMA sources: A rows through the segment map per lane (32-bit byte offsets from p.A; rows beyond M - 1 re-read
  // the last row, their results are never stored), W rows from a tile-uniform base + lane part
  unsigned la[2][2], lw[2];  // (CONV: la = the row's pixel, b << 24 | y << 12 | x)
  unsigned lch[2] = {0u, 0u};  // CONV: byte offset of the lane's 16-byte chunk inside a 128-byte K-tile row
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int chunk = (lane & 7) ^ (srow >> 1) ^ (4 * j);  // = (lane&7) ^ (((wave*16 + j*8 + srow) >> 1) & 7)
    lw[j] = ((unsigned)srow * (unsigned)p.ldw + chunk * 8) * 2u;
    lch[j] = (unsigned)chunk * 16u;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      // (MF = 7: wave 7's rows lie beyond the 112 rows a wave row uses -- it fetches duplicates of other rows into LDS rows
      //  nobody reads, so that every wave issues the same 8 pieces per K-tile)
      const int m = min(m0 + hh * HROWS + wave * 16 + j * 8 + srow, p.M - 1);
      if (CONV) {
        const int hw = p.cH * p.cW;
        const int b = m / hw, rem = m - b * hw;
        const int y = rem / p.cW, x = rem - y * p.cW;
        la[hh][j] = ((unsigned)b << 24) | ((unsigned)y << 12) | (unsigned)x;
      } else {
        la[hh][j] = (unsigned)m;  // (mapped through the row segments below)
      }
    }
  }
  if (!CONV) {
    // a tile inside one row segment (every tile of an image stream) maps its rows with one scalar division instead of four per lane
    // (round 5: the per-lane integer divisions were ~ 0.3 us in front of the first DMA piece of every tile)
    const int a_seg0 = m0 / p.a_seg_len;
    const bool a_uniform = min(m0 + BM - 1, p.M - 1) / p.a_seg_len == a_seg0;
    const int a_base = a_seg0 * p.a_seg_stride - a_seg0 * p.a_seg_len;
    if (a_uniform) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) la[hh][j] += (unsigned)a_base;
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) la[hh][j] = (unsigned)(((int)la[hh][j] / p.a_seg_len) * p.a_seg_stride + ((int)la[hh][j] % p.a_seg_len));
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) la[hh][j] = (la[hh][j] * (unsigned)p.lda + (lch[j] >> 1)) * 2u;
  }
  // CONV: tap (dy, dx in -1..1) and channel byte offset of the NEXT activation K-tile to be issued; stored tensor [cB, Hs, Ws, cC]
  const int cv_ush = CONV && p.ups == 1 ? 1 : 0;
  const int cv_Hs = p.cH >> cv_ush, cv_Ws = p.cW >> cv_ush;
  const int cv_C2 = p.cC * 2;
  int cv_dy = -1, cv_dx = -1, cv_cb = 0;
  if (CONV) {
    const int cpt = p.cC / BK;
    const int tap = k0 / cpt;
    cv_cb = (k0 - tap * cpt) * (BK * 2);
    cv_dy = tap / 3 - 1;
    cv_dx = tap - (tap / 3) * 3 - 1;
  }
  const char* gA = (const char*)p.A + (CONV ? (size_t)0 : (size_t)k0 * (BK * 2));
  const char* gW = (const char*)p.W + ((size_t)n0 + wave * 16) * (size_t)p.ldw * 2 + (size_t)k0 * (BK * 2);
  // (half a column tile at the end of N: rows 128-255 of the weight slot are a second copy of rows 0-127)
  const size_t w128 = n0 + T256 > p.N ? (size_t)0 : (size_t)128 * p.ldw * 2, w8 = (size_t)8 * p.ldw * 2;
  const bool col_ok = n0 + wn * 64 < p.N;  // wave-uniform: this wave's 64 columns exist

  // LDS-DMA in the buffer form: SGPR resource (base, 4 GiB range) + 32-bit lane offset + scalar offset -- no 64-bit
  // per-lane address and no VALU per piece
  const __amdgpu_buffer_rsrc_t rA =
      __builtin_amdgcn_make_buffer_rsrc((void*)gA, 0, CONV ? p.cB * cv_Hs * cv_Ws * cv_C2 : -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc((void*)gW, 0, -1, 0x00020000);
  // ring slots (byte offsets from W_BASE) of the weights of K-tiles i, i+1, i+2 of the loop below
  unsigned wo_cur = 0u, wo_nxt = OP_BYTES, wo_nn = 2u * OP_BYTES;
  // one of the 8 DMA instructions of K-tile i: gidx 0..3 the activation pieces (half, j), 4..7 the weight pieces into slot `wslot`
  auto issue_piece_to = [&](int i, int gidx, unsigned wslot) {
    const int hh = gidx & 1, j = (gidx >> 1) & 1;
    if (gidx < 4 && CONV) {
      const unsigned pc = la[hh][j];
      const int iy = (int)((pc >> 12) & 0xFFFu) + cv_dy, ix = (int)(pc & 0xFFFu) + cv_dx;
      const bool ok = (unsigned)iy < (unsigned)p.cH && (unsigned)ix < (unsigned)p.cW;
      const int spix = ((int)(pc >> 24) * cv_Hs + (iy >> cv_ush)) * cv_Ws + (ix >> cv_ush);
      const unsigned voff = ok ? (unsigned)spix * (unsigned)cv_C2 + lch[j] : 0x80000000u;  // padding tap: out of range -> zeros
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_ptr_t)((lds_char*)0 + (i & 1) * OP_BYTES + (wave * 16) * 128 + hh * HALF_BYTES + j * 1024),
                                               16, (int)voff, cv_cb, 0, 0);
    } else if (gidx < 4)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_ptr_t)((lds_char*)0 + (i & 1) * OP_BYTES + (wave * 16) * 128 + hh * HALF_BYTES + j * 1024),
                                               16, (int)la[hh][j], ((DK_V3_ABL & 128) ? 0 : i) * (BK * 2), 0, 0);
    else
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (lds_ptr_t)((lds_char*)0 + W_BASE + wslot + (wave * 16) * 128 + hh * HALF_BYTES + j * 1024),
                                               16, (int)lw[j], (int)(hh * w128 + j * w8) + ((DK_V3_ABL & 128) ? 0 : i) * (BK * 2), 0, 0);
  };
  auto issue_piece = [&](int i, int gidx) { issue_piece_to(i, gidx, wo_nn); };  // the loop only ever issues K-tile i+2
  auto conv_advance = [&]() {  // CONV: the activation pieces of one K-tile are out -- on to the next 64 channels / the next tap
    if (CONV) {
      cv_cb += BK * 2;
      if (cv_cb == cv_C2) {
        cv_cb = 0;
        if (++cv_dx == 2) cv_dx = -1, ++cv_dy;
      }
    }
  };

  f32x4 acc[4][MF];  // [nf][mf]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < MF; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

  // ---------------- K loop: register-pipelined, hand-counted LDS waits ----------------
#define DK_LDS_RD(DST, ADDR, OFF)                                                              \
  do {                                                                                        \
    if (!(DK_V3_ABL & 2) || !in_loop) asm volatile("ds_read_b128 %0, %1 offset:" #OFF : "=v"(DST) : "v"(ADDR)); \
  } while (0)
#define DK_RDW(SET, BUFOFF, KK)                    \
  do {                                             \
    const unsigned aW_ = offk[KK] + sW + (BUFOFF); \
    DK_LDS_RD(wf##SET[0], aW_, 0);                 \
    DK_LDS_RD(wf##SET[1], aW_, 2048);              \
    DK_LDS_RD(wf##SET[2], aW_, 4096);              \
    DK_LDS_RD(wf##SET[3], aW_, 6144);              \
  } while (0)
#define DK_RDA_LO(SET, BUFOFF, KK)                 \
  do {                                             \
    const unsigned aA_ = offk[KK] + sA + (BUFOFF); \
    DK_LDS_RD(xf##SET[0], aA_, 0);                 \
    DK_LDS_RD(xf##SET[1], aA_, 2048);              \
    DK_LDS_RD(xf##SET[2], aA_, 4096);              \
    DK_LDS_RD(xf##SET[3], aA_, 6144);              \
  } while (0)
#define DK_RDA_HI(SET, BUFOFF, KK)                 \
  do {                                             \
    const unsigned aA_ = offk[KK] + sA + (BUFOFF); \
    DK_LDS_RD(xf##SET[0], aA_, 8192);              \
    DK_LDS_RD(xf##SET[1], aA_, 10240);             \
    DK_LDS_RD(xf##SET[2], aA_, 12288);             \
    if (NHI > 3) DK_LDS_RD(xf##SET[3], aA_, 14336); \
  } while (0)
// the wait in front of the tile barrier: own fragment reads and own DMA pieces of the next K-tile; the four weight pieces of
// K-tile i+2 (issued last) stay in flight when there are any (KEEP)
#define DK_TILE_WAIT(V, KEEP)                                                                                            \
  do {                                                                                                                   \
    if (KEEP)                                                                                                            \
      asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" : "+v"(V[0]), "+v"(V[1]), "+v"(V[2]), "+v"(V[3])::"memory");          \
    else                                                                                                                 \
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(V[0]), "+v"(V[1]), "+v"(V[2]), "+v"(V[3])::"memory");          \
  } while (0)
#define DK_WAIT4(N, V) asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(V[0]), "+v"(V[1]), "+v"(V[2]), "+v"(V[3]))
// everything but the NHI hi-fragment reads issued last has landed
#define DK_WAIT8_HI(V, U)                        \
  do {                                           \
    if constexpr (NHI == 4) DK_WAIT8(4, V, U);   \
    else DK_WAIT8(3, V, U);                      \
  } while (0)
#define DK_WAIT8(N, V, U)                  \
  asm volatile("s_waitcnt lgkmcnt(" #N ")" \
               : "+v"(V[0]), "+v"(V[1]), "+v"(V[2]), "+v"(V[3]), "+v"(U[0]), "+v"(U[1]), "+v"(U[2]), "+v"(U[3]))
// 16 MFMAs acc[nf][MB + mf] += W[nf] . A[mf], with NG DMA pieces (TILE, G0 ..) in front of slots PH, PH+4, ... when ON
// (NM = m-fragments of the group: 4, or NHI for the hi group; a step is 4 * NM MFMAs, MFMA e_ = (nf = e_ / NM, mf = e_ % NM); the
//  pieces sit NM slots apart so that four of them fit any step)
#define DK_MMG(WSET, ASET, MB, NM, TILE, G0, NG, PH, ON) DK_MMGR(WSET, ASET, MB, NM, TILE, G0, NG, PH, ON, 0, 4 * (NM))
#define DK_MMGR(WSET, ASET, MB, NM, TILE, G0, NG, PH, ON, E0, E1)                                                 \
  do {                                                                                                            \
    _Pragma("unroll") for (int e_ = (E0); e_ < (E1); ++e_) {                                                           \
      if (!(DK_V3_ABL & 1) && (NG) > 0 && (ON) && e_ >= (PH) && ((e_ - (PH)) % (NM)) == 0 && ((e_ - (PH)) / (NM)) < (NG)) \
        issue_piece((TILE), (G0) + ((e_ - (PH)) / (NM)));                                                         \
      acc[e_ / (NM)][(MB) + (e_ % (NM))] = mfma_16x16x32(wf##WSET[e_ / (NM)], xf##ASET[e_ % (NM)], \
                                                                                   acc[e_ / (NM)][(MB) + (e_ % (NM))]);          \
      __builtin_amdgcn_sched_barrier(0);                                                                          \
    }                                                                                                             \
  } while (0)
// One K-tile for the wave group that reads its fragments in FRONT of every 16-MFMA step.  ON2 (compile-time): whether the
// DMA pieces of K-tile i+2 are issued (weights in the first step, activations behind the barrier -- in that program order,
// see DK_TILE_WAIT) -- false only in the last two K-tiles, so that the steady-state loop carries no branches around the pieces.
#define DK_ITER(PH, ON1, ON2)                                                                                    \
  {                                                                                                              \
    constexpr bool in_loop = true;                                                                               \
    const unsigned bo = (i & 1) * OP_BYTES;                                                                      \
    DK_RDA_HI(1, bo, 0);                                                                                         \
    DK_WAIT8_HI(wf0, xf0);                                                                                       \
    DK_MMG(0, 0, 0, 4, i + 2, 4, 4, PH, ON2);                                                                    \
    DK_RDW(1, wo_cur, 1);                                                                                        \
    DK_RDA_LO(0, bo, 1);                                                                                         \
    DK_WAIT4(8, xf1);                                                                                            \
    DK_MMG(0, 1, 4, NHI, i + 2, 0, 0, PH, false);                                                                \
    DK_RDA_HI(1, bo, 1);                                                                                         \
    DK_WAIT8_HI(wf1, xf0);                                                                                       \
    DK_MMG(1, 0, 0, 4, i + 2, 0, 0, PH, false);                                                                  \
    DK_TILE_WAIT(xf1, ON2);                                                                                      \
    if (!(DK_V3_ABL & 4)) __builtin_amdgcn_s_barrier();                                                          \
    asm volatile("" ::: "memory");                                                                               \
    DK_RDW(0, wo_nxt, 0); /* unconditional: after the last tile these read stale ring data that */               \
    DK_RDA_LO(0, bo ^ OP_BYTES, 0); /* nobody uses; they are waited for behind the loop          */               \
    DK_MMG(1, 1, 4, NHI, i + 2, 0, 4, PH, ON2);                                                                  \
    DK_ROTATE_W();                                                                                               \
  }
// The same K-tile for the second wave of each SIMD with its fragment reads behind MFMA slot R of every step instead of
// in front of it, so that the two waves of a SIMD do not run their read / wait sections at the same time (+1.5-2 %).
#define DK_ITER_SKEW(PH, R, ON1, ON2)                                                                            \
  {                                                                                                              \
    constexpr bool in_loop = true;                                                                               \
    const unsigned bo = (i & 1) * OP_BYTES;                                                                      \
    constexpr int RH = (R) * NHI / 4; /* the same relative slot inside a hi step of 4 * NHI MFMAs */            \
    DK_WAIT8(0, wf0, xf0);                                                                                       \
    DK_MMGR(0, 0, 0, 4, i + 2, 4, 4, PH, ON2, 0, R);                                                             \
    DK_RDA_HI(1, bo, 0);                                                                                         \
    DK_MMGR(0, 0, 0, 4, i + 2, 4, 4, PH, ON2, R, 16);                                                            \
    DK_WAIT4(0, xf1);                                                                                            \
    DK_MMGR(0, 1, 4, NHI, i + 2, 0, 0, 0, false, 0, RH);                                                         \
    DK_RDW(1, wo_cur, 1);                                                                                        \
    DK_RDA_LO(0, bo, 1);                                                                                         \
    DK_MMGR(0, 1, 4, NHI, i + 2, 0, 0, 0, false, RH, 4 * NHI);                                                   \
    DK_WAIT8(0, wf1, xf0);                                                                                       \
    DK_MMGR(1, 0, 0, 4, i + 2, 0, 0, 0, false, 0, R);                                                            \
    DK_RDA_HI(1, bo, 1);                                                                                         \
    DK_MMGR(1, 0, 0, 4, i + 2, 0, 0, 0, false, R, 16);                                                           \
    DK_TILE_WAIT(xf1, ON2);                                                                                      \
    if (!(DK_V3_ABL & 4)) __builtin_amdgcn_s_barrier();                                                          \
    asm volatile("" ::: "memory");                                                                               \
    DK_MMGR(1, 1, 4, NHI, i + 2, 0, 4, PH, ON2, 0, RH);                                                          \
    DK_RDW(0, wo_nxt, 0);                                                                                        \
    DK_RDA_LO(0, bo ^ OP_BYTES, 0);                                                                              \
    DK_MMGR(1, 1, 4, NHI, i + 2, 0, 4, PH, ON2, RH, 4 * NHI);                                                    \
    DK_ROTATE_W();                                                                                               \
  }
// all K-tiles of this workgroup: branch-free steady state, then the two tiles that issue less.  The fragments in flight
// at a section boundary are waited for there (an inline-asm load must not be in flight across a compiler-visible merge).
#define DK_ROTATE_W()           \
  do {                          \
    const unsigned t_ = wo_cur; \
    wo_cur = wo_nxt;            \
    wo_nxt = wo_nn;             \
    wo_nn = t_;                 \
    conv_advance();             \
  } while (0)
#define DK_DRIVE(ITER, ...)                                                                                      \
  {                                                                                                              \
    int i = 0;                                                                                                   \
    for (; i + 2 < nk; ++i) ITER(__VA_ARGS__, true, true)                                                        \
    DK_WAIT8(0, wf0, xf0);                                                                                       \
    if (i + 1 < nk) {                                                                                            \
      ITER(__VA_ARGS__, true, false)                                                                             \
      ++i;                                                                                                       \
      DK_WAIT8(0, wf0, xf0);                                                                                     \
    }                                                                                                            \
    ITER(__VA_ARGS__, false, false)                                                                              \
    DK_WAIT8(0, wf0, xf0);                                                                                       \
  }

  {
    ex8 wf0[4], wf1[4], xf0[4], xf1[4];
    // prologue: K-tile 0, then K-tile 1 (the loop's first wait lets only its own four weight pieces, of K-tile 2, stay in flight)
#pragma unroll
    for (int gidx = 0; gidx < 8; ++gidx) issue_piece_to(0, gidx, wo_cur);
    conv_advance();
    if (nk > 1) {
#pragma unroll
      for (int gidx = 0; gidx < 8; ++gidx) issue_piece_to(1, gidx, wo_nxt);
      conv_advance();
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // (the first fragment reads sit INSIDE the branches: an inline-asm load that is still in flight must not be
    //  live across a compiler-visible branch, see gemm256sk.hip)
    constexpr bool in_loop = false;
    if (wm == 0) {
      DK_RDW(0, wo_cur, 0);
      DK_RDA_LO(0, 0u, 0);
      DK_DRIVE(DK_ITER, DK_V3_PH0)
    } else {
      DK_RDW(0, wo_cur, 0);
      DK_RDA_LO(0, 0u, 0);
#if DK_V3_SKEW
      DK_DRIVE(DK_ITER_SKEW, DK_V3_PH1, DK_V3_SKEW_R)
#else
      DK_DRIVE(DK_ITER, DK_V3_PH1)
#endif
    }
  }
#undef DK_LDS_RD
#undef DK_RDW
#undef DK_RDA_LO
#undef DK_RDA_HI
#undef DK_WAIT4
#undef DK_TILE_WAIT
#undef DK_WAIT8
#undef DK_WAIT8_HI
#undef DK_MMG
#undef DK_MMGR
#undef DK_ITER
#undef DK_ITER_SKEW
#undef DK_DRIVE
#undef DK_ROTATE_W

  // ---------------- K split, round 6: the pieces of a cut tile exchange their RAW accumulators (registers -> slab -> registers) ----------------
  // Until round 6 a cut tile went through a second tail: fp32 staging images (two passes over the LDS), row-major fp32 slabs written from the read-back,
  // the finisher adding them row by row inside its epilogue loop.  The accumulators are in registers on both sides: a producer now stores them as they are
  // (thread-linear: one coalesced 16-byte write-through store per thread and accumulator quad), the finisher adds them in front of the ordinary
  // whole-tile tail (bias before staging, bf16 image, one LDS round trip) -- gemm256f8.hip's exchange, which was written first.  Same hand-off protocol
  // (guide G16): write-through stores, vmcnt(0) in every wave, barrier, one relaxed agent-scope flag store; finisher: relaxed poll, one agent-scope
  // acquire, barrier, plain loads.  Summation order of a cut tile: finisher's K range first, then the producers' in piece order (as before).
  // (Linears only: the conv form of the 256-row kernel sits at exactly 256 registers and keeps the fp32-image path below -- this block cost it 7 spills)
  if (!CONV && piece >= 0) {
    const int n_prod_x = sp.S - 1;
    // (thread index from a FRESH lane id + the scalar wave id: a value carried across the K loop costs a register there -- the conv form of the
    //  256-row kernel has none to spare)
    int lane_x;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_x));
    const unsigned toff = (unsigned)(wave * 64 + lane_x) * 4u;  // floats
    auto leader = [wave, lane_x] { return wave == 0 && lane_x == 0; };
    if (piece >= 1) {
      dk_ksplit_store_acc<MF>(sp.slabs + (size_t)(rt * n_prod_x + piece - 1) * DK_KSPLIT_SLAB_FLOATS, toff, acc);  // (uniform base: scalar registers)
      dk_ksplit_publish(sp.flags, rt, n_prod_x, piece, leader);
      return;
    }
    dk_ksplit_wait(sp.flags, rt, n_prod_x, sp.error_word, leader);
    for (int pp = 0; pp < n_prod_x; ++pp) {
      const float* const slab = sp.slabs + (size_t)(rt * n_prod_x + pp) * DK_KSPLIT_SLAB_FLOATS;
#pragma unroll
      for (int nf = 0; nf < 4; ++nf)
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
          const f32x4 o = *(const f32x4*)(slab + (size_t)(nf * 8 + mf) * 2048 + toff);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[nf][mf][e] += o[e];
        }
    }
    dk_ksplit_release(sp.flags, rt, n_prod_x, leader);
    piece = -1;  // from here on the finisher is a whole tile
  }
  if (!CONV) __builtin_assume(piece < 0);  // (no Linear tile reaches the fp32-image tail path below any more; convolutions still do)

  // ---------------- tail: accumulators -> LDS (wave-private image) -> row-major (dk_gemm_tail.h) ----------------
  // All waves passed the last loop barrier after their final ds_read, so the ring is free.
  // whole tiles: the bias of this lane's 16 columns (4 per 16-column fragment), all loads up front -- one latency, not one per pass,
  // and in front of the tile set-up, whose chain of scalar loads and divisions covers it
  u32x2 bias_q[4] = {u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}};
  if (piece < 0 && p.bias && col_ok) {
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) bias_q[nf] = *(const u32x2*)(p.bias + n0 + wn * 64 + nf * 16 + 4 * q);
  }
  DkTailTile t = dk_tail_tile<false>(p, m0, n0, BM, wm * HROWS, p.M, p.ldc, p.c_seg_len, p.ldr);
  dk_tail_first_rows<-1>(p, t);
  t.kfuse = !CONV && piece < 0 && t.kfuse;  // (a whole Linear tile)
  const int rrow = lane >> 2, rc2 = (lane & 3) * 2;  // read-back: this lane's row of a 16-row step and its first 16-byte chunk of an fp32 image row

  // split tile (convolutions): a producer stores its fp32 partial tile image to its slab; the finisher first waits for every producer of
  // the tile (dk_ksplit.h)
  const int n_prod = sp.S - 1;
  float* const my_slab = piece >= 1 ? sp.slabs + (size_t)(rt * n_prod + piece - 1) * DK_KSPLIT_SLAB_FLOATS : nullptr;
  auto leader = [&] { return tid == 0; };
  if (piece == 0 && !(DK_V3_ABL & 16)) dk_ksplit_wait(sp.flags, rt, n_prod, sp.error_word, leader);

  // Key tile of a q / k / v projection with the fused QKNorm + RoPE: the sum of squares of every row over its head's columns, from the
  // accumulators
  if (t.kfuse) dk_tail_sumsq_exchange<MF>(acc, bias_q, [&](int, int) { return p.alpha; }, wave, l15, q);
  // how a finished row leaves
  auto store_raw = [&](size_t crow, int ocol, bool ok, u32x4 sv) {
    // (lab: 32 = the C stores sit behind a condition that is false at run time -- the work stays, the traffic goes)
    if (((DK_V3_ABL & 32) ? p.alpha == -1234.5f : true) && ok) *(u32x4*)(t.Cb + crow * (size_t)t.ldcb + ocol) = sv;
  };
  auto store = [&](int, size_t crow, int ocol, bool ok, const float* vv) {
    const uint4 o4 = dk_tail_pack8(vv);
    const u32x4 ov = {o4.x, o4.y, o4.z, o4.w};
#if DK_V3_NT_STORE
    if (((DK_V3_ABL & 32) ? p.alpha == -1234.5f : true) && ok) __builtin_nontemporal_store(ov, (u32x4*)(t.Cb + crow * (size_t)t.ldcb + ocol));
#else
    store_raw(crow, ocol, ok, ov);
#endif
  };
  // the two 32-column halves of the wave tile (compile-time index: the accumulators must stay in registers)
  // (STAGE / EMIT: a whole tile stages BOTH halves -- two 8 KiB bf16 images per wave -- before it reads the first one back: one
  //  LDS round trip of latency per tile instead of two; a split tile's 16 KiB fp32 image holds one half at a time)
  auto tail_pass = [&](auto ni_c, auto stage_c, auto emit_c) {
    constexpr int ni = decltype(ni_c)::value;
    constexpr bool STAGE = decltype(stage_c)::value, EMIT = decltype(emit_c)::value;
    const unsigned reg0 = (unsigned)wave * 16384u + ((STAGE && EMIT) ? 0u : (unsigned)ni * 8192u);  // this pass's image
    // stage: lane owns row mf*16 + l15, columns (nf & 1)*16 + 4*q + {0..3} of this 32-column half.  A whole tile (no K split)
    // stages round_act(alpha * acc + bias) -- what every epilogue starts from -- as bf16: half the LDS bytes of the fp32 image;
    // split tiles stage the fp32 partial sums (128-byte rows, 16-byte chunk c at position c ^ ((row >> 1) & 7))
    const bool bf_stage = piece < 0;
    if (!STAGE) {
    } else if (bf_stage) {
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) {
        float b4[4];
        unpack2(bias_q[ni * 2 + nf][0], b4[0], b4[1]);
        unpack2(bias_q[ni * 2 + nf][1], b4[2], b4[3]);
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
          const f32x4 a = acc[ni * 2 + nf][mf];
          uint2 w;
          w.x = pack2(a[0] * p.alpha + b4[0], a[1] * p.alpha + b4[1]);
          w.y = pack2(a[2] * p.alpha + b4[2], a[3] * p.alpha + b4[3]);
          *(__attribute__((address_space(3))) u32x2*)((lds_char*)0 + reg0 + dk_tail_stage_off(mf * 16 + l15, nf, q)) = u32x2{w.x, w.y};
        }
      }
    } else {
#pragma unroll
      for (int nf = 0; nf < 2; ++nf)
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
          const int row = mf * 16 + l15;
          *(__attribute__((address_space(3))) f32x4*)((lds_char*)0 + reg0 + row * 128 + (((nf * 4 + q) ^ ((row >> 1) & 7)) << 4)) = acc[ni * 2 + nf][mf];
        }
    }
    // (same wave writes and reads the image: program order + the compiler's lgkmcnt suffice)
    if (!EMIT || !col_ok) return;
    const int coff = wn * 64 + ni * 32;  // first of this pass's 32 columns inside the tile
    // whole tile: the shared row loop, one pass per call.  It is instantiated per form -- tile-uniform maps (FAST) or a per-lane walk through
    // the maps -- so that the common case keeps its short body (one v_add per address, batched loads)
    auto rows = [&](auto fast_c, auto ek_c, auto kf_c) {
      dk_tail_rows<decltype(fast_c)::value, decltype(ek_c)::value, decltype(kf_c)::value, MF, false, 1, true>(
          p, t, lane, [&](int) { return DkTailPass{reg0, coff}; }, [&](int, int, int row) { return dk_tail_sumsq_read(wave, row, p.kn_D); }, store, store_raw);
    };
    // split tile (convolutions): the fp32 image keeps a row loop of its own on the shared per-row pieces -- a producer stores its rows to its
    // slab and is done; the finisher adds the slabs, and the bias goes in after the sum (run-time epilogue, no fused norm)
    auto split_rows = [&](auto fast_c) {
      constexpr bool FAST = decltype(fast_c)::value;
      const int col = t.n0 + coff + rc2 * 4, ocol = t.ncol0 + coff + rc2 * 4;
      const bool gated = t.epi == DK_EPI_GATE_RES;
      float bias8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gate8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (p.bias && piece == 0) dk_tail_unpack8(*(const uint4*)(p.bias + col), bias8);
      if (FAST && gated) dk_tail_unpack8(*(const uint4*)(t.gate_row + col), gate8);
      DkTailWalk w;
      if (!FAST) w.start(p, p.c_seg_len, t.mrow0 + rrow, t.has_res, gated);
#pragma unroll
      for (int itr = 0; itr < MF; ++itr) {
        const int row = itr * 16 + rrow;  // row inside the wave's block of HROWS rows
        size_t crow = t.physC0 + row, rrow_phys = t.physR0 + row;
        bool valid = true;
        if (!FAST) {
          valid = t.mrow0 + row < p.M;
          crow = w.crow(p);
          rrow_phys = w.rrow(p);
          if (gated && valid) dk_tail_unpack8(*(const uint4*)(w.gate(p) + col), gate8);
          w.step(p, p.c_seg_len, t.has_res, gated);
        }
        const unsigned sw = (unsigned)((row >> 1) & 7);
        f32x4 a0 = *(const __attribute__((address_space(3))) f32x4*)((lds_char*)0 + reg0 + row * 128 + (((unsigned)rc2 ^ sw) << 4));
        f32x4 a1 = *(const __attribute__((address_space(3))) f32x4*)((lds_char*)0 + reg0 + row * 128 + (((unsigned)(rc2 + 1) ^ sw) << 4));
        const size_t slab_idx = (size_t)(wm * HROWS + row) * 256 + coff + rc2 * 4;
        if (piece >= 1) {
          if (!(DK_V3_ABL & 8)) {  // (lab: 8 = producers do not store)
            dk_ksplit_store_b128(my_slab + slab_idx, a0);
            dk_ksplit_store_b128(my_slab + slab_idx + 4, a1);
          }
          continue;
        }
        for (int pp = 0; pp < ((DK_V3_ABL & 16) ? 0 : n_prod); ++pp) {  // (lab: 16 = finishers neither wait nor read)
          const float* sl = sp.slabs + (size_t)(rt * n_prod + pp) * DK_KSPLIT_SLAB_FLOATS + slab_idx;
          const f32x4 o0 = *(const f32x4*)sl, o1 = *(const f32x4*)(sl + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) a0[e] += o0[e], a1[e] += o1[e];
        }
        float vv[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          vv[e] = round_act(a0[e] * p.alpha + bias8[e]);
          vv[4 + e] = round_act(a1[e] * p.alpha + bias8[4 + e]);
        }
        auto res = [&] { return (FAST || valid) ? *(const uint4*)(p.res + rrow_phys * (size_t)p.ldr + col) : make_uint4(0u, 0u, 0u, 0u); };
        dk_tail_epilogue8(vv, t.epi, t.has_res, res, gate8);
        store(itr, crow, ocol, FAST || valid, vv);
      }
    };
    using EkRun = std::integral_constant<int, -1>;
    using No = std::false_type;
    using Yes = std::true_type;
    const int epi = t.epi;
    if (t.kfuse) {  // (whole tile, bias-only epilogue -- checked by the launcher)
      if (t.fast)
        rows(Yes{}, std::integral_constant<int, DK_EPI_BIAS>{}, Yes{});
      else
        rows(No{}, std::integral_constant<int, DK_EPI_BIAS>{}, Yes{});
    } else if (bf_stage && t.fast) {
      // the common epilogues with the epilogue folded at compile time (no scalar branches inside the row loop)
      if (epi == DK_EPI_BIAS)
        rows(Yes{}, std::integral_constant<int, DK_EPI_BIAS>{}, No{});
      else if (epi == DK_EPI_BIAS_GELU)
        rows(Yes{}, std::integral_constant<int, DK_EPI_BIAS_GELU>{}, No{});
      else if (epi == DK_EPI_GATE_RES)
        rows(Yes{}, std::integral_constant<int, DK_EPI_GATE_RES>{}, No{});
      else if (epi == DK_EPI_RES)
        rows(Yes{}, std::integral_constant<int, DK_EPI_RES>{}, No{});
      else
        rows(Yes{}, EkRun{}, No{});
    } else if (bf_stage) {
      rows(No{}, EkRun{}, No{});
    } else if (t.fast) {
      split_rows(Yes{});
    } else {
      split_rows(No{});
    }
  };
  if (!((DK_V3_ABL & 64) && p.alpha != -1234.5f)) {  // (lab: 64 = no tail at run time)
    if (piece < 0) {
      tail_pass(std::integral_constant<int, 0>{}, std::true_type{}, std::false_type{});
      tail_pass(std::integral_constant<int, 1>{}, std::true_type{}, std::false_type{});
      tail_pass(std::integral_constant<int, 0>{}, std::false_type{}, std::true_type{});
      tail_pass(std::integral_constant<int, 1>{}, std::false_type{}, std::true_type{});
    } else {
      tail_pass(std::integral_constant<int, 0>{}, std::true_type{}, std::true_type{});
      tail_pass(std::integral_constant<int, 1>{}, std::true_type{}, std::true_type{});
    }
  }
  if (piece >= 1)
    dk_ksplit_publish(sp.flags, rt, n_prod, piece, leader);
  else if (piece == 0)
    dk_ksplit_release(sp.flags, rt, n_prod, leader);
}

#ifndef DK_ELEM_F16  // (one copy: gemm256v3_f16.hip compiles this file a second time inside namespace dk_f16 for the kernel and its launcher)
bool dk_gemm256v3_eligible(const GemmParams& p) {
  if (p.M <= 0 || p.N % 128 != 0 || p.K % BK != 0 || (!p.conv && p.lda % 8 != 0) || p.ldw % 8 != 0 || p.ldc % 8 != 0) return false;
  if (p.conv) {  // 3x3 / pad 1 / stride 1 (optionally over the nearest-x2 view); pixel packed as b:8 | y:12 | x:12, 31-bit byte offsets
    if (p.N % 256 != 0) return false;  // (a half column tile would waste half the MFMAs of a 128-channel stage: the 128^2 kernel's)
    if (p.ups < 0 || p.ups > 1 || p.cC % BK != 0 || p.K != 9 * p.cC || p.M != p.cB * p.cH * p.cW || p.n_split != 0) return false;
    if (p.cB > 256 || p.cH > 4096 || p.cW > 4096 || (p.ups == 1 && (p.cH % 2 != 0 || p.cW % 2 != 0))) return false;
    if ((size_t)p.cB * (p.cH >> p.ups) * (p.cW >> p.ups) * p.cC * 2 >= (1ull << 31) || ((uintptr_t)p.A & 15) != 0) return false;
  }
  if (!dk_gemm_tail_operands_ok(p) || (p.n_split > 0 && p.ldc2 % 8 != 0)) return false;
  if (p.a_seg_len <= 0 || p.c_seg_len <= 0) return false;
  if ((p.kn_w != nullptr && p.conv) || !dk_qknorm_eligible(p)) return false;
  // 16-byte stores in the tail
  if (((uintptr_t)p.C & 15) != 0 || ((uintptr_t)p.C2 & 15) != 0) return false;
  // 32-bit byte offsets on the DMA side: the A rows this problem touches and 8 rows of W
  const size_t a_rows = (size_t)((p.M - 1) / p.a_seg_len) * p.a_seg_stride + (size_t)((p.M - 1) % p.a_seg_len) + 1;
  return (p.conv || a_rows * (size_t)p.lda * 2 < (1ull << 32)) && (size_t)p.ldw * 2 * 8 < (1ull << 31);
}

size_t dk_gemm_split_workspace_bytes() { return DK_KSPLIT_WS_BYTES; }
#endif

// tile-parallel launch of `p` and, optionally, a second problem `p2` with the same N, K, alpha and epilogue: tile height, tiles and K split
// as routed (dk_gemm_route)
int dk_launch_gemm256v3(const GemmParams& p, const GemmParams* p2, const GemmRoute& r, hipStream_t stream) {
#ifndef DK_ELEM_F16
  if (p.dtype == DK_DTYPE_F16) return dk_f16::dk_launch_gemm256v3(p, p2, r, stream);
#endif
  static DkDeviceOnce attr_once;
  if (attr_once.first()) {
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_gemm256v3_kernel<8, false>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_gemm256v3_kernel<7, false>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_gemm256v3_kernel<8, true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_gemm256v3_kernel<7, true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    attr_once.mark();
  }
  SplitArgs sp;
  memset(&sp, 0, sizeof(sp));
  sp.n_dp = r.split.n_dp; sp.n_rem = r.split.n_rem; sp.S = r.split.S; sp.ks = r.split.ks;
  if (r.split.n_rem > 0) {
    sp.slabs = (float*)p.workspace;
    sp.flags = (unsigned*)((char*)p.workspace + DK_KSPLIT_FLAGS_OFF);
    sp.error_word = sp.flags + DK_KSPLIT_ERROR_WORD;
  }
  const GemmParams& pb = p2 ? *p2 : p;
  const int grid = r.split.n_dp + r.split.n_rem * r.split.S;
  double work = 2.0 * (double)p.M * (double)p.N * (double)p.K;
  if (p2) work += 2.0 * (double)p2->M * (double)p2->N * (double)p2->K;
  dk_prof_begin(p.conv ? 1 : 0, work, stream);
  if (p.conv) {
    if (r.tile_rows == 256)
      hipLaunchKernelGGL((dk_gemm256v3_kernel<8, true>), dim3(grid), dim3(512), LDS_BYTES, stream, p, pb, r.tiles_a, r.tiles_b, sp);
    else
      hipLaunchKernelGGL((dk_gemm256v3_kernel<7, true>), dim3(grid), dim3(512), LDS_BYTES, stream, p, pb, r.tiles_a, r.tiles_b, sp);
  } else if (r.tile_rows == 256)
    hipLaunchKernelGGL((dk_gemm256v3_kernel<8, false>), dim3(grid), dim3(512), LDS_BYTES, stream, p, pb, r.tiles_a, r.tiles_b, sp);
  else
    hipLaunchKernelGGL((dk_gemm256v3_kernel<7, false>), dim3(grid), dim3(512), LDS_BYTES, stream, p, pb, r.tiles_a, r.tiles_b, sp);
  dk_prof_end(stream);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}
