// 256 x 256 x 128 fp8 (OCP e4m3) GEMM on the block-scaled MFMA of gfx950: fp8 weights / fp8-quantised activations, fp32
// accumulation, bf16 (or MX-fp8) output -- the Linear layers of the MMDiT blocks for BASELINE.json configs[3]
// ("FLUX.1-dev, fp8 weights / bf16 activations, CDNA4 fp8 MFMA").  Call sites: every nn.Linear of the transformer blocks,
// python/src/diffusionkit/mlx/mmdit.py:821-832 and the fused linear1 / linear2 of the single-stream blocks (:693-751);
// the reference's own quantised path is MLX's 4-bit nn.QuantizedLinear (mlx/model_io.py:728-734,772-775) -- this is the
// MI355X-native counterpart, not a restatement of it.
//
// Number formats
//   W   [N, K] e4m3 + one fp32 scale per output channel (wscale[n], applied in the tail); the hardware scale of the
//       weight operand is the constant 2^0.
//   A   [M, K] e4m3 + one E8M0 scale per (row, 32 consecutive K) -- the OCP MX block format.  The hardware applies it:
//       v_mfma_scale_f32_16x16x128_f8f6f4 takes, per lane, the scale of the lane's (row, 32-K block) from a byte of a VGPR.
//       Scale bytes live in a side array laid out so that ONE coalesced 8-byte load per lane and K-tile brings a wave the
//       scales of its 128 rows (dk_mx_scale_index below); producers: dk_ln_modulate_mx8, dk_quantize_mx8 (fp8_ops.hip)
//       and this kernel's own tail (fc1 + GELU -> fc2's input).
//   C   bf16 like the bf16 kernels, or MX-fp8 (same format as A) when the consumer is another fp8 GEMM.
//
// Kernel shape = the bf16 kernel's (gemm256v3.hip): 8 waves (2 x 4), wave tile 128 (m) x 64 (n), LDS-DMA
// (buffer_load_dwordx4 ... lds) into a ring of two activation + three weight slots of 32 KiB (see LDS_BYTES), hand-counted LDS waits, LDS-staged row-major tail.
// A K-tile is 128 fp8 = 128 bytes per row -- byte-for-byte the bf16 kernel's 64-element tile, so DMA, ring and bank
// behaviour carry over -- and ONE MFMA per (16 x 16) fragment pair consumes it whole: 32 MFMAs of 2 x 16 x 16 x 128 flop per
// wave and K-tile, each twice as long as a bf16 16x16x32 one, i.e. the same MFMA time per K-tile for twice the K depth.
//
// Operand fragment (pinned on hardware by scripts/fp8_probe.hip, profiles/r02_fp8_probe.log): lane (l15 = lane & 15,
// q = lane >> 4) holds row l15; its first four registers are K-elements [16 q, 16 q + 16), its last four [64 + 16 q, 64 + 16 q + 16)
// -- the instruction is two K = 64 halves -- and the scale register byte of lane (l15, g) is the E8M0 scale of row l15, K-elements
// [32 g, 32 g + 32).  Read j of a fragment therefore takes the 16-byte chunk 4 j + q of the row: exactly the bf16 kernel's
// conflict-free pattern (chunk (4 j + q) ^ swz(row)), and the 8 scale bytes a lane loads per K-tile are those of block q.
//
// K-tile schedule (4 steps of 8 MFMAs; A fragments in two sets of two, W fragments in ONE set of four that is reloaded
// fragment by fragment behind its last use):
//   S0  A1 <- m-frags 2,3     MFMA (n 0..3) x (m 0,1), n-major, waiting for W[n] one fragment at a time   + DMA of tile i+1
//   S1  A0 <- m-frags 4,5     MFMA x (m 2,3)
//   S2  A1 <- m-frags 6,7     MFMA x (m 4,5)
//       wait: own DMA pieces + scale load of tile i+1 landed, own reads done; tile barrier
//   S3  A0 <- tile i+1 m 0,1  MFMA x (m 6,7), n-major; W[n] <- tile i+1 right behind its two MFMAs  + DMA of tile i+2
#include <cstring>
#include <type_traits>

#include "dk_kernels.h"
#include "dk_gemm_tail.h"

#ifndef DK_F8_ABL
#define DK_F8_ABL 0  // lab only (timing ablations, results wrong): 1 no scale loads in the K loop, 2 no DMA in it, 4 no fragment reads in it
#endif
#ifndef DK_F8_SAFE
#define DK_F8_SAFE 0  // lab / debugging: every LDS wait is lgkmcnt(0)
#endif

#define T256 256
#define BKB 128                      // bytes (= fp8 elements) of a row per K-tile
#define HALF_BYTES (128 * BKB)       // 128 rows
#define OP_BYTES (2 * HALF_BYTES)    // one operand of one K-tile: rows 0-127, rows 128-255
// LDS ring: two slots of the activation operand, THREE of the weight operand (all 160 KiB): weights stream from HBM (every
// block of the model has its own), activations come out of L2 / Infinity Cache -- so the weight pieces of K-tile i+2 are issued
// 1.75 K-tiles ahead of their first read, the activation pieces 1.0 ahead (the in-order vmcnt lets the newest four stay in flight)
#define W_BASE (2 * OP_BYTES)
#define LDS_BYTES (5 * OP_BYTES)

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef __attribute__((address_space(3))) char lds_char;
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

// position of block `bid` inside the XCD-contiguous order of `count` blocks (hardware places block b on XCD b & 7)
__device__ __forceinline__ int f8_xcd_contiguous(int bid, int count) {
  const int x = bid & 7;
  int start = 0;
  for (int y = 0; y < x; ++y) start += y < count ? (count - y + 7) >> 3 : 0;
  return start + (bid >> 3);
}

// K split of a launch that is at most half a round of tiles (round 6; gemm256v3.hip's SplitArgs for the all-remainder case): every tile is cut into S
// equal K ranges, piece 0 = [0, ks) is the tile's finisher, pieces 1 .. S-1 share [ks, nk) and are producers (raw fp32 accumulators -> slab, flag).
// Block order = dispatch order: the finishers first, then the producers; tiles * S <= #CU, so every workgroup is resident and a finisher's wait ends.
struct F8Split {
  float* slabs;     // [tiles * (S - 1)][512 threads x 32 accumulator quads] fp32, thread-linear (dk_ksplit_store_acc)
  unsigned* flags;  // [tiles * (S - 1)], zero between launches (reset by the finisher)
  unsigned* error_word;
  int S;            // pieces per tile (0 / 1: no split)
  int ks;           // K-tiles of the finisher piece
};

__global__ __launch_bounds__(512, 2) void dk_gemm256f8_kernel(GemmF8Params pa, GemmF8Params pb, int tiles_a, int tiles_b, F8Split sp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if ((unsigned)(size_t)(lds_char*)smem != 0u) __builtin_trap();  // the LDS image is addressed from 0
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int l15 = lane & 15, q = lane >> 4;

  const int n_tiles = tiles_a + tiles_b;
  const int piece = sp.S > 1 ? (int)blockIdx.x / n_tiles : -1;  // -1 whole tile, 0 finisher, >= 1 producer
  const int tile = f8_xcd_contiguous(sp.S > 1 ? (int)blockIdx.x - piece * n_tiles : (int)blockIdx.x, n_tiles);
  const bool second = tile >= tiles_a;
  // ONE scalar base into the kernel-argument segment for this tile's parameter block (round 4; gemm256v3.hip).  Written as
  // `second ? pb : pa` the compiler kept both blocks' M .. c_seg_len in SCRATCH and read them back with dynamically indexed scratch_load_dword
  // (105 sites, vector registers, memory latency at the head of every prologue and tail) and selected the rest field by field: 106 SGPRs + lane
  // spills.  Now 72 SGPRs, 232 VGPRs, no scratch: +7-12 % per launch on the FLUX shapes, FLUX.1-dev fp8 44.2 -> 42.7 ms per step
  // (profiles/r04_gemm_fp8_scalar_params.log, r04_gemm_kernarg_pointer.log).
  static_assert(sizeof(GemmF8Params) % 8 == 0 && alignof(GemmF8Params) == 8, "pb follows pa without padding");
  typedef const __attribute__((address_space(4))) GemmF8Params karg_params_t;
  const __attribute__((address_space(4))) char* kbase = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
  karg_params_t& p = *(karg_params_t*)(kbase + (second ? sizeof(GemmF8Params) : 0));
  // (the twelve ints prologue and tail share, as named scalars)
  const int p_M = p.M;
  const int p_N = p.N;
  const int p_K = p.K;
  const int p_lda = p.lda;
  const int p_ldw = p.ldw;
  const int p_ldc = p.ldc;
  const int p_ldr = p.ldr;
  const int p_a_seg_len = p.a_seg_len;
  const int p_a_seg_stride = p.a_seg_stride;
  const int p_a_row0 = p.a_row0;
  const int p_sa_nblk = p.sa_nblk;
  const int p_c_seg_len = p.c_seg_len;
  const int tl = second ? tile - tiles_a : tile;
  const int nk_full = p_K / BKB;
  int k0 = 0, nk = nk_full;  // this workgroup's K-tile range [k0, k0 + nk)
  if (piece == 0) {
    nk = sp.ks;
  } else if (piece > 0) {
    const int rest = nk_full - sp.ks, np = sp.S - 1;
    k0 = sp.ks + rest * (piece - 1) / np;
    nk = sp.ks + rest * piece / np - k0;
  }
  const int nbm = (p_M + T256 - 1) / T256, nbn = p_N / T256;

  // lane-constant parts of the LDS fragment addresses: row l15 (+ 16 * fragment), read j = position (4 j + q) ^ swz(row)
  unsigned offk[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) offk[j] = (unsigned)(l15 * 128 + (((j * 4 + q) ^ (l15 >> 1)) << 4));
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
  const int m0 = tm * T256, n0 = tn * T256;

  // DMA sources: LDS position (lane & 7) of a row takes global chunk (lane & 7) ^ swz(row) (the read side XORs it back)
  unsigned la[2][2], lw[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int chunk = (lane & 7) ^ (srow >> 1) ^ (4 * j);  // = (lane & 7) ^ swz(row), row = wave * 16 + j * 8 + srow
    lw[j] = (unsigned)srow * (unsigned)p_ldw + chunk * 16;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int m = min(m0 + hh * 128 + wave * 16 + j * 8 + srow, p_M - 1);
      const unsigned phys = (unsigned)((m / p_a_seg_len) * p_a_seg_stride + (m % p_a_seg_len));
      la[hh][j] = phys * (unsigned)p_lda + chunk * 16;
    }
  }
  const char* gA = (const char*)p.A + (size_t)k0 * BKB;
  const char* gW = (const char*)p.W + ((size_t)n0 + wave * 16) * (size_t)p_ldw + (size_t)k0 * BKB;
  const size_t w128 = (size_t)128 * p_ldw, w8 = (size_t)8 * p_ldw;
  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc((void*)gA, 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc((void*)gW, 0, -1, 0x00020000);
  // the four DMA instructions (k: half, j) of one operand of K-tile i; `slot` = byte offset of the ring slot it goes to
  auto issue_a = [&](int i, int k) {
    const int hh = k & 1, j = k >> 1;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_ptr_t)((lds_char*)0 + (i & 1) * OP_BYTES + (wave * 16) * 128 + hh * HALF_BYTES + j * 1024),
                                             16, (int)la[hh][j], i * BKB, 0, 0);
  };
  auto issue_w = [&](int i, unsigned slot, int k) {
    const int hh = k & 1, j = k >> 1;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (lds_ptr_t)((lds_char*)0 + W_BASE + slot + (wave * 16) * 128 + hh * HALF_BYTES + j * 1024), 16,
                                             (int)lw[j], (int)(hh * w128 + j * w8) + i * BKB, 0, 0);
  };

  // E8M0 scales of this wave's 128 A rows for one K-tile: 8 bytes per lane (byte mf = row mf * 16 + l15, block q), one
  // coalesced 512-byte read per wave (layout: dk_mx_scale_index).  The wave's rows must be one aligned 128-row block of the
  // physical buffer (checked by the launcher: every row range starts at a multiple of 128 rows; its last block may be partial).
  // (clamped to the last row block of M: the second wave row of a tile whose rows end at m0 + 128 owns no rows -- its results are
  //  masked -- and must not read scale bytes past the caller's side array)
  const int mrow0 = m0 + wm * 128;
  const int mrow_sc = min(mrow0, (p_M - 1) & ~127);
  const unsigned a_blk = (unsigned)(((mrow_sc / p_a_seg_len) * p_a_seg_stride + (mrow_sc % p_a_seg_len) + p_a_row0) >> 7);
  const size_t sa_step = (size_t)p_sa_nblk * 512;  // bytes between K-tiles
  const unsigned char* sa_ptr = p.SA + ((size_t)a_blk * 64 + lane) * 8 + (size_t)k0 * sa_step;
  u32x2 sa_cur, sa_nxt;

  f32x4 acc[4][8];  // [nf][mf]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

#define F8_RD(DST, ADDR, OFF)                                                                                        \
  do {                                                                                                               \
    if (!(DK_F8_ABL & 4) || !in_loop) asm volatile("ds_read_b128 %0, %1 offset:" #OFF : "=v"(DST) : "v"(ADDR));       \
  } while (0)
// the two m-fragments (MFA, MFA + 1) of a set: 4 reads
#define F8_RDA(SET, BUFOFF, OFFA, OFFB)                 \
  do {                                                  \
    const unsigned a0_ = offk[0] + sA + (BUFOFF);       \
    const unsigned a1_ = offk[1] + sA + (BUFOFF);       \
    F8_RD(SET##lo[0], a0_, OFFA);                       \
    F8_RD(SET##hi[0], a1_, OFFA);                       \
    F8_RD(SET##lo[1], a0_, OFFB);                       \
    F8_RD(SET##hi[1], a1_, OFFB);                       \
  } while (0)
#define F8_RDW(NF, BUFOFF, OFF)                         \
  do {                                                  \
    F8_RD(wlo[NF], offk[0] + sW + (BUFOFF), OFF);       \
    F8_RD(whi[NF], offk[1] + sW + (BUFOFF), OFF);       \
  } while (0)
#if DK_F8_SAFE
#define F8_CNT(N) "0"
#else
#define F8_CNT(N) #N
#endif
#define F8_WAIT2(N, A, B) asm volatile("s_waitcnt lgkmcnt(" F8_CNT(N) ")" : "+v"(A), "+v"(B))
#define F8_WAIT4(N, A, B, C_, D_) asm volatile("s_waitcnt lgkmcnt(" F8_CNT(N) ")" : "+v"(A), "+v"(B), "+v"(C_), "+v"(D_))
#define F8_WAIT6(N, A, B, C_, D_, E_, F_) \
  asm volatile("s_waitcnt lgkmcnt(" F8_CNT(N) ")" : "+v"(A), "+v"(B), "+v"(C_), "+v"(D_), "+v"(E_), "+v"(F_))
// the wait in front of the tile barrier: own fragment reads, own DMA pieces of the next K-tile and its scale load; the four
// weight pieces of K-tile i+2 (the newest four memory operations) stay in flight
#define F8_TILE_WAIT(KEEP, A, B, C_, D_, S_) \
  asm volatile("s_waitcnt vmcnt(" #KEEP ") lgkmcnt(0)" : "+v"(A), "+v"(B), "+v"(C_), "+v"(D_), "+v"(S_)::"memory")
#define F8_FRAG(LO, HI) __builtin_shufflevector(LO, HI, 0, 1, 2, 3, 4, 5, 6, 7)
// one MFMA: acc[NF][MF] += W[NF] . A(SET)[AI]; scale of the activation rows = byte (MF & 3) of sa_cur[MF >> 2]
#define F8_MM(NF, SET, AI, MF)                                                                                              \
  do {                                                                                                                      \
    acc[NF][MF] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(F8_FRAG(wlo[NF], whi[NF]), F8_FRAG(SET##lo[AI], SET##hi[AI]), \
                                                                   acc[NF][MF], 0, 0, 0, 0x7F7F7F7F, (MF) & 3, (int)sa_cur[(MF) >> 2]); \
    __builtin_amdgcn_sched_barrier(0);                                                                                      \
  } while (0)
// a DMA piece in front of MFMA slot SLOT of a step, when this wave group's phase PH puts it there (W: weight pieces, A: activation)
#define F8_PIECE_ON(ON, SLOT, PH) ((ON) && !(DK_F8_ABL & 2) && (SLOT) >= (PH) && (((SLOT) - (PH)) & 1) == 0 && (((SLOT) - (PH)) >> 1) < 4)
#define F8_PIECE_W(ON, TILE, SLOT, PH)                                             \
  do {                                                                             \
    if (F8_PIECE_ON(ON, SLOT, PH)) issue_w((TILE), wo_nn, ((SLOT) - (PH)) >> 1);   \
  } while (0)
#define F8_PIECE_A(ON, TILE, SLOT, PH)                                             \
  do {                                                                             \
    if (F8_PIECE_ON(ON, SLOT, PH)) issue_a((TILE), ((SLOT) - (PH)) >> 1);          \
  } while (0)
// One K-tile.  ON1 / ON2 (compile-time): whether the scales of K-tile i+1 / the DMA pieces of K-tile i+2 (weights in S0,
// activations in S3 -- in that program order, see F8_TILE_WAIT) are issued -- false only in the last two K-tiles, so that the
// steady-state loop carries no branches around them.  wo_cur / wo_nxt / wo_nn: ring slots of the weights of K-tiles i, i+1, i+2.
#define F8_ITER(PH, ON1, ON2)                                                                                       \
  {                                                                                                                 \
    constexpr bool in_loop = true;                                                                                  \
    const unsigned bo = (i & 1) * OP_BYTES;                                                                         \
    /* ---- S0: (n 0..3) x (m 0,1) ---- */                                                                         \
    F8_WAIT6(6, a0lo[0], a0hi[0], a0lo[1], a0hi[1], wlo[0], whi[0]);                                                \
    F8_RDA(a1, bo, 4096, 6144);                                                                                     \
    if ((ON1) && !(DK_F8_ABL & 1)) asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(sa_nxt) : "v"(sa_ptr + (size_t)(i + 1) * sa_step) : "memory"); \
    F8_PIECE_W(ON2, i + 2, 0, PH); F8_MM(0, a0, 0, 0);                                                             \
    F8_PIECE_W(ON2, i + 2, 1, PH); F8_MM(0, a0, 1, 1);                                                             \
    F8_WAIT2(8, wlo[1], whi[1]);                                                                                    \
    F8_PIECE_W(ON2, i + 2, 2, PH); F8_MM(1, a0, 0, 0);                                                             \
    F8_PIECE_W(ON2, i + 2, 3, PH); F8_MM(1, a0, 1, 1);                                                             \
    F8_WAIT2(6, wlo[2], whi[2]);                                                                                    \
    F8_PIECE_W(ON2, i + 2, 4, PH); F8_MM(2, a0, 0, 0);                                                             \
    F8_PIECE_W(ON2, i + 2, 5, PH); F8_MM(2, a0, 1, 1);                                                             \
    F8_WAIT2(4, wlo[3], whi[3]);                                                                                    \
    F8_PIECE_W(ON2, i + 2, 6, PH); F8_MM(3, a0, 0, 0);                                                             \
    F8_PIECE_W(ON2, i + 2, 7, PH); F8_MM(3, a0, 1, 1);                                                             \
    /* ---- S1: x (m 2,3) ---- */                                                                                   \
    F8_RDA(a0, bo, 8192, 10240);                                                                                    \
    F8_WAIT4(4, a1lo[0], a1hi[0], a1lo[1], a1hi[1]);                                                                \
    F8_MM(0, a1, 0, 2); F8_MM(0, a1, 1, 3); F8_MM(1, a1, 0, 2); F8_MM(1, a1, 1, 3);                                 \
    F8_MM(2, a1, 0, 2); F8_MM(2, a1, 1, 3); F8_MM(3, a1, 0, 2); F8_MM(3, a1, 1, 3);                                 \
    /* ---- S2: x (m 4,5) ---- */                                                                                   \
    F8_RDA(a1, bo, 12288, 14336);                                                                                   \
    F8_WAIT4(4, a0lo[0], a0hi[0], a0lo[1], a0hi[1]);                                                                \
    F8_MM(0, a0, 0, 4); F8_MM(0, a0, 1, 5); F8_MM(1, a0, 0, 4); F8_MM(1, a0, 1, 5);                                 \
    F8_MM(2, a0, 0, 4); F8_MM(2, a0, 1, 5); F8_MM(3, a0, 0, 4); F8_MM(3, a0, 1, 5);                                 \
    if (ON2) F8_TILE_WAIT(4, a1lo[0], a1hi[0], a1lo[1], a1hi[1], sa_nxt);                                           \
    else F8_TILE_WAIT(0, a1lo[0], a1hi[0], a1lo[1], a1hi[1], sa_nxt);                                               \
    __builtin_amdgcn_s_barrier();                                                                                   \
    asm volatile("" ::: "memory");                                                                                  \
    /* ---- S3: x (m 6,7); next tile's first A set and, fragment by fragment, its W set ---- */                     \
    F8_RDA(a0, bo ^ OP_BYTES, 0, 2048);  /* unconditional: after the last tile these read stale ring data nobody uses */ \
    F8_PIECE_A(ON2, i + 2, 0, PH); F8_MM(0, a1, 0, 6);                                                             \
    F8_PIECE_A(ON2, i + 2, 1, PH); F8_MM(0, a1, 1, 7);                                                             \
    F8_RDW(0, wo_nxt, 0);                                                                                       \
    F8_PIECE_A(ON2, i + 2, 2, PH); F8_MM(1, a1, 0, 6);                                                             \
    F8_PIECE_A(ON2, i + 2, 3, PH); F8_MM(1, a1, 1, 7);                                                             \
    F8_RDW(1, wo_nxt, 2048);                                                                                    \
    F8_PIECE_A(ON2, i + 2, 4, PH); F8_MM(2, a1, 0, 6);                                                             \
    F8_PIECE_A(ON2, i + 2, 5, PH); F8_MM(2, a1, 1, 7);                                                             \
    F8_RDW(2, wo_nxt, 4096);                                                                                    \
    F8_PIECE_A(ON2, i + 2, 6, PH); F8_MM(3, a1, 0, 6);                                                             \
    F8_PIECE_A(ON2, i + 2, 7, PH); F8_MM(3, a1, 1, 7);                                                             \
    F8_RDW(3, wo_nxt, 6144);                                                                                    \
    sa_cur = sa_nxt;                                                                                                \
    { const unsigned t_ = wo_cur; wo_cur = wo_nxt; wo_nxt = wo_nn; wo_nn = t_; }                                    \
  }
// everything in flight at a section boundary is waited for there (an inline-asm load must not be live across a
// compiler-visible merge)
#define F8_DRAIN()                                                                                                  \
  do {                                                                                                              \
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a0lo[0]), "+v"(a0hi[0]), "+v"(a0lo[1]), "+v"(a0hi[1]));              \
    asm volatile("" : "+v"(wlo[0]), "+v"(whi[0]), "+v"(wlo[1]), "+v"(whi[1]));                                      \
    asm volatile("" : "+v"(wlo[2]), "+v"(whi[2]), "+v"(wlo[3]), "+v"(whi[3]));                                      \
  } while (0)
#define F8_DRIVE(PH)                                     \
  {                                                      \
    int i = 0;                                           \
    for (; i + 2 < nk; ++i) F8_ITER(PH, true, true)      \
    F8_DRAIN();                                          \
    if (i + 1 < nk) {                                    \
      F8_ITER(PH, true, false)                           \
      ++i;                                               \
      F8_DRAIN();                                        \
    }                                                    \
    F8_ITER(PH, false, false)                            \
    F8_DRAIN();                                          \
  }

  {
    i32x4 wlo[4], whi[4], a0lo[2], a0hi[2], a1lo[2], a1hi[2];
    // prologue: scales of K-tile 0, K-tile 0 completely, then K-tile 1 (the loop's first wait lets only its own four weight
    // pieces, of K-tile 2, stay in flight)
    // (the asm load's destination must not be read -- not even copied -- before its wait: no branch-dependent statement names it,
    //  so that no merge of two definitions makes the compiler copy the register while the load is in flight; a first build did)
    unsigned wo_cur = 0u, wo_nxt = OP_BYTES, wo_nn = 2u * OP_BYTES;
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(sa_cur) : "v"(sa_ptr) : "memory");
#pragma unroll
    for (int k = 0; k < 4; ++k) issue_w(0, wo_cur, k);
#pragma unroll
    for (int k = 0; k < 4; ++k) issue_a(0, k);
    if (nk > 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) issue_a(1, k);
#pragma unroll
      for (int k = 0; k < 4; ++k) issue_w(1, wo_nxt, k);
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("" : "+v"(sa_cur));  // from here on the scales of K-tile 0 are there in either case
    sa_nxt = u32x2{0u, 0u};
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // (the first fragment reads sit INSIDE the branches: an inline-asm load that is still in flight must not be live across
    //  a compiler-visible branch)
    constexpr bool in_loop = false;
    if (wm == 0) {
      F8_RDA(a0, 0u, 0, 2048);
      F8_RDW(0, wo_cur, 0); F8_RDW(1, wo_cur, 2048); F8_RDW(2, wo_cur, 4096); F8_RDW(3, wo_cur, 6144);
      F8_DRIVE(0)
    } else {
      F8_RDA(a0, 0u, 0, 2048);
      F8_RDW(0, wo_cur, 0); F8_RDW(1, wo_cur, 2048); F8_RDW(2, wo_cur, 4096); F8_RDW(3, wo_cur, 6144);
      F8_DRIVE(1)
    }
  }
#undef F8_RD
#undef F8_RDA
#undef F8_RDW
#undef F8_WAIT2
#undef F8_WAIT4
#undef F8_WAIT6
#undef F8_TILE_WAIT
#undef F8_MM
#undef F8_PIECE_ON
#undef F8_PIECE_W
#undef F8_PIECE_A
#undef F8_ITER
#undef F8_DRAIN
#undef F8_DRIVE

  // ---------------- K split: producers hand their raw accumulators to the tile's finisher (dk_ksplit.h, gemm256v3.hip's Linear form).
  // The MX scales were applied inside the MFMAs, the weight scale and the bias are applied once, by the finisher's tail: partial sums simply add.
  if (piece >= 0) {
    const int n_prod = sp.S - 1;
    auto leader = [&] { return tid == 0; };
    if (piece >= 1) {
      dk_ksplit_store_acc<8>(sp.slabs + (size_t)(tile * n_prod + piece - 1) * DK_KSPLIT_SLAB_FLOATS + (size_t)tid * 4, 0u, acc);
      dk_ksplit_publish(sp.flags, tile, n_prod, piece, leader);
      return;
    }
    dk_ksplit_wait(sp.flags, tile, n_prod, sp.error_word, leader);
    for (int pp = 0; pp < n_prod; ++pp) dk_ksplit_add_acc<8>(acc, sp.slabs + (size_t)(tile * n_prod + pp) * DK_KSPLIT_SLAB_FLOATS + (size_t)tid * 4, 0u);
    dk_ksplit_release(sp.flags, tile, n_prod, leader);
  }

  // ---------------- tail: accumulators -> LDS (wave-private image) -> row-major (dk_gemm_tail.h) ----------------
  // All waves passed the last loop barrier after their final ds_read of live data, so the ring is free.
  // the weight scales and the bias of this lane's 16 columns (4 per 16-column fragment), all loads up front, in front of the tile set-up (its chain of scalar loads and divisions covers
  // their latency)
  f32x4 ws_q[4];
  u32x2 bias_q[4] = {u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}, u32x2{0u, 0u}};
#pragma unroll
  for (int nf = 0; nf < 4; ++nf) {
    ws_q[nf] = *(const f32x4*)(p.wscale + n0 + wn * 64 + nf * 16 + 4 * q);
    if (p.bias) bias_q[nf] = *(const u32x2*)(p.bias + n0 + wn * 64 + nf * 16 + 4 * q);
  }
  DkTailTile t = dk_tail_tile<false>(p, m0, n0, T256, wm * 128, p_M, p_ldc, p_c_seg_len, p_ldr);
  dk_tail_first_rows<-1>(p, t);
  const bool out_mx8 = (p.n_split > 0 && n0 >= p.n_split) ? p.c2_mx8 != 0 : p.c_mx8 != 0;
  const unsigned reg0 = (unsigned)wave * 16384u;  // this wave's 16 KiB staging image
  const int rrow = lane >> 2;

  // Key tile of a q / k / v projection with the fused QKNorm + RoPE: the sum of squares of every row over its head's columns, from the
  // accumulators
  if (t.kfuse) dk_tail_sumsq_exchange<8>(acc, bias_q, [&](int nf, int e) { return ws_q[nf][e]; }, wave, l15, q);
  // the two 32-column halves of the wave tile (compile-time index: the accumulators must stay in registers)
  auto tail_pass = [&](auto ni_c) {
    constexpr int ni = decltype(ni_c)::value;
    // stage round_bf16(wscale * acc + bias) -- what every epilogue starts from -- as bf16: lane owns row mf*16 + l15, columns
    // (nf & 1)*16 + 4*q + {0..3} of this 32-column half
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      float b4[4];
      unpack2bf(bias_q[ni * 2 + nf][0], b4[0], b4[1]);
      unpack2bf(bias_q[ni * 2 + nf][1], b4[2], b4[3]);
      const f32x4 w4 = ws_q[ni * 2 + nf];
#pragma unroll
      for (int mf = 0; mf < 8; ++mf) {
        const f32x4 a = acc[ni * 2 + nf][mf];
        const unsigned lo = pack2bf(a[0] * w4[0] + b4[0], a[1] * w4[1] + b4[1]), hi = pack2bf(a[2] * w4[2] + b4[2], a[3] * w4[3] + b4[3]);
        *(__attribute__((address_space(3))) u32x2*)((lds_char*)0 + reg0 + dk_tail_stage_off(mf * 16 + l15, nf, q)) = u32x2{lo, hi};
      }
    }
    // the shared row loop, one pass per call; this kernel's own: the MX-fp8 output
    auto rows = [&](auto fast_c, auto ek_c, auto mx_c, auto kf_c) {
      constexpr bool FAST = decltype(fast_c)::value;
      constexpr bool KF = decltype(kf_c)::value;  // key tile with the fused QKNorm + RoPE (bias-only epilogue, bf16 out)
      constexpr int EK = decltype(ek_c)::value;   // the epilogue as a compile-time constant (straight-line row loop), or -1: `epi`
      constexpr int MX = decltype(mx_c)::value;   // output: 1 MX-fp8, 0 bf16, -1: `out_mx8`
      const bool omx = MX >= 0 ? MX == 1 : out_mx8;
      // MX-fp8 output on a tile-uniform row map: a lane's eight rows (itr) are the eight 16-row fragments of its 128-row block, and
      // their scale bytes are the eight consecutive bytes of ONE word of the side array (dk_mx_scale_index: byte (r / 16) % 8) --
      // collected in two registers over the (fully unrolled) loop, stored once per lane quad and 32-column half
      unsigned sc_lo = 0u, sc_hi = 0u;
      auto store_raw = [&](size_t crow, int ocol, bool ok, u32x4 sv) {
        if (ok) *(u32x4*)(t.Cb + crow * (size_t)t.ldcb + ocol) = sv;
      };
      auto store = [&](int itr, size_t crow, int ocol, bool ok, float* vv) {
        if (omx) {
          // MX-fp8 output: the four lanes of a row hold one 32-column block; values are rounded to bf16 first (what the bf16
          // path would have stored), then quantised -- 8 bytes per lane, one scale byte per block
#pragma unroll
          for (int e = 0; e < 8; ++e) vv[e] = round_bf16(vv[e]);
          unsigned e8;
          const uint2 q8 = dk_mx8_quantize8(vv, e8);
          if (ok) *(uint2*)((unsigned char*)t.Cb + crow * (size_t)t.ldcb + ocol) = q8;
          if (FAST) {
            if (itr < 4) sc_lo |= e8 << (8 * (itr & 3));
            else sc_hi |= e8 << (8 * (itr & 3));
          } else if (ok && (lane & 3) == 0) {
            p.SC[dk_mx_scale_index((unsigned)crow + (unsigned)p.c_row0, (unsigned)(p.sc_kb0 + (ocol >> 5)), (unsigned)p.sc_nblk)] = (unsigned char)e8;
          }
        } else {
          const uint4 o4 = dk_tail_pack8(vv);
          store_raw(crow, ocol, ok, u32x4{o4.x, o4.y, o4.z, o4.w});
        }
      };
      dk_tail_rows<FAST, EK, KF, 8, false, 1, MX == 0>(
          p, t, lane, [&](int) { return DkTailPass{reg0, wn * 64 + ni * 32}; }, [&](int, int, int row) { return dk_tail_sumsq_read(wave, row, p.kn_D); },
          store, store_raw);
      if (FAST && omx && (lane & 3) == 0) {
        // rows physC0 + c_row0 + rrow + 16 * {0..7}: one aligned 128-row block (the launcher checks the alignment), bytes 0..7
        const unsigned r0 = (unsigned)t.physC0 + (unsigned)p.c_row0 + (unsigned)rrow;
        const unsigned kb = (unsigned)(p.sc_kb0 + ((t.ncol0 + wn * 64 + ni * 32) >> 5));
        *(uint2*)(p.SC + dk_mx_scale_index(r0, kb, (unsigned)p.sc_nblk)) = make_uint2(sc_lo, sc_hi);
      }
    };
    using Run = std::integral_constant<int, -1>;
    using No = std::false_type;
    using Yes = std::true_type;
    const int epi = t.epi;
    if (t.kfuse) {  // (bias-only epilogue, bf16 out -- checked by the launcher)
      if (t.fast)
        rows(Yes{}, std::integral_constant<int, DK_EPI_BIAS>{}, std::integral_constant<int, 0>{}, Yes{});
      else
        rows(No{}, std::integral_constant<int, DK_EPI_BIAS>{}, std::integral_constant<int, 0>{}, Yes{});
    } else if (t.fast) {
      // the model's combinations with epilogue and output kind folded at compile time (no scalar branches inside the row loop)
      if (epi == DK_EPI_BIAS && !out_mx8)
        rows(Yes{}, std::integral_constant<int, DK_EPI_BIAS>{}, std::integral_constant<int, 0>{}, No{});
      else if (epi == DK_EPI_BIAS_GELU && out_mx8)
        rows(Yes{}, std::integral_constant<int, DK_EPI_BIAS_GELU>{}, std::integral_constant<int, 1>{}, No{});
      else if (epi == DK_EPI_GATE_RES && !out_mx8)
        rows(Yes{}, std::integral_constant<int, DK_EPI_GATE_RES>{}, std::integral_constant<int, 0>{}, No{});
      else
        rows(Yes{}, Run{}, Run{}, No{});
    } else {
      rows(No{}, Run{}, Run{}, No{});
    }
  };
  tail_pass(std::integral_constant<int, 0>{});
  tail_pass(std::integral_constant<int, 1>{});
}

bool dk_gemm256f8_eligible(const GemmF8Params& p) {
  if (p.M <= 0 || p.N % 256 != 0 || p.K % BKB != 0 || p.lda % 16 != 0 || p.ldw % 16 != 0 || p.lda < p.K || p.ldw < p.K) return false;
  if (p.A == nullptr || p.W == nullptr || p.SA == nullptr || p.wscale == nullptr || p.C == nullptr) return false;
  if (!dk_gemm_tail_operands_ok(p) || p.a_seg_len <= 0 || p.c_seg_len <= 0) return false;
  // scale reads: every wave's 128 rows are one aligned 128-row block of the A buffer -- every row range starts on a physical row that is a
  // multiple of 128.  A range may END inside a block (its last block is partial: the DMA clamps to row M - 1, the tail masks rows >= M), so a
  // launch that stays inside its first segment takes any M; only a map of several segments needs whole blocks per segment.
  const bool a_one_seg = p.M <= p.a_seg_len;
  if (p.a_row0 % 128 != 0 || p.sa_nblk <= 0 || (!a_one_seg && (p.a_seg_len % 128 != 0 || p.a_seg_stride % 128 != 0))) return false;
  if ((p.kn_w != nullptr && p.c_mx8) || !dk_qknorm_eligible(p)) return false;  // (the fused QKNorm writes a bf16 first output)
  // outputs: bf16 rows of 16-byte stores, or MX-fp8 rows of 8-byte stores with the scale side array
  auto al = [](const void* q, int a) { return ((uintptr_t)q & (uintptr_t)(a - 1)) == 0; };
  if (p.c_mx8 ? (p.ldc % 8 != 0 || !al(p.C, 8)) : (p.ldc % 8 != 0 || !al(p.C, 16))) return false;
  if (p.n_split > 0 && (p.c2_mx8 ? (p.ldc2 % 8 != 0 || !al(p.C2, 8)) : (p.ldc2 % 8 != 0 || !al(p.C2, 16)))) return false;
  const bool c_one_seg = p.M <= p.c_seg_len;
  if ((p.c_mx8 || (p.n_split > 0 && p.c2_mx8)) &&
      (p.SC == nullptr || p.sc_nblk <= 0 || p.c_row0 % 128 != 0 || (!c_one_seg && (p.c_seg_len % 128 != 0 || p.c_seg_stride % 128 != 0))))
    return false;  // (the tail stores a whole 128-row block's eight scale bytes as one word; the rows of a last, partial block byte by byte)
  // nothing is read or written past the scale side arrays: the last row block a wave touches lies inside sa_nblk / sc_nblk blocks
  const long a_last = (long)p.a_row0 + (long)((p.M - 1) / p.a_seg_len) * p.a_seg_stride + (p.M - 1) % p.a_seg_len;
  if ((a_last >> 7) >= p.sa_nblk) return false;
  if (p.c_mx8 || (p.n_split > 0 && p.c2_mx8)) {
    const long c_last = (long)p.c_row0 + (long)((p.M - 1) / p.c_seg_len) * p.c_seg_stride + (p.M - 1) % p.c_seg_len;
    if ((c_last >> 7) >= p.sc_nblk) return false;
  }
  if (!al(p.wscale, 16)) return false;
  // 32-bit byte offsets on the DMA side
  const size_t a_rows = (size_t)((p.M - 1) / p.a_seg_len) * p.a_seg_stride + (size_t)((p.M - 1) % p.a_seg_len) + 1;
  return a_rows * (size_t)p.lda < (1ull << 32) && (size_t)p.ldw * 8 < (1ull << 31);
}

// tile-parallel launch of `p` and, optionally, a second problem `p2` with the same N, K and epilogues
int dk_launch_gemm256f8(const GemmF8Params& p, const GemmF8Params* p2, hipStream_t stream) {
  DK_REQUIRE(dk_gemm256f8_eligible(p), "gemm256f8: shape / strides / scale layout not eligible");
  if (p2) {
    DK_REQUIRE(dk_gemm256f8_eligible(*p2), "gemm256f8: second problem not eligible");
    DK_REQUIRE(p2->N == p.N && p2->K == p.K && p2->epi == p.epi && p2->n_split == p.n_split && p2->c_mx8 == p.c_mx8 &&
                   (p.n_split == 0 || (p2->epi2 == p.epi2 && p2->c2_mx8 == p.c2_mx8)),
               "grouped fp8 GEMM: N, K, epilogue must match");
  }
  static DkDeviceOnce attr_once;
  if (attr_once.first()) {
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_gemm256f8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    attr_once.mark();
  }
  const int tiles_a = ((p.M + T256 - 1) / T256) * (p.N / T256);
  const int tiles_b = p2 ? ((p2->M + T256 - 1) / T256) * (p2->N / T256) : 0;
  // K split (round 6): the bf16 rule (dk_plan_split; an fp8 K-tile of 128 elements takes as long as a bf16 one of 64) on a launch of at most half a
  // round of tiles, where it cuts every tile -- FLUX's fc2 / linear2 below 1024 x 1024.  (This kernel has no remainder mode, n_dp == 0: its finishers
  // come first and every workgroup is resident.)
  F8Split sp;
  memset(&sp, 0, sizeof(sp));
  const int n_cu = dk_device_cu_count(), tiles = tiles_a + tiles_b;
  const SplitPlan pl = dk_plan_split(tiles, p.K / BKB, dk_ksplit_ws_ok(p, p2), n_cu, true);
  if (tiles * 2 <= (n_cu & ~7) && pl.n_rem > 0) {
    sp.S = pl.S; sp.ks = pl.ks;
    sp.slabs = (float*)p.workspace;
    sp.flags = (unsigned*)((char*)p.workspace + DK_KSPLIT_FLAGS_OFF);
    sp.error_word = sp.flags + DK_KSPLIT_ERROR_WORD;
  }
  const int grid = (tiles_a + tiles_b) * (sp.S > 1 ? sp.S : 1);
  double work = 2.0 * (double)p.M * (double)p.N * (double)p.K;
  if (p2) work += 2.0 * (double)p2->M * (double)p2->N * (double)p2->K;
  dk_prof_begin(3, work, stream);
  hipLaunchKernelGGL(dk_gemm256f8_kernel, dim3(grid), dim3(512), LDS_BYTES, stream, p, p2 ? *p2 : p, tiles_a, tiles_b, sp);
  dk_prof_end(stream);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}
