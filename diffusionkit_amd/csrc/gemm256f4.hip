// 256 x 256 x 128 W4A8 GEMM on the block-scaled MFMA of gfx950: OCP MX-fp4 weights (E2M1 elements, one E8M0 scale per output channel and
// 32 consecutive K) against the MX-fp8 activations of the fp8 path (gemm256f8.hip), fp32 accumulation, bf16 (or MX-fp8) output -- the Linear
// layers of the MMDiT blocks at a quarter of the bf16 bytes.  The reference's quantised checkpoints are MLX affine int4 (mlx/model_io.py:728-734);
// this is the hardware's own 4-bit format instead: v_mfma_scale_f32_16x16x128_f8f6f4 takes the fp4 operand (cbsz = 4) and both operands' block
// scales as they are -- there is no dequantiser anywhere.
//
// Number formats
//   W   [N, K] E2M1, two per byte (even K in the low nibble), + SW: one E8M0 byte per (n, 32 K) applied by the hardware, + wscale[n] fp32 applied
//       in the tail (weights.py: quantize_weight_mxfp4 defines all three).
//   A   [M, K] e4m3 + E8M0 per (row, 32 K): the fp8 kernel's operand, byte for byte (dk_mx_scale_index).
//   C   bf16, or MX-fp8 when the consumer is another GEMM of this kind.
//
// Operand fragment of the fp4 side (pinned on hardware by scripts/fp4_probe.hip, profiles/mxfp4_probe.log -- hypothesis H0 passes, H1..H3 fail):
// lane (l15 = lane & 15, q = lane >> 4) holds row l15, K-elements [32 q, 32 q + 32) of the K-tile in its FOUR registers, in order, the even
// element of a byte in the low nibble; the scale byte `opsel` of the scale register of lane (l15, g) is the E8M0 scale of row l15, K-elements
// [32 g, 32 g + 32) -- a lane's scale governs exactly the lane's own data.  (The fp8 side keeps its two K = 64 halves, profiles/r02_fp8_probe.log.)
//
// Weight layout in memory (weights.py: pack_mxfp4; static weights are laid out for the kernel, not row-major).  W is a uint8 [N, ldw] array,
// ldw = dk_weight_pitch_fp4(K) >= K / 2, whose 16-row groups are FRAGMENT ROWS of 16 * ldw contiguous bytes: K-tile t of output channels
// [16 f, 16 f + 16) is the 1024 bytes at f * 16 * ldw + t * 1024, and inside them lane (l15, q)'s 16 bytes sit at (q * 16 + l15) * 16 -- the
// register image of the whole wave, in lane order.  One `buffer_load_dwordx4 ... lds` of a wave therefore copies one fragment (16 channels, where
// the fp8 kernel's 128-byte rows give 8) from 1024 contiguous bytes to 1024 contiguous LDS bytes, and a lane's fragment read is ONE ds_read_b128
// at base + lane * 16: linear over the wave, so there is no bank conflict to argue about and no swizzle on this side.
//   SW  uint8 [N / 64][K / 128][64 lanes][4]: byte nf of lane (l15, g) = scale of channel 64 G + 16 nf + l15, K block 4 t + g -- a wave's 64
//       output channels of one K-tile are one coalesced 256-byte load, four bytes per lane, and fragment nf's MFMAs pick theirs with opsel = nf.
//
// Kernel shape = the fp8 kernel's: 8 waves (2 x 4), wave tile 128 (m) x 64 (n), LDS-DMA ring, hand-counted LDS waits, shared LDS-staged tail
// (dk_gemm_tail.h) and K split (dk_ksplit.h).  A weight slot is 16 KiB instead of 32.  What the freed LDS buys: nothing is spent on it here.
// Two activation slots (64 KiB) + three weight slots (48 KiB) = 112 KiB; a second workgroup per CU would need <= 80 KiB AND half the registers
// (this body holds 128 accumulator + ~100 operand / address VGPRs per lane, as the fp8 one), so occupancy cannot move; the weight ring stays
// three deep because its depth in K-TILES, not in bytes, is what covers the HBM latency (pieces of K-tile i + 2 are issued 1.75 K-tiles ahead of
// their first read, as in the fp8 kernel) and a fourth slot would change the hand-counted vmcnt schedule for a gain nobody has measured.  The
// allocation is 132 KiB: the tail's eight 16 KiB staging images + the 4 KiB row-sum exchange are now what sizes it.
//
// K-tile schedule: the fp8 kernel's four steps of 8 MFMAs with ONE read per weight fragment and TWO weight DMA pieces per wave (fragments
// `wave` and `wave + 8`):
//   S0  A1 <- m-frags 2,3     MFMA (n 0..3) x (m 0,1), n-major, waiting for W[n] one fragment at a time   + 2 weight pieces + scales of tile i+1
//   S1  A0 <- m-frags 4,5     MFMA x (m 2,3)
//   S2  A1 <- m-frags 6,7     MFMA x (m 4,5)
//       wait: own DMA pieces + both scale loads of tile i+1 landed (vmcnt(2): the two weight pieces of tile i+2 stay in flight), own reads done; barrier
//   S3  A0 <- tile i+1 m 0,1  MFMA x (m 6,7), n-major; W[n] <- tile i+1 right behind its two MFMAs  + 4 activation pieces of tile i+2
#include <cstring>
#include <type_traits>

#include "dk_kernels.h"
#include "dk_gemm_tail.h"

#ifndef DK_F4_SAFE
#define DK_F4_SAFE 0  // lab / debugging: every LDS wait is lgkmcnt(0)
#endif

#define T256 256
#define BKB 128                      // fp8 bytes (= K elements) of an activation row per K-tile
#define HALF_BYTES (128 * BKB)       // 128 activation rows
#define OP_BYTES (2 * HALF_BYTES)    // the activation operand of one K-tile
#define WFRAG_BYTES 1024             // one weight fragment: 16 channels x 128 K x 4 bits
#define W_SLOT (16 * WFRAG_BYTES)    // the weight operand of one K-tile
#define W_BASE (2 * OP_BYTES)
#define LDS_BYTES (8 * 16384 + 4096) // ring: W_BASE + 3 * W_SLOT = 112 KiB; tail: 8 staging images + the row-sum exchange (DK_TAIL_XCH_OFF)
static_assert(W_BASE + 3 * W_SLOT <= LDS_BYTES && DK_TAIL_XCH_OFF + 8 * 128 * 4 <= LDS_BYTES, "ring and tail fit the allocation");

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef __attribute__((address_space(3))) char lds_char;
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

// position of block `bid` inside the XCD-contiguous order of `count` blocks (hardware places block b on XCD b & 7)
__device__ __forceinline__ int f4_xcd_contiguous(int bid, int count) {
  const int x = bid & 7;
  int start = 0;
  for (int y = 0; y < x; ++y) start += y < count ? (count - y + 7) >> 3 : 0;
  return start + (bid >> 3);
}

// K split of a launch of at most half a round of tiles: the fp8 kernel's protocol (gemm256f8.hip F8Split; dk_ksplit.h)
struct F4Split {
  float* slabs;
  unsigned* flags;
  unsigned* error_word;
  int S;   // pieces per tile (0 / 1: no split)
  int ks;  // K-tiles of the finisher piece
};

__global__ __launch_bounds__(512, 2) void dk_gemm256f4_kernel(GemmF4Params pa, GemmF4Params pb, int tiles_a, int tiles_b, F4Split sp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if ((unsigned)(size_t)(lds_char*)smem != 0u) __builtin_trap();  // the LDS image is addressed from 0
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int l15 = lane & 15, q = lane >> 4;

  const int n_tiles = tiles_a + tiles_b;
  const int piece = sp.S > 1 ? (int)blockIdx.x / n_tiles : -1;  // -1 whole tile, 0 finisher, >= 1 producer
  const int tile = f4_xcd_contiguous(sp.S > 1 ? (int)blockIdx.x - piece * n_tiles : (int)blockIdx.x, n_tiles);
  const bool second = tile >= tiles_a;
  // one scalar base into the kernel-argument segment for this tile's parameter block (gemm256f8.hip: `second ? pb : pa` went through scratch)
  static_assert(sizeof(GemmF4Params) % 8 == 0 && alignof(GemmF4Params) == 8, "pb follows pa without padding");
  typedef const __attribute__((address_space(4))) GemmF4Params karg_params_t;
  const __attribute__((address_space(4))) char* kbase = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
  karg_params_t& p = *(karg_params_t*)(kbase + (second ? sizeof(GemmF4Params) : 0));
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

  // activation fragments: row l15 (+ 16 * fragment), read j = position (4 j + q) ^ swz(row) (the fp8 kernel's); weight fragments: lane * 16
  unsigned offk[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) offk[j] = (unsigned)(l15 * 128 + (((j * 4 + q) ^ (l15 >> 1)) << 4));
  const unsigned sA = wm * HALF_BYTES;
  const unsigned sW = W_BASE + wn * 4 * WFRAG_BYTES + (unsigned)lane * 16u;

  const int srow = lane >> 3;
  const int GROUP = 4;
  const int tpg = GROUP * nbn;
  const int g = tl / tpg;
  const int first_m = g * GROUP;
  const int gsz = min(nbm - first_m, GROUP);
  const int tm = first_m + (tl % tpg) % gsz;
  const int tn = (tl % tpg) / gsz;
  const int m0 = tm * T256, n0 = tn * T256;

  // activation DMA sources: LDS position (lane & 7) of a row takes global chunk (lane & 7) ^ swz(row) (the read side XORs it back)
  unsigned la[2][2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int chunk = (lane & 7) ^ (srow >> 1) ^ (4 * j);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int m = min(m0 + hh * 128 + wave * 16 + j * 8 + srow, p_M - 1);
      const unsigned phys = (unsigned)((m / p_a_seg_len) * p_a_seg_stride + (m % p_a_seg_len));
      la[hh][j] = phys * (unsigned)p_lda + chunk * 16;
    }
  }
  const char* gA = (const char*)p.A + (size_t)k0 * BKB;
  // weights: this wave copies fragments `wave` and `wave + 8` of the tile's 16, each 1024 contiguous bytes per K-tile
  const char* gW = (const char*)p.W + ((size_t)(n0 >> 4) + wave) * 16 * (size_t)p_ldw + (size_t)k0 * WFRAG_BYTES;
  const int w8f = 8 * 16 * p_ldw;  // bytes between fragment rows f and f + 8 (< 2^31: checked by the launcher)
  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc((void*)gA, 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc((void*)gW, 0, -1, 0x00020000);
  auto issue_a = [&](int i, int k) {
    const int hh = k & 1, j = k >> 1;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_ptr_t)((lds_char*)0 + (i & 1) * OP_BYTES + (wave * 16) * 128 + hh * HALF_BYTES + j * 1024),
                                             16, (int)la[hh][j], i * BKB, 0, 0);
  };
  auto issue_w = [&](int i, unsigned slot, int k) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (lds_ptr_t)((lds_char*)0 + W_BASE + slot + (wave + 8 * k) * WFRAG_BYTES), 16, lane * 16,
                                             k * w8f + i * WFRAG_BYTES, 0, 0);
  };

  // E8M0 scales of this wave's 128 A rows for one K-tile (gemm256f8.hip: 8 bytes per lane, clamped to the last row block of M) ...
  const int mrow0 = m0 + wm * 128;
  const int mrow_sc = min(mrow0, (p_M - 1) & ~127);
  const unsigned a_blk = (unsigned)(((mrow_sc / p_a_seg_len) * p_a_seg_stride + (mrow_sc % p_a_seg_len) + p_a_row0) >> 7);
  const size_t sa_step = (size_t)p_sa_nblk * 512;  // bytes between K-tiles
  const unsigned char* sa_ptr = p.SA + ((size_t)a_blk * 64 + lane) * 8 + (size_t)k0 * sa_step;
  u32x2 sa_cur, sa_nxt;
  // ... and of its 64 weight channels: 4 bytes per lane, 256 bytes per wave and K-tile
  const unsigned char* sw_ptr = p.SW + (((size_t)(n0 >> 6) + wn) * nk_full + k0) * 256 + lane * 4;
  unsigned sw_cur, sw_nxt;

  f32x4 acc[4][8];  // [nf][mf]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

#define F4_RD(DST, ADDR, OFF) asm volatile("ds_read_b128 %0, %1 offset:" #OFF : "=v"(DST) : "v"(ADDR))
// the two m-fragments (MFA, MFA + 1) of a set: 4 reads
#define F4_RDA(SET, BUFOFF, OFFA, OFFB)                 \
  do {                                                  \
    const unsigned a0_ = offk[0] + sA + (BUFOFF);       \
    const unsigned a1_ = offk[1] + sA + (BUFOFF);       \
    F4_RD(SET##lo[0], a0_, OFFA);                       \
    F4_RD(SET##hi[0], a1_, OFFA);                       \
    F4_RD(SET##lo[1], a0_, OFFB);                       \
    F4_RD(SET##hi[1], a1_, OFFB);                       \
  } while (0)
// one weight fragment: 1 read
#define F4_RDW(NF, BUFOFF, OFF) F4_RD(w[NF], sW + (BUFOFF), OFF)
#if DK_F4_SAFE
#define F4_CNT(N) "0"
#else
#define F4_CNT(N) #N
#endif
#define F4_WAIT1(N, A) asm volatile("s_waitcnt lgkmcnt(" F4_CNT(N) ")" : "+v"(A))
#define F4_WAIT4(N, A, B, C_, D_) asm volatile("s_waitcnt lgkmcnt(" F4_CNT(N) ")" : "+v"(A), "+v"(B), "+v"(C_), "+v"(D_))
#define F4_WAIT5(N, A, B, C_, D_, E_) asm volatile("s_waitcnt lgkmcnt(" F4_CNT(N) ")" : "+v"(A), "+v"(B), "+v"(C_), "+v"(D_), "+v"(E_))
// the wait in front of the tile barrier: own fragment reads, own DMA pieces of the next K-tile and its two scale loads; the two
// weight pieces of K-tile i+2 (the newest two memory operations) stay in flight
#define F4_TILE_WAIT(KEEP, A, B, C_, D_, S_, T_) \
  asm volatile("s_waitcnt vmcnt(" #KEEP ") lgkmcnt(0)" : "+v"(A), "+v"(B), "+v"(C_), "+v"(D_), "+v"(S_), "+v"(T_)::"memory")
#define F4_AFRAG(LO, HI) __builtin_shufflevector(LO, HI, 0, 1, 2, 3, 4, 5, 6, 7)
#define F4_WFRAG(W_) __builtin_shufflevector(W_, W_, 0, 1, 2, 3, -1, -1, -1, -1)  // (the builtin's operand type is 8 registers; cbsz = 4 reads four)
// one MFMA: acc[NF][MF] += W[NF] . A(SET)[AI]; weight scale = byte NF of sw_cur, activation scale = byte (MF & 3) of sa_cur[MF >> 2]
#define F4_MM(NF, SET, AI, MF)                                                                                                        \
  do {                                                                                                                                \
    acc[NF][MF] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(F4_WFRAG(w[NF]), F4_AFRAG(SET##lo[AI], SET##hi[AI]), acc[NF][MF], 4, 0, \
                                                                   NF, (int)sw_cur, (MF) & 3, (int)sa_cur[(MF) >> 2]);                  \
    __builtin_amdgcn_sched_barrier(0);                                                                                                \
  } while (0)
// a DMA piece in front of MFMA slot SLOT of a step, when this wave group's phase PH puts it there: NP pieces on every other slot from PH on
#define F4_PIECE_ON(ON, SLOT, PH, NP) ((ON) && (SLOT) >= (PH) && (((SLOT) - (PH)) & 1) == 0 && (((SLOT) - (PH)) >> 1) < (NP))
#define F4_PIECE_W(ON, TILE, SLOT, PH)                                                \
  do {                                                                                \
    if (F4_PIECE_ON(ON, SLOT, PH, 2)) issue_w((TILE), wo_nn, ((SLOT) - (PH)) >> 1);   \
  } while (0)
#define F4_PIECE_A(ON, TILE, SLOT, PH)                                                \
  do {                                                                                \
    if (F4_PIECE_ON(ON, SLOT, PH, 4)) issue_a((TILE), ((SLOT) - (PH)) >> 1);          \
  } while (0)
// One K-tile.  ON1 / ON2 (compile-time): whether the scales of K-tile i+1 / the DMA pieces of K-tile i+2 (weights in S0, activations in S3 -- in
// that program order, see F4_TILE_WAIT) are issued.  wo_cur / wo_nxt / wo_nn: ring slots of the weights of K-tiles i, i+1, i+2.
// LDS reads in flight on entry: a0 (4), w[0..3] (1 each), in that order.  Counts: S0 needs a0 + w[0] -> 3 may remain; then +4 (a1) = 7 in
// flight, w[1] -> 6, w[2] -> 5, w[3] -> 4; S1 / S2 as the fp8 kernel (4 + 4 in flight, the older set -> 4).
#define F4_ITER(PH, ON1, ON2)                                                                                       \
  {                                                                                                                 \
    const unsigned bo = (i & 1) * OP_BYTES;                                                                         \
    /* ---- S0: (n 0..3) x (m 0,1) ---- */                                                                         \
    F4_WAIT5(3, a0lo[0], a0hi[0], a0lo[1], a0hi[1], w[0]);                                                          \
    F4_RDA(a1, bo, 4096, 6144);                                                                                     \
    if (ON1) {                                                                                                      \
      asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(sa_nxt) : "v"(sa_ptr + (size_t)(i + 1) * sa_step) : "memory"); \
      asm volatile("global_load_dword %0, %1, off" : "=v"(sw_nxt) : "v"(sw_ptr + (size_t)(i + 1) * 256) : "memory"); \
    }                                                                                                               \
    F4_PIECE_W(ON2, i + 2, 0, PH); F4_MM(0, a0, 0, 0);                                                             \
    F4_PIECE_W(ON2, i + 2, 1, PH); F4_MM(0, a0, 1, 1);                                                             \
    F4_WAIT1(6, w[1]);                                                                                              \
    F4_PIECE_W(ON2, i + 2, 2, PH); F4_MM(1, a0, 0, 0);                                                             \
    F4_PIECE_W(ON2, i + 2, 3, PH); F4_MM(1, a0, 1, 1);                                                             \
    F4_WAIT1(5, w[2]);                                                                                              \
    F4_MM(2, a0, 0, 0);                                                                                             \
    F4_MM(2, a0, 1, 1);                                                                                             \
    F4_WAIT1(4, w[3]);                                                                                              \
    F4_MM(3, a0, 0, 0);                                                                                             \
    F4_MM(3, a0, 1, 1);                                                                                             \
    /* ---- S1: x (m 2,3) ---- */                                                                                   \
    F4_RDA(a0, bo, 8192, 10240);                                                                                    \
    F4_WAIT4(4, a1lo[0], a1hi[0], a1lo[1], a1hi[1]);                                                                \
    F4_MM(0, a1, 0, 2); F4_MM(0, a1, 1, 3); F4_MM(1, a1, 0, 2); F4_MM(1, a1, 1, 3);                                 \
    F4_MM(2, a1, 0, 2); F4_MM(2, a1, 1, 3); F4_MM(3, a1, 0, 2); F4_MM(3, a1, 1, 3);                                 \
    /* ---- S2: x (m 4,5) ---- */                                                                                   \
    F4_RDA(a1, bo, 12288, 14336);                                                                                   \
    F4_WAIT4(4, a0lo[0], a0hi[0], a0lo[1], a0hi[1]);                                                                \
    F4_MM(0, a0, 0, 4); F4_MM(0, a0, 1, 5); F4_MM(1, a0, 0, 4); F4_MM(1, a0, 1, 5);                                 \
    F4_MM(2, a0, 0, 4); F4_MM(2, a0, 1, 5); F4_MM(3, a0, 0, 4); F4_MM(3, a0, 1, 5);                                 \
    if (ON2) F4_TILE_WAIT(2, a1lo[0], a1hi[0], a1lo[1], a1hi[1], sa_nxt, sw_nxt);                                   \
    else F4_TILE_WAIT(0, a1lo[0], a1hi[0], a1lo[1], a1hi[1], sa_nxt, sw_nxt);                                       \
    __builtin_amdgcn_s_barrier();                                                                                   \
    asm volatile("" ::: "memory");                                                                                  \
    /* ---- S3: x (m 6,7); next tile's first A set and, fragment by fragment, its W set ---- */                     \
    F4_RDA(a0, bo ^ OP_BYTES, 0, 2048);  /* unconditional: after the last tile these read stale ring data nobody uses */ \
    F4_PIECE_A(ON2, i + 2, 0, PH); F4_MM(0, a1, 0, 6);                                                             \
    F4_PIECE_A(ON2, i + 2, 1, PH); F4_MM(0, a1, 1, 7);                                                             \
    F4_RDW(0, wo_nxt, 0);                                                                                           \
    F4_PIECE_A(ON2, i + 2, 2, PH); F4_MM(1, a1, 0, 6);                                                             \
    F4_PIECE_A(ON2, i + 2, 3, PH); F4_MM(1, a1, 1, 7);                                                             \
    F4_RDW(1, wo_nxt, 1024);                                                                                        \
    F4_PIECE_A(ON2, i + 2, 4, PH); F4_MM(2, a1, 0, 6);                                                             \
    F4_PIECE_A(ON2, i + 2, 5, PH); F4_MM(2, a1, 1, 7);                                                             \
    F4_RDW(2, wo_nxt, 2048);                                                                                        \
    F4_PIECE_A(ON2, i + 2, 6, PH); F4_MM(3, a1, 0, 6);                                                             \
    F4_PIECE_A(ON2, i + 2, 7, PH); F4_MM(3, a1, 1, 7);                                                             \
    F4_RDW(3, wo_nxt, 3072);                                                                                        \
    sa_cur = sa_nxt;                                                                                                \
    sw_cur = sw_nxt;                                                                                                \
    { const unsigned t_ = wo_cur; wo_cur = wo_nxt; wo_nxt = wo_nn; wo_nn = t_; }                                    \
  }
// everything in flight at a section boundary is waited for there (an inline-asm load must not be live across a compiler-visible merge)
#define F4_DRAIN()                                                                                                  \
  do {                                                                                                              \
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a0lo[0]), "+v"(a0hi[0]), "+v"(a0lo[1]), "+v"(a0hi[1]));              \
    asm volatile("" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]));                                              \
  } while (0)
#define F4_DRIVE(PH)                                     \
  {                                                      \
    int i = 0;                                           \
    for (; i + 2 < nk; ++i) F4_ITER(PH, true, true)      \
    F4_DRAIN();                                          \
    if (i + 1 < nk) {                                    \
      F4_ITER(PH, true, false)                           \
      ++i;                                               \
      F4_DRAIN();                                        \
    }                                                    \
    F4_ITER(PH, false, false)                            \
    F4_DRAIN();                                          \
  }

  {
    i32x4 w[4], a0lo[2], a0hi[2], a1lo[2], a1hi[2];
    // prologue: scales of K-tile 0, K-tile 0 completely, then K-tile 1 (the loop's first wait lets only its own two weight pieces, of K-tile 2,
    // stay in flight).  (The asm loads' destinations must not be read -- not even copied -- before their wait: no branch-dependent statement
    // names them.)
    unsigned wo_cur = 0u, wo_nxt = W_SLOT, wo_nn = 2u * W_SLOT;
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(sa_cur) : "v"(sa_ptr) : "memory");
    asm volatile("global_load_dword %0, %1, off" : "=v"(sw_cur) : "v"(sw_ptr) : "memory");
#pragma unroll
    for (int k = 0; k < 2; ++k) issue_w(0, wo_cur, k);
#pragma unroll
    for (int k = 0; k < 4; ++k) issue_a(0, k);
    if (nk > 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) issue_a(1, k);
#pragma unroll
      for (int k = 0; k < 2; ++k) issue_w(1, wo_nxt, k);
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("" : "+v"(sa_cur), "+v"(sw_cur));  // from here on the scales of K-tile 0 are there in either case
    sa_nxt = u32x2{0u, 0u};
    sw_nxt = 0u;
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    // (the first fragment reads sit INSIDE the branches: an inline-asm load that is still in flight must not be live across a
    //  compiler-visible branch)
    if (wm == 0) {
      F4_RDA(a0, 0u, 0, 2048);
      F4_RDW(0, wo_cur, 0); F4_RDW(1, wo_cur, 1024); F4_RDW(2, wo_cur, 2048); F4_RDW(3, wo_cur, 3072);
      F4_DRIVE(0)
    } else {
      F4_RDA(a0, 0u, 0, 2048);
      F4_RDW(0, wo_cur, 0); F4_RDW(1, wo_cur, 1024); F4_RDW(2, wo_cur, 2048); F4_RDW(3, wo_cur, 3072);
      F4_DRIVE(1)
    }
  }
#undef F4_RD
#undef F4_RDA
#undef F4_RDW
#undef F4_WAIT1
#undef F4_WAIT4
#undef F4_WAIT5
#undef F4_TILE_WAIT
#undef F4_MM
#undef F4_PIECE_ON
#undef F4_PIECE_W
#undef F4_PIECE_A
#undef F4_ITER
#undef F4_DRAIN
#undef F4_DRIVE

  // ---------------- K split: producers hand their raw accumulators to the tile's finisher (dk_ksplit.h), exactly as the fp8 kernel does: both
  // operands' block scales were applied inside the MFMAs, wscale and the bias are applied once, by the finisher's tail -- partial sums simply add.
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

  // ---------------- tail: accumulators -> LDS (wave-private image) -> row-major (dk_gemm_tail.h), the fp8 kernel's statement for statement ----
  // All waves passed the last loop barrier after their final ds_read of live data, so the ring is free.
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

  if (t.kfuse) dk_tail_sumsq_exchange<8>(acc, bias_q, [&](int nf, int e) { return ws_q[nf][e]; }, wave, l15, q);
  // the two 32-column halves of the wave tile (compile-time index: the accumulators must stay in registers)
  auto tail_pass = [&](auto ni_c) {
    constexpr int ni = decltype(ni_c)::value;
    // stage round_bf16(wscale * acc + bias) as bf16: lane owns row mf*16 + l15, columns (nf & 1)*16 + 4*q + {0..3} of this 32-column half
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
    // the shared row loop, one pass per call; with the MX-fp8 output of the fp8 kernel
    auto rows = [&](auto fast_c, auto ek_c, auto mx_c, auto kf_c) {
      constexpr bool FAST = decltype(fast_c)::value;
      constexpr bool KF = decltype(kf_c)::value;
      constexpr int EK = decltype(ek_c)::value;
      constexpr int MX = decltype(mx_c)::value;  // output: 1 MX-fp8, 0 bf16, -1: `out_mx8`
      const bool omx = MX >= 0 ? MX == 1 : out_mx8;
      unsigned sc_lo = 0u, sc_hi = 0u;
      auto store_raw = [&](size_t crow, int ocol, bool ok, u32x4 sv) {
        if (ok) *(u32x4*)(t.Cb + crow * (size_t)t.ldcb + ocol) = sv;
      };
      auto store = [&](int itr, size_t crow, int ocol, bool ok, float* vv) {
        if (omx) {
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

// what this kernel cannot take, by name (nullptr: eligible)
const char* dk_gemm256f4_refusal(const GemmF4Params& p) {
  auto al = [](const void* q, int a) { return ((uintptr_t)q & (uintptr_t)(a - 1)) == 0; };
  if (p.M <= 0) return "M <= 0";
  if (p.K <= 0 || p.K % BKB != 0) return "K is not a multiple of 128";
  if (p.N <= 0 || p.N % 256 != 0) return "N is not a multiple of 256";
  if (p.A == nullptr || p.W == nullptr || p.SA == nullptr || p.SW == nullptr || p.wscale == nullptr || p.C == nullptr) return "a null operand";
  if (p.lda % 16 != 0 || p.lda < p.K) return "activation pitch: a multiple of 16 bytes, at least K";
  if (p.ldw % 64 != 0 || p.ldw < p.K / 2) return "weight pitch: a multiple of 64 bytes (whole 1024-byte fragments per 16 channels), at least K / 2";
  if (!al(p.W, 16)) return "weights not 16-byte aligned";
  if (!al(p.SW, 4) || !al(p.SA, 8)) return "misaligned scale array (weights: 4 bytes, activations: 8)";
  if (!al(p.wscale, 16)) return "wscale not 16-byte aligned";
  if (!dk_gemm_tail_operands_ok(p) || p.a_seg_len <= 0 || p.c_seg_len <= 0) return "tail operands (column split, residual, gate, bias) or row maps";
  // activation scale reads: every wave's 128 rows are one aligned 128-row block of the A buffer (gemm256f8.hip)
  const bool a_one_seg = p.M <= p.a_seg_len;
  if (p.a_row0 % 128 != 0 || p.sa_nblk <= 0 || (!a_one_seg && (p.a_seg_len % 128 != 0 || p.a_seg_stride % 128 != 0)))
    return "activation row ranges must start on 128-row scale blocks";
  if ((p.kn_w != nullptr && p.c_mx8) || !dk_qknorm_eligible(p)) return "fused QKNorm: bf16 first output, whole 256-column tiles";
  if (p.c_mx8 ? (p.ldc % 8 != 0 || !al(p.C, 8)) : (p.ldc % 8 != 0 || !al(p.C, 16))) return "output pitch / alignment";
  if (p.n_split > 0 && (p.c2_mx8 ? (p.ldc2 % 8 != 0 || !al(p.C2, 8)) : (p.ldc2 % 8 != 0 || !al(p.C2, 16)))) return "second output pitch / alignment";
  const bool c_one_seg = p.M <= p.c_seg_len;
  if ((p.c_mx8 || (p.n_split > 0 && p.c2_mx8)) &&
      (p.SC == nullptr || p.sc_nblk <= 0 || p.c_row0 % 128 != 0 || (!c_one_seg && (p.c_seg_len % 128 != 0 || p.c_seg_stride % 128 != 0))))
    return "MX-fp8 output: scale array, row ranges on 128-row scale blocks";
  const long a_last = (long)p.a_row0 + (long)((p.M - 1) / p.a_seg_len) * p.a_seg_stride + (p.M - 1) % p.a_seg_len;
  if ((a_last >> 7) >= p.sa_nblk) return "activation rows past the scale array";
  if (p.c_mx8 || (p.n_split > 0 && p.c2_mx8)) {
    const long c_last = (long)p.c_row0 + (long)((p.M - 1) / p.c_seg_len) * p.c_seg_stride + (p.M - 1) % p.c_seg_len;
    if ((c_last >> 7) >= p.sc_nblk) return "output rows past the scale array";
  }
  // 32-bit byte offsets on the DMA side: activation rows, and weight fragment row f + 8 plus the K-tile offset
  const size_t a_rows = (size_t)((p.M - 1) / p.a_seg_len) * p.a_seg_stride + (size_t)((p.M - 1) % p.a_seg_len) + 1;
  if (a_rows * (size_t)p.lda >= (1ull << 32)) return "activation buffer beyond 32-bit offsets";
  if ((size_t)p.ldw * 128 + (size_t)(p.K / BKB) * WFRAG_BYTES >= (1ull << 31)) return "weight pitch beyond 32-bit offsets";
  return nullptr;
}
bool dk_gemm256f4_eligible(const GemmF4Params& p) { return dk_gemm256f4_refusal(p) == nullptr; }

// tile-parallel launch of `p` and, optionally, a second problem `p2` with the same N, K and epilogues
int dk_launch_gemm256f4(const GemmF4Params& p, const GemmF4Params* p2, hipStream_t stream) {
  if (const char* why = dk_gemm256f4_refusal(p)) {
    dk_set_error(std::string("gemm256f4: ") + why);
    return -1;
  }
  if (p2) {
    if (const char* why = dk_gemm256f4_refusal(*p2)) {
      dk_set_error(std::string("gemm256f4: second problem: ") + why);
      return -1;
    }
    DK_REQUIRE(p2->N == p.N && p2->K == p.K && p2->epi == p.epi && p2->n_split == p.n_split && p2->c_mx8 == p.c_mx8 &&
                   (p.n_split == 0 || (p2->epi2 == p.epi2 && p2->c2_mx8 == p.c2_mx8)),
               "grouped fp4 GEMM: N, K, epilogue must match");
  }
  static DkDeviceOnce attr_once;
  if (attr_once.first()) {
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_gemm256f4_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    attr_once.mark();
  }
  const int tiles_a = ((p.M + T256 - 1) / T256) * (p.N / T256);
  const int tiles_b = p2 ? ((p2->M + T256 - 1) / T256) * (p2->N / T256) : 0;
  // K split: the shared rule (dk_plan_split) on a launch of at most half a round of tiles, where it cuts every tile -- as the fp8 kernel
  F4Split sp;
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
  hipLaunchKernelGGL(dk_gemm256f4_kernel, dim3(grid), dim3(512), LDS_BYTES, stream, p, p2 ? *p2 : p, tiles_a, tiles_b, sp);
  dk_prof_end(stream);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}
