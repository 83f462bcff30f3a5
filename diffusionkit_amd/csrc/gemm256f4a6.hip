// 256 x 256 x 128 W4A6 GEMM on the block-scaled MFMA of gfx950: OCP MX-fp4 weights (gemm256f4.hip's operand, byte for byte) against MX-fp6
// activations (E2M3, one E8M0 scale per row and 32 consecutive K; weights.py: quantize_activation_mxfp6), fp32 accumulation, bf16 (or MX-fp8)
// output.  v_mfma_scale_f32_16x16x128_f8f6f4 takes 8 passes while either operand is 8 bits wide and 4 when both are 6 bits or narrower
// (profiles/mxfp6_probe.log: 13.4 ns against 6.9 ns per MFMA in one wave): this kernel is gemm256f4.hip with the activation operand at 6 bits.
//
// Operand fragment of the fp6 side (pinned on hardware by scripts/fp6_probe.hip, profiles/mxfp6_probe.log -- hypothesis G0 passes, G1..G3 fail):
// lane (l15, q) holds row l15, K-elements [32 q, 32 q + 32) of the K-tile as 192 bits in its registers 0 .. 5, element e in bits [6 e, 6 e + 6);
// registers 6 and 7 are not read.  The scale byte `opsel` of lane (l15, g) is the scale of row l15, K [32 g, 32 g + 32), as on the fp4 side, whose
// layout does not move when the other operand becomes fp6 (the same log).
//
// Activation layout in memory (written by fp6_ops.hip, restated by weights.py: pack_activation_mxfp6): the mirror of the weight layout.  A is a
// uint8 [rows, lda] array, lda = 96 bytes per K-tile, whose 16-row groups are fragment rows of 16 * lda contiguous bytes; K-tile t of rows
// [16 f, 16 f + 16) is the 1536 bytes at f * 16 * lda + t * 1536: first the leading 16 bytes (registers 0 .. 3) of the 64 lanes at lane * 16, then
// the trailing 8 (registers 4, 5) at 1024 + lane * 8.  A lane's fragment read is one ds_read_b128 and one ds_read_b64, both aligned and linear over
// the wave: no bank conflict, no swizzle.  The 16 fragments of a row tile and K-tile are 24 KiB of LDS, filled by 24 linear 1024-byte
// `buffer_load_dwordx4 ... lds` pieces, three per wave; a piece may straddle two fragments, every lane carries its own global offset (dwordx3
// pieces of 768 bytes would need 32, four per wave, for the same bytes).  Rows past M: the last row group is zero-filled by the quantiser, row
// groups past it are clamped to it -- no load is predicated.
//   SA  the dk_mx_scale_index side array of the MX-fp8 buffers: lane (l15, g) reads the 8 bytes of its eight 16-row fragments.
//
// Ring depth: TWO activation slots of 24 KiB + THREE weight slots of 16 KiB = 96 KiB (the fp4 kernel: 112).  The fp4 kernel's depth is counted in
// K-tiles: activation pieces of K-tile i + 2 go out in the last step of K-tile i and are waited for before the last step of K-tile i + 1, weight
// pieces 1.75 K-tiles ahead of their first read.  With 4-pass MFMAs a K-tile takes half as long, so the same depth covers half the time; the 40 KiB
// that are free below the tail's 132 KiB allocation would hold a third activation slot.  It is NOT spent here: a third slot moves the DMA of the
// activations one K-tile earlier and re-counts every vmcnt of the loop and the prologue, and the counters (profiles/mxfp6_activations.md) show
// no wait it would remove: against the fp4 kernel the MFMA busy time halves, the waves' waiting FALLS (46 % -> 33 % of the wave cycles, LDS 5.6 %),
// and what stays is the issue of the loop's other instructions, the prologue and the tail.
// The hand-counted waits are the fp4 kernel's except for the prologue: three activation pieces per wave and K-tile instead of four.
//
// K-tile schedule (gemm256f4.hip):
//   S0  A1 <- m-frags 2,3     MFMA (n 0..3) x (m 0,1), n-major, waiting for W[n] one fragment at a time   + 2 weight pieces + scales of tile i+1
//   S1  A0 <- m-frags 4,5     MFMA x (m 2,3)
//   S2  A1 <- m-frags 6,7     MFMA x (m 4,5)
//       wait: own DMA pieces + both scale loads of tile i+1 landed (vmcnt(2)), own reads done; barrier
//   S3  A0 <- tile i+1 m 0,1  MFMA x (m 6,7), n-major; W[n] <- tile i+1 right behind its two MFMAs  + 3 activation pieces of tile i+2
#include <cstring>
#include <type_traits>

#include "dk_kernels.h"
#include "dk_gemm_tail.h"

#define T256 256
#define BKB 128                      // K elements per K-tile
#define AFRAG_BYTES 1536             // one activation fragment: 16 rows x 128 K x 6 bits
#define HALF_BYTES (8 * AFRAG_BYTES) // 128 activation rows
#define OP_BYTES (2 * HALF_BYTES)    // the activation operand of one K-tile: 24 KiB
#define WFRAG_BYTES 1024             // one weight fragment: 16 channels x 128 K x 4 bits
#define W_SLOT (16 * WFRAG_BYTES)    // the weight operand of one K-tile
#define W_BASE (2 * OP_BYTES)
#define LDS_BYTES (8 * 16384 + 4096) // ring: W_BASE + 3 * W_SLOT = 96 KiB; tail: 8 staging images + the row-sum exchange (DK_TAIL_XCH_OFF)
static_assert(W_BASE + 3 * W_SLOT <= LDS_BYTES && DK_TAIL_XCH_OFF + 8 * 128 * 4 <= LDS_BYTES, "ring and tail fit the allocation");

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef __attribute__((address_space(3))) char lds_char;
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

// position of block `bid` inside the XCD-contiguous order of `count` blocks (hardware places block b on XCD b & 7)
__device__ __forceinline__ int a6_xcd_contiguous(int bid, int count) {
  const int x = bid & 7;
  int start = 0;
  for (int y = 0; y < x; ++y) start += y < count ? (count - y + 7) >> 3 : 0;
  return start + (bid >> 3);
}

// K split of a launch of at most half a round of tiles: the fp8 kernel's protocol (gemm256f8.hip F8Split; dk_ksplit.h)
struct A6Split {
  float* slabs;
  unsigned* flags;
  unsigned* error_word;
  int S;   // pieces per tile (0 / 1: no split)
  int ks;  // K-tiles of the finisher piece
};

__global__ __launch_bounds__(512, 2) void dk_gemm256f4a6_kernel(GemmF4Params pa, GemmF4Params pb, int tiles_a, int tiles_b, A6Split sp) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if ((unsigned)(size_t)(lds_char*)smem != 0u) __builtin_trap();  // the LDS image is addressed from 0
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int l15 = lane & 15, q = lane >> 4;

  const int n_tiles = tiles_a + tiles_b;
  const int piece = sp.S > 1 ? (int)blockIdx.x / n_tiles : -1;  // -1 whole tile, 0 finisher, >= 1 producer
  const int tile = a6_xcd_contiguous(sp.S > 1 ? (int)blockIdx.x - piece * n_tiles : (int)blockIdx.x, n_tiles);
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

  // activation fragments: registers 0 .. 3 at lane * 16, registers 4, 5 at 1024 + lane * 8 of the 1536 bytes; weight fragments: lane * 16
  const unsigned offk[2] = {(unsigned)lane * 16u, 1024u + (unsigned)lane * 8u};
  const unsigned sA = wm * HALF_BYTES;
  const unsigned sW = W_BASE + wn * 4 * WFRAG_BYTES + (unsigned)lane * 16u;

  const int GROUP = 4;
  const int tpg = GROUP * nbn;
  const int g = tl / tpg;
  const int first_m = g * GROUP;
  const int gsz = min(nbm - first_m, GROUP);
  const int tm = first_m + (tl % tpg) % gsz;
  const int tn = (tl % tpg) / gsz;
  const int m0 = tm * T256, n0 = tn * T256;

  // activation DMA sources: this wave copies the 1024-byte pieces 3 wave .. 3 wave + 2 of the slot's 24; a lane's 16 bytes of a piece lie in
  // fragment (byte / 1536) of the tile, whose row group is clamped to the last one of M (row-group starts are multiples of 16 through the row map)
  unsigned la[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int byte = (wave * 3 + k) * 1024 + lane * 16;
    const int f = byte / AFRAG_BYTES;
    const int m = min(m0 + f * 16, (p_M - 1) & ~15);
    const unsigned phys = (unsigned)((m / p_a_seg_len) * p_a_seg_stride + (m % p_a_seg_len));
    la[k] = (phys >> 4) * 16u * (unsigned)p_lda + (unsigned)(byte - f * AFRAG_BYTES);
  }
  const char* gA = (const char*)p.A + (size_t)k0 * AFRAG_BYTES;
  // weights: this wave copies fragments `wave` and `wave + 8` of the tile's 16, each 1024 contiguous bytes per K-tile
  const char* gW = (const char*)p.W + ((size_t)(n0 >> 4) + wave) * 16 * (size_t)p_ldw + (size_t)k0 * WFRAG_BYTES;
  const int w8f = 8 * 16 * p_ldw;  // bytes between fragment rows f and f + 8 (< 2^31: checked by the launcher)
  const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc((void*)gA, 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc((void*)gW, 0, -1, 0x00020000);
  auto issue_a = [&](int i, int k) {
    // (the LDS address is made from an integer: arithmetic on a null LDS pointer let the compiler pin pieces 1 and 2 of the loop to slot 1)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_ptr_t)(size_t)(unsigned)((i & 1) * OP_BYTES + (wave * 3 + k) * 1024), 16, (int)la[k],
                                             i * AFRAG_BYTES, 0, 0);
  };
  auto issue_w = [&](int i, unsigned slot, int k) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (lds_ptr_t)(size_t)(unsigned)(W_BASE + slot + (wave + 8 * k) * WFRAG_BYTES), 16, lane * 16,
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

#define A6_RD(DST, ADDR, OFF) asm volatile("ds_read_b128 %0, %1 offset:" #OFF : "=v"(DST) : "v"(ADDR))
#define A6_RD64(DST, ADDR, OFF) asm volatile("ds_read_b64 %0, %1 offset:" #OFF : "=v"(DST) : "v"(ADDR))
// the two m-fragments (MFA, MFA + 1) of a set: 4 reads (registers 0 .. 3 and 4, 5 of each)
#define A6_RDA(SET, BUFOFF, OFFA, OFFB)                 \
  do {                                                  \
    const unsigned a0_ = offk[0] + sA + (BUFOFF);       \
    const unsigned a1_ = offk[1] + sA + (BUFOFF);       \
    A6_RD(SET##lo[0], a0_, OFFA);                       \
    A6_RD64(SET##hi[0], a1_, OFFA);                     \
    A6_RD(SET##lo[1], a0_, OFFB);                       \
    A6_RD64(SET##hi[1], a1_, OFFB);                     \
  } while (0)
// one weight fragment: 1 read
#define A6_RDW(NF, BUFOFF, OFF) A6_RD(w[NF], sW + (BUFOFF), OFF)
#define A6_CNT(N) #N
#define A6_WAIT1(N, A) asm volatile("s_waitcnt lgkmcnt(" A6_CNT(N) ")" : "+v"(A))
#define A6_WAIT4(N, A, B, C_, D_) asm volatile("s_waitcnt lgkmcnt(" A6_CNT(N) ")" : "+v"(A), "+v"(B), "+v"(C_), "+v"(D_))
#define A6_WAIT5(N, A, B, C_, D_, E_) asm volatile("s_waitcnt lgkmcnt(" A6_CNT(N) ")" : "+v"(A), "+v"(B), "+v"(C_), "+v"(D_), "+v"(E_))
// the wait in front of the tile barrier: own fragment reads, own DMA pieces of the next K-tile and its two scale loads; the two
// weight pieces of K-tile i+2 (the newest two memory operations) stay in flight
#define A6_TILE_WAIT(KEEP, A, B, C_, D_, S_, T_) \
  asm volatile("s_waitcnt vmcnt(" #KEEP ") lgkmcnt(0)" : "+v"(A), "+v"(B), "+v"(C_), "+v"(D_), "+v"(S_), "+v"(T_)::"memory")
#define A6_AFRAG(LO, HI) __builtin_shufflevector(LO, __builtin_shufflevector(HI, HI, 0, 1, -1, -1), 0, 1, 2, 3, 4, 5, -1, -1)  // (blgp = 2 reads six)
#define A6_WFRAG(W_) __builtin_shufflevector(W_, W_, 0, 1, 2, 3, -1, -1, -1, -1)  // (the builtin's operand type is 8 registers; cbsz = 4 reads four)
// one MFMA: acc[NF][MF] += W[NF] . A(SET)[AI]; weight scale = byte NF of sw_cur, activation scale = byte (MF & 3) of sa_cur[MF >> 2]
#define A6_MM(NF, SET, AI, MF)                                                                                                        \
  do {                                                                                                                                \
    acc[NF][MF] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A6_WFRAG(w[NF]), A6_AFRAG(SET##lo[AI], SET##hi[AI]), acc[NF][MF], 4, 2, \
                                                                   NF, (int)sw_cur, (MF) & 3, (int)sa_cur[(MF) >> 2]);                  \
    __builtin_amdgcn_sched_barrier(0);                                                                                                \
  } while (0)
// a DMA piece in front of MFMA slot SLOT of a step, when this wave group's phase PH puts it there: NP pieces on every other slot from PH on
#define A6_PIECE_ON(ON, SLOT, PH, NP) ((ON) && (SLOT) >= (PH) && (((SLOT) - (PH)) & 1) == 0 && (((SLOT) - (PH)) >> 1) < (NP))
#define A6_PIECE_W(ON, TILE, SLOT, PH)                                                \
  do {                                                                                \
    if (A6_PIECE_ON(ON, SLOT, PH, 2)) issue_w((TILE), wo_nn, ((SLOT) - (PH)) >> 1);   \
  } while (0)
#define A6_PIECE_A(ON, TILE, SLOT, PH)                                                \
  do {                                                                                \
    if (A6_PIECE_ON(ON, SLOT, PH, 3)) issue_a((TILE), ((SLOT) - (PH)) >> 1);          \
  } while (0)
// One K-tile.  ON1 / ON2 (compile-time): whether the scales of K-tile i+1 / the DMA pieces of K-tile i+2 (weights in S0, activations in S3 -- in
// that program order, see A6_TILE_WAIT) are issued.  wo_cur / wo_nxt / wo_nn: ring slots of the weights of K-tiles i, i+1, i+2.
// LDS reads in flight on entry: a0 (4), w[0..3] (1 each), in that order.  Counts: S0 needs a0 + w[0] -> 3 may remain; then +4 (a1) = 7 in
// flight, w[1] -> 6, w[2] -> 5, w[3] -> 4; S1 / S2 as the fp8 kernel (4 + 4 in flight, the older set -> 4).
#define A6_ITER(PH, ON1, ON2)                                                                                       \
  {                                                                                                                 \
    const unsigned bo = (i & 1) * OP_BYTES;                                                                         \
    /* ---- S0: (n 0..3) x (m 0,1) ---- */                                                                         \
    A6_WAIT5(3, a0lo[0], a0hi[0], a0lo[1], a0hi[1], w[0]);                                                          \
    A6_RDA(a1, bo, 3072, 4608);                                                                                     \
    if (ON1) {                                                                                                      \
      asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(sa_nxt) : "v"(sa_ptr + (size_t)(i + 1) * sa_step) : "memory"); \
      asm volatile("global_load_dword %0, %1, off" : "=v"(sw_nxt) : "v"(sw_ptr + (size_t)(i + 1) * 256) : "memory"); \
    }                                                                                                               \
    A6_PIECE_W(ON2, i + 2, 0, PH); A6_MM(0, a0, 0, 0);                                                             \
    A6_PIECE_W(ON2, i + 2, 1, PH); A6_MM(0, a0, 1, 1);                                                             \
    A6_WAIT1(6, w[1]);                                                                                              \
    A6_PIECE_W(ON2, i + 2, 2, PH); A6_MM(1, a0, 0, 0);                                                             \
    A6_PIECE_W(ON2, i + 2, 3, PH); A6_MM(1, a0, 1, 1);                                                             \
    A6_WAIT1(5, w[2]);                                                                                              \
    A6_MM(2, a0, 0, 0);                                                                                             \
    A6_MM(2, a0, 1, 1);                                                                                             \
    A6_WAIT1(4, w[3]);                                                                                              \
    A6_MM(3, a0, 0, 0);                                                                                             \
    A6_MM(3, a0, 1, 1);                                                                                             \
    /* ---- S1: x (m 2,3) ---- */                                                                                   \
    A6_RDA(a0, bo, 6144, 7680);                                                                                     \
    A6_WAIT4(4, a1lo[0], a1hi[0], a1lo[1], a1hi[1]);                                                                \
    A6_MM(0, a1, 0, 2); A6_MM(0, a1, 1, 3); A6_MM(1, a1, 0, 2); A6_MM(1, a1, 1, 3);                                 \
    A6_MM(2, a1, 0, 2); A6_MM(2, a1, 1, 3); A6_MM(3, a1, 0, 2); A6_MM(3, a1, 1, 3);                                 \
    /* ---- S2: x (m 4,5) ---- */                                                                                   \
    A6_RDA(a1, bo, 9216, 10752);                                                                                    \
    A6_WAIT4(4, a0lo[0], a0hi[0], a0lo[1], a0hi[1]);                                                                \
    A6_MM(0, a0, 0, 4); A6_MM(0, a0, 1, 5); A6_MM(1, a0, 0, 4); A6_MM(1, a0, 1, 5);                                 \
    A6_MM(2, a0, 0, 4); A6_MM(2, a0, 1, 5); A6_MM(3, a0, 0, 4); A6_MM(3, a0, 1, 5);                                 \
    if (ON2) A6_TILE_WAIT(2, a1lo[0], a1hi[0], a1lo[1], a1hi[1], sa_nxt, sw_nxt);                                   \
    else A6_TILE_WAIT(0, a1lo[0], a1hi[0], a1lo[1], a1hi[1], sa_nxt, sw_nxt);                                       \
    __builtin_amdgcn_s_barrier();                                                                                   \
    asm volatile("" ::: "memory");                                                                                  \
    /* ---- S3: x (m 6,7); next tile's first A set and, fragment by fragment, its W set ---- */                     \
    A6_RDA(a0, OP_BYTES - bo, 0, 1536);  /* unconditional: after the last tile these read stale ring data nobody uses */ \
    A6_PIECE_A(ON2, i + 2, 0, PH); A6_MM(0, a1, 0, 6);                                                             \
    A6_PIECE_A(ON2, i + 2, 1, PH); A6_MM(0, a1, 1, 7);                                                             \
    A6_RDW(0, wo_nxt, 0);                                                                                           \
    A6_PIECE_A(ON2, i + 2, 2, PH); A6_MM(1, a1, 0, 6);                                                             \
    A6_PIECE_A(ON2, i + 2, 3, PH); A6_MM(1, a1, 1, 7);                                                             \
    A6_RDW(1, wo_nxt, 1024);                                                                                        \
    A6_PIECE_A(ON2, i + 2, 4, PH); A6_MM(2, a1, 0, 6);                                                             \
    A6_PIECE_A(ON2, i + 2, 5, PH); A6_MM(2, a1, 1, 7);                                                             \
    A6_RDW(2, wo_nxt, 2048);                                                                                        \
    A6_PIECE_A(ON2, i + 2, 6, PH); A6_MM(3, a1, 0, 6);                                                             \
    A6_PIECE_A(ON2, i + 2, 7, PH); A6_MM(3, a1, 1, 7);                                                             \
    A6_RDW(3, wo_nxt, 3072);                                                                                        \
    sa_cur = sa_nxt;                                                                                                \
    sw_cur = sw_nxt;                                                                                                \
    { const unsigned t_ = wo_cur; wo_cur = wo_nxt; wo_nxt = wo_nn; wo_nn = t_; }                                    \
  }
// everything in flight at a section boundary is waited for there (an inline-asm load must not be live across a compiler-visible merge)
#define A6_DRAIN()                                                                                                  \
  do {                                                                                                              \
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a0lo[0]), "+v"(a0hi[0]), "+v"(a0lo[1]), "+v"(a0hi[1]));              \
    asm volatile("" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]));                                              \
  } while (0)
#define A6_DRIVE(PH)                                     \
  {                                                      \
    int i = 0;                                           \
    for (; i + 2 < nk; ++i) A6_ITER(PH, true, true)      \
    A6_DRAIN();                                          \
    if (i + 1 < nk) {                                    \
      A6_ITER(PH, true, false)                           \
      ++i;                                               \
      A6_DRAIN();                                        \
    }                                                    \
    A6_ITER(PH, false, false)                            \
    A6_DRAIN();                                          \
  }

  {
    i32x4 w[4], a0lo[2], a1lo[2];
    i32x2 a0hi[2], a1hi[2];
    // prologue: scales of K-tile 0, K-tile 0 completely, then K-tile 1 (the loop's first wait lets only its own two weight pieces, of K-tile 2,
    // stay in flight).  (The asm loads' destinations must not be read -- not even copied -- before their wait: no branch-dependent statement
    // names them.)
    unsigned wo_cur = 0u, wo_nxt = W_SLOT, wo_nn = 2u * W_SLOT;
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(sa_cur) : "v"(sa_ptr) : "memory");
    asm volatile("global_load_dword %0, %1, off" : "=v"(sw_cur) : "v"(sw_ptr) : "memory");
#pragma unroll
    for (int k = 0; k < 2; ++k) issue_w(0, wo_cur, k);
#pragma unroll
    for (int k = 0; k < 3; ++k) issue_a(0, k);
    if (nk > 1) {
#pragma unroll
      for (int k = 0; k < 3; ++k) issue_a(1, k);
#pragma unroll
      for (int k = 0; k < 2; ++k) issue_w(1, wo_nxt, k);
      asm volatile("s_waitcnt vmcnt(5)" ::: "memory");  // 3 activation + 2 weight pieces of K-tile 1 stay in flight
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
      A6_RDA(a0, 0u, 0, 1536);
      A6_RDW(0, wo_cur, 0); A6_RDW(1, wo_cur, 1024); A6_RDW(2, wo_cur, 2048); A6_RDW(3, wo_cur, 3072);
      A6_DRIVE(0)
    } else {
      A6_RDA(a0, 0u, 0, 1536);
      A6_RDW(0, wo_cur, 0); A6_RDW(1, wo_cur, 1024); A6_RDW(2, wo_cur, 2048); A6_RDW(3, wo_cur, 3072);
      A6_DRIVE(1)
    }
  }
#undef A6_RD
#undef A6_RD64
#undef A6_RDA
#undef A6_RDW
#undef A6_WAIT1
#undef A6_WAIT4
#undef A6_WAIT5
#undef A6_TILE_WAIT
#undef A6_MM
#undef A6_PIECE_ON
#undef A6_PIECE_W
#undef A6_PIECE_A
#undef A6_ITER
#undef A6_DRAIN
#undef A6_DRIVE

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
const char* dk_gemm256f4a6_refusal(const GemmF4Params& p) {
  auto al = [](const void* q, int a) { return ((uintptr_t)q & (uintptr_t)(a - 1)) == 0; };
  if (p.M <= 0) return "M <= 0";
  if (p.K <= 0 || p.K % BKB != 0) return "K is not a multiple of 128";
  if (p.N <= 0 || p.N % 256 != 0) return "N is not a multiple of 256";
  if (p.A == nullptr || p.W == nullptr || p.SA == nullptr || p.SW == nullptr || p.wscale == nullptr || p.C == nullptr) return "a null operand";
  if (p.lda % 96 != 0 || p.lda < p.K / BKB * 96) return "activation pitch: a multiple of 96 bytes (whole 1536-byte fragments per 16 rows), at least 96 per K-tile";
  if (!al(p.A, 16)) return "activations not 16-byte aligned";
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
  if ((a_rows + 15) / 16 * 16 * (size_t)p.lda + (size_t)(p.K / BKB) * AFRAG_BYTES >= (1ull << 31)) return "activation buffer beyond 32-bit offsets";
  if ((size_t)p.ldw * 128 + (size_t)(p.K / BKB) * WFRAG_BYTES >= (1ull << 31)) return "weight pitch beyond 32-bit offsets";
  return nullptr;
}

// What a launch of `p` (and `p2`) is: the refusals, the tile counts and the K split -- host only, the launcher and dk_gemm_fp4a6_plan both take it
// from here.  K split: the shared rule (dk_plan_split) on a launch of at most half a round of tiles, where it cuts every tile -- as the fp8 kernel.
int dk_gemm256f4a6_route(const GemmF4Params& p, const GemmF4Params* p2, GemmA6Route& r) {
  if (const char* why = dk_gemm256f4a6_refusal(p)) {
    dk_set_error(std::string("gemm256f4a6: ") + why);
    return -1;
  }
  if (p2) {
    if (const char* why = dk_gemm256f4a6_refusal(*p2)) {
      dk_set_error(std::string("gemm256f4a6: second problem: ") + why);
      return -1;
    }
    DK_REQUIRE(p2->N == p.N && p2->K == p.K && p2->epi == p.epi && p2->n_split == p.n_split && p2->c_mx8 == p.c_mx8 &&
                   (p.n_split == 0 || (p2->epi2 == p.epi2 && p2->c2_mx8 == p.c2_mx8)),
               "grouped fp4 GEMM: N, K, epilogue must match");
  }
  r.tiles_a = ((p.M + T256 - 1) / T256) * (p.N / T256);
  r.tiles_b = p2 ? ((p2->M + T256 - 1) / T256) * (p2->N / T256) : 0;
  r.n_cu = dk_device_cu_count();
  r.S = 0; r.ks = p.K / BKB;
  const int tiles = r.tiles_a + r.tiles_b;
  const SplitPlan pl = dk_plan_split(tiles, p.K / BKB, dk_ksplit_ws_ok(p, p2), r.n_cu, true);
  if (tiles * 2 <= (r.n_cu & ~7) && pl.n_rem > 0) { r.S = pl.S; r.ks = pl.ks; }
  return 0;
}

// tile-parallel launch of `p` and, optionally, a second problem `p2` with the same N, K and epilogues
int dk_launch_gemm256f4a6(const GemmF4Params& p, const GemmF4Params* p2, hipStream_t stream) {
  GemmA6Route r;
  if (const int rc = dk_gemm256f4a6_route(p, p2, r)) return rc;
  static DkDeviceOnce attr_once;
  if (attr_once.first()) {
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_gemm256f4a6_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
    attr_once.mark();
  }
  const int tiles_a = r.tiles_a, tiles_b = r.tiles_b;
  A6Split sp;
  memset(&sp, 0, sizeof(sp));
  if (r.S > 1) {
    sp.S = r.S; sp.ks = r.ks;
    sp.slabs = (float*)p.workspace;
    sp.flags = (unsigned*)((char*)p.workspace + DK_KSPLIT_FLAGS_OFF);
    sp.error_word = sp.flags + DK_KSPLIT_ERROR_WORD;
  }
  const int grid = (tiles_a + tiles_b) * (sp.S > 1 ? sp.S : 1);
  double work = 2.0 * (double)p.M * (double)p.N * (double)p.K;
  if (p2) work += 2.0 * (double)p2->M * (double)p2->N * (double)p2->K;
  dk_prof_begin(3, work, stream);
  hipLaunchKernelGGL(dk_gemm256f4a6_kernel, dim3(grid), dim3(512), LDS_BYTES, stream, p, p2 ? *p2 : p, tiles_a, tiles_b, sp);
  dk_prof_end(stream);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}
