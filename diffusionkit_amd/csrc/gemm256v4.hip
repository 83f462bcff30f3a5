// 256 x 256 x 64 bf16 MFMA GEMM, fourth generation: ONE wave per SIMD (256 threads), a 128 x 128 block of the tile per wave with its
// 256 accumulators in AGPRs, and the whole main body -- prologue DMA, K loop, the two peeled last K-tiles, the drain of the accumulators
// into the bf16 staging image -- as ONE hand-scheduled inline-asm block with the register file addressed by hand
// (gemm256v4_asm.inc, written and CPU-checked by scripts/gen_gemm256v4.py: an instruction-level emulator runs the same instruction
// list with every DMA piece and LDS read completing as late, or as early, as its waits allow).  Same contract, grouped launch, column
// split and epilogues as gemm256v3.hip; nn.Linear call sites python/src/diffusionkit/mlx/mmdit.py:821-832 and the fused
// linear1 / linear2 of the single-stream blocks (:693-751).
//
// Why (NOTES_r03 open item 1): in the 8-wave frame of gemm256v3.hip a wave holds 128 accumulators and re-reads its
// fragments from LDS for every 32 MFMAs; the lone wave of this frame reads a whole K = 32 slice of BOTH operands (64 registers) one
// slice ahead of the 64 MFMAs that use it -- a third fewer LDS reads per MAC, one non-MFMA instruction between two MFMAs, and each
// operand's ring slot is released by its own barrier as soon as its second slice has been read, so the LDS-DMA pieces of K-tile i + 2
// have 1.25 - 1.5 K-tiles to land in a TWO-slot ring (128 KiB, the rest of the LDS stays free).  The schedule follows the shape of the
// vendor library's MT256x256x64 kernel as read from its disassembly (profiles/NOTES_r05.md); nothing of it is linked or copied.
//
// Shapes: N % 256 == 0, K % 64 == 0, any M, any row-segment maps; no K split, no half tiles, no convolution form (gemm256v3.hip keeps
// those).  C / D layout as in gemm256v3.hip: lane holds row m = mf*16 + (lane & 15), columns n = nf*16 + 4*(lane >> 4) + {0..3}.
//
// Tail: the asm block leaves round_bf16(alpha * acc + bias) in the LDS image gemm256v3.hip's tail stages (eight wave-private 16 KiB
// regions; a wave of this kernel owns two of them), so the read-back is the one all three 256 x 256 kernels share (dk_gemm_tail.h): 8 columns
// per lane, one 16-byte store per lane and row, epilogues folded at compile time.  The fused QKNorm + RoPE of key / query tiles takes its
// row sums from the staged image (a wave's 128 columns hold whole heads: no exchange between waves).
#include <cstring>
#include <type_traits>

#include "dk_kernels.h"
#include "dk_gemm_tail.h"

#define V4_T 256
#define V4_BK 64
#define V4_LDS_BYTES (4 * 32768)

typedef __attribute__((address_space(3))) char v4_lds_char;
typedef unsigned int u32x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

// position of block `bid` inside the XCD-contiguous order of `count` blocks (hardware places block b on XCD b & 7)
__device__ __forceinline__ int v4_xcd_contiguous(int bid, int count) {
  const int x = bid & 7;
  int start = 0;
  for (int y = 0; y < x; ++y) start += y < count ? (count - y + 7) >> 3 : 0;
  return start + (bid >> 3);
}

#ifndef V4_NT
#define V4_NT 0  // lab: cache policy of the C stores -- 0 plain (L2 write-back), 1 non-temporal (nt), 2 write-through to memory (sc0 sc1)
#endif
__device__ __forceinline__ void v4_store16(bf16_t* ptr, u32x4 v) {
#if V4_NT == 1
  __builtin_nontemporal_store(v, (u32x4*)ptr);
#elif V4_NT == 2
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(ptr), "v"(v) : "memory");
#else
  *(u32x4*)ptr = v;
#endif
}

// read-back of the staged tile: the shared row loop (dk_gemm_tail.h) in this kernel's frame -- a wave owns a 128 x 128 block of the tile, two of
// the 16 KiB image regions of each of its two row halves: four 32-column passes, every load of all four in front of the first store (a lone
// wave has nothing else to cover a memory round trip).  FAST / EK / KF / CUT: see dk_tail_rows
template <bool FAST, int EK, bool KF, int MF, bool CUT = false, class P>
__device__ __forceinline__ void v4_rows(const P& p, const DkTailTile& tile, int wm, int wn2, int lane) {
  DkTailTile t = tile;
  dk_tail_first_rows<EK>(p, t);
  // KF: sum of squares of every row over its head's columns, from the staged (bf16-rounded) values: this lane's 8 rows, per head
  // (kn_D = 128: the wave's 128 columns are one head; 64: two heads = the two virtual waves).  This order of summation is this kernel's own:
  // gemm256v3.hip sums the accumulators (dk_tail_sumsq_exchange), so key tiles of the two agree within rounding, not bit for bit
  float ss[2][MF];
  if (KF) {
#pragma unroll
    for (int vwn = 0; vwn < 2; ++vwn) {
#pragma unroll
      for (int itr = 0; itr < MF; ++itr) ss[vwn][itr] = 0.f;
      for (int ni = 0; ni < 2; ++ni) {
        const unsigned reg0 = (unsigned)((wm * 4 + 2 * wn2 + vwn) * 16384 + ni * 8192);
#pragma unroll
        for (int itr = 0; itr < MF; ++itr) {
          const u32x4 sv = dk_tail_read(reg0, itr * 16 + (lane >> 2), lane & 3);
          float vv[8];
          dk_tail_unpack8(make_uint4(sv[0], sv[1], sv[2], sv[3]), vv);
#pragma unroll
          for (int e = 0; e < 8; ++e) ss[vwn][itr] += vv[e] * vv[e];
        }
      }
#pragma unroll
      for (int itr = 0; itr < MF; ++itr) {
        ss[vwn][itr] += __shfl_xor(ss[vwn][itr], 1, 64);
        ss[vwn][itr] += __shfl_xor(ss[vwn][itr], 2, 64);
      }
    }
    if (p.kn_D == 128) {
#pragma unroll
      for (int itr = 0; itr < MF; ++itr) ss[0][itr] = ss[1][itr] = ss[0][itr] + ss[1][itr];
    }
  }
  auto pass_of = [&](int pass) {
    const int wn = 2 * wn2 + (pass >> 1), ni = pass & 1;
    return DkTailPass{(unsigned)((wm * 4 + wn) * 16384 + ni * 8192), wn * 64 + ni * 32};
  };
  auto ss_of = [&](int pass, int itr, int) { return ss[pass >> 1][itr]; };
  auto store_raw = [&](size_t crow, int ocol, bool ok, u32x4 sv) {
    if (ok) v4_store16(t.Cb + crow * (size_t)t.ldcb + ocol, sv);
  };
  auto store = [&](int, size_t crow, int ocol, bool ok, const float* vv) {
    const uint4 o4 = dk_tail_pack8(vv);
    store_raw(crow, ocol, ok, u32x4{o4.x, o4.y, o4.z, o4.w});
  };
  dk_tail_rows<FAST, EK, KF, MF, CUT, 4, true>(p, t, lane, pass_of, ss_of, store, store_raw);
}

// MF: 16-row activation fragments per wave: 8 = 256-row tiles, 7 = 224-row tiles (the launcher takes the height with the fewest rounds x height,
// gemm256v3.hip's rule: 4352 rows x 12 column tiles are 204 tiles of 256 rows -- 80 % of the CUs -- or 240 of 224)
template <int MF>
__global__ __launch_bounds__(256, 1) void dk_gemm256v4_kernel(GemmParams pa, GemmParams pb, int tiles_a, int tiles_b, int skew) {
  constexpr int BM = 32 * MF, HROWS = 16 * MF;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if ((unsigned)(size_t)(v4_lds_char*)smem != 0u) __builtin_trap();  // the LDS image is addressed from 0
  // Start skew (multi-round launches): the first round's workgroups start up to `skew` x 0.25 us apart (by their position inside their
  // XCD), and every later round inherits the spread -- without it all 256 CUs reach their tails at the same moment and 256 x 128 KiB of
  // C leave in one burst per round while the matrix pipes idle (profiles/r03_gemm_k_sweep_ablations.log: 2.4 us of a 9.8 us fixed cost)
  if (skew > 0 && blockIdx.x < 256) {
    const int n = (int)((blockIdx.x >> 3) & 31) * skew / 32;
    for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(8);
  }
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn2 = wave & 1;
  const int l15 = lane & 15, q = lane >> 4;

  const int tile = v4_xcd_contiguous(blockIdx.x, tiles_a + tiles_b);
  const bool second = tile >= tiles_a;
  // one scalar base into the kernel-argument segment for this tile's parameter block (gemm256v3.hip, round 4)
  static_assert(sizeof(GemmParams) % 8 == 0 && alignof(GemmParams) == 8, "pb follows pa without padding");
  typedef const __attribute__((address_space(4))) GemmParams karg_params_t;
  const __attribute__((address_space(4))) char* kbase = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
  karg_params_t& p = *(karg_params_t*)(kbase + (second ? sizeof(GemmParams) : 0));
  const int tl = second ? tile - tiles_a : tile;
  const int nbm = (p.M + BM - 1) / BM, nbn = p.N / V4_T;
  const int GROUP = 4;
  const int tpg = GROUP * nbn;
  const int g = tl / tpg;
  const int first_m = g * GROUP;
  const int gsz = min(nbm - first_m, GROUP);
  const int tm = first_m + (tl % tpg) % gsz;
  const int tn = (tl % tpg) / gsz;
  const int m0 = tm * BM, n0 = tn * V4_T;

  // ---- DMA piece offsets: piece gg of a wave covers rows hh*128 + (wave*2 + u)*16 + j*8 + (lane >> 3) of the operand's 256-row K-tile,
  // 16-byte chunk (lane & 7) of LDS row r holds global chunk (lane & 7) ^ ((r >> 1) & 7) (conflict-free ds_read_b128, gemm256v3.hip)
  const int srow = lane >> 3;
  u32x8 voX, voW;
  // (a tile that lies inside one row segment -- every tile of the image stream -- maps its rows with one scalar division instead of eight
  //  per lane: the integer divisions were ~ 0.4 us in front of the first DMA piece of every tile)
  const int a_seg0 = m0 / p.a_seg_len;
  const bool a_uniform = min(m0 + BM - 1, p.M - 1) / p.a_seg_len == a_seg0;
  const int a_base = a_seg0 * p.a_seg_stride - a_seg0 * p.a_seg_len;
#pragma unroll
  for (int gg = 0; gg < 8; ++gg) {
    const int hh = gg & 1, j = (gg >> 1) & 1, u = gg >> 2;
    const int rih = (wave * 2 + u) * 16 + j * 8 + srow;  // row inside the 128-row LDS half
    const int row = hh * 128 + rih;
    const int chunk = (lane & 7) ^ (srow >> 1) ^ (4 * j);
    // rows beyond M - 1 re-read the last row, their results are never stored; MF = 7: LDS rows 112 .. 127 of a half hold duplicates nobody reads
    voX[gg] = (unsigned)min(m0 + hh * HROWS + min(rih, HROWS - 1), p.M - 1);
    voW[gg] = ((unsigned)row * (unsigned)p.ldw + chunk * 8) * 2u;
  }
  if (a_uniform) {  // (a scalar branch: the divisions below are not executed)
#pragma unroll
    for (int gg = 0; gg < 8; ++gg) voX[gg] += (unsigned)a_base;
  } else {
#pragma unroll
    for (int gg = 0; gg < 8; ++gg) voX[gg] = (unsigned)(((int)voX[gg] / p.a_seg_len) * p.a_seg_stride + ((int)voX[gg] % p.a_seg_len));
  }
#pragma unroll
  for (int gg = 0; gg < 8; ++gg) {
    const int j = (gg >> 1) & 1;
    const int chunk = (lane & 7) ^ (srow >> 1) ^ (4 * j);
    voX[gg] = (voX[gg] * (unsigned)p.lda + chunk * 8) * 2u;
  }
  // fragment read addresses (X kk0, X kk1, W kk0, W kk1) and the two drain addresses
  u32x4 rd;
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const unsigned offk = (unsigned)(l15 * 128 + (((kk * 4 + q) ^ (l15 >> 1)) << 4));
    rd[kk] = wm * 16384 + offk;
    rd[2 + kk] = 65536 + wn2 * 16384 + offk;
  }
  u32x2 dr;
  dr[0] = (unsigned)((wm * 4 + 2 * wn2) * 16384) + dk_tail_stage_off(l15, 0, q);
  dr[1] = dr[0] ^ 32u;
  // bias of this lane's 32 columns (4 per 16-column fragment)
  f32x8 bq[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) bq[i][e] = 0.f;
  if (p.bias) {
#pragma unroll
    for (int nf8 = 0; nf8 < 8; ++nf8) {
      const u32x2 b2 = *(const u32x2*)(p.bias + n0 + wn2 * 128 + nf8 * 16 + 4 * q);
      float b0, b1, b2f, b3;
      unpack2bf(b2[0], b0, b1);
      unpack2bf(b2[1], b2f, b3);
      bq[nf8 >> 1][(nf8 & 1) * 4 + 0] = b0;
      bq[nf8 >> 1][(nf8 & 1) * 4 + 1] = b1;
      bq[nf8 >> 1][(nf8 & 1) * 4 + 2] = b2f;
      bq[nf8 >> 1][(nf8 & 1) * 4 + 3] = b3;
    }
  }
  const char* gA = (const char*)p.A;
  const char* gW = (const char*)p.W + (size_t)n0 * (size_t)p.ldw * 2;
  const u32x4 rX = {(unsigned)(size_t)gA, (unsigned)((size_t)gA >> 32) & 0xffffu, 0xffffffffu, 0x00020000u};
  const u32x4 rW = {(unsigned)(size_t)gW, (unsigned)((size_t)gW >> 32) & 0xffffu, 0xffffffffu, 0x00020000u};
  const int nk = p.K / V4_BK;
  const float alpha = p.alpha;

#ifdef V4_TRACE  // lab (scripts/build_lab.sh TRACE=1): time stamps of workgroups 0 and gridDim.x - 1, wave 0, into p.workspace
  unsigned long long t_entry = __builtin_readcyclecounter(), ts0, ts1, ts2, ts3;
  asm volatile(
#include "../../profiles/lab_kernels/gemm256v4_variants/gemm256v4_asm_trace.inc"
      : "={s[74:75]}"(ts0), "={s[76:77]}"(ts1), "={s[78:79]}"(ts2), "={s[80:81]}"(ts3)
      : [koff] "s"(0), [nk] "s"(nk), [dstx] "s"(wave * 4096), [alpha] "s"(alpha), [wave] "s"(wave), "{v[0:7]}"(voX), "{v[8:15]}"(voW), "{v[16:19]}"(rd),
        "{v[24:25]}"(dr), "{v[160:167]}"(bq[0]), "{v[168:175]}"(bq[1]), "{v[176:183]}"(bq[2]), "{v[184:191]}"(bq[3]), "{s[60:63]}"(rX), "{s[64:67]}"(rW)
      :
#include "gemm256v4_clobbers.inc"
  );
#else
  if constexpr (MF == 7) {
    asm volatile(
#include "gemm256v4_asm7.inc"
        :
        : [koff] "s"(0), [nk] "s"(nk), [dstx] "s"(wave * 4096), [alpha] "s"(alpha), [wave] "s"(wave), "{v[0:7]}"(voX), "{v[8:15]}"(voW), "{v[16:19]}"(rd),
          "{v[24:25]}"(dr), "{v[160:167]}"(bq[0]), "{v[168:175]}"(bq[1]), "{v[176:183]}"(bq[2]), "{v[184:191]}"(bq[3]), "{s[60:63]}"(rX), "{s[64:67]}"(rW)
        :
#include "gemm256v4_clobbers.inc"
    );
  } else
  asm volatile(
#include "gemm256v4_asm.inc"
      :
      : [koff] "s"(0), [nk] "s"(nk), [dstx] "s"(wave * 4096), [alpha] "s"(alpha), [wave] "s"(wave), "{v[0:7]}"(voX), "{v[8:15]}"(voW), "{v[16:19]}"(rd),
        "{v[24:25]}"(dr), "{v[160:167]}"(bq[0]), "{v[168:175]}"(bq[1]), "{v[176:183]}"(bq[2]), "{v[184:191]}"(bq[3]), "{s[60:63]}"(rX), "{s[64:67]}"(rW)
      :
#include "gemm256v4_clobbers.inc"
  );
#endif

  // ---------------- tail: staged bf16 image -> row-major, epilogues on the way ----------------
  const DkTailTile t = dk_tail_tile<true>(p, m0, n0, BM, wm * HROWS, p.M, p.ldc, p.c_seg_len, p.ldr);
  const bool fast = t.fast, cut = t.cut;
  if (t.kfuse) {  // (bias-only epilogue -- checked by the launcher)
    if (fast) v4_rows<true, DK_EPI_BIAS, true, MF>(p, t, wm, wn2, lane);
    else if (cut) v4_rows<true, DK_EPI_BIAS, true, MF, true>(p, t, wm, wn2, lane);
    else v4_rows<false, DK_EPI_BIAS, true, MF>(p, t, wm, wn2, lane);
  } else if (cut) {
    if (t.epi == DK_EPI_BIAS) v4_rows<true, DK_EPI_BIAS, false, MF, true>(p, t, wm, wn2, lane);
    else if (t.epi == DK_EPI_BIAS_GELU) v4_rows<true, DK_EPI_BIAS_GELU, false, MF, true>(p, t, wm, wn2, lane);
    else if (t.epi == DK_EPI_GATE_RES) v4_rows<true, DK_EPI_GATE_RES, false, MF, true>(p, t, wm, wn2, lane);
    else v4_rows<false, -1, false, MF>(p, t, wm, wn2, lane);
  } else if (fast) {
    if (t.epi == DK_EPI_BIAS) v4_rows<true, DK_EPI_BIAS, false, MF>(p, t, wm, wn2, lane);
    else if (t.epi == DK_EPI_BIAS_GELU) v4_rows<true, DK_EPI_BIAS_GELU, false, MF>(p, t, wm, wn2, lane);
    else if (t.epi == DK_EPI_GATE_RES) v4_rows<true, DK_EPI_GATE_RES, false, MF>(p, t, wm, wn2, lane);
    else if (t.epi == DK_EPI_RES) v4_rows<true, DK_EPI_RES, false, MF>(p, t, wm, wn2, lane);
    else v4_rows<true, -1, false, MF>(p, t, wm, wn2, lane);
  } else {
    v4_rows<false, -1, false, MF>(p, t, wm, wn2, lane);
  }
#ifdef V4_TRACE
  if (p.workspace != nullptr && wave == 0 && lane == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x - 1)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the tail's stores have left)
    unsigned long long* o = (unsigned long long*)p.workspace + (blockIdx.x == 0 ? 0 : 8);
    o[0] = t_entry; o[1] = ts0; o[2] = ts1; o[3] = ts2; o[4] = ts3; o[5] = __builtin_readcyclecounter();
  }
#endif
}

int g_dk_v4_skew = -1;  // dk_tune_set("gemm_skew", v): start skew of multi-round launches in 0.25 us steps; -1 (default): none

// dk_tune_set("gemm", 10) forces this kernel on every shape it accepts; -1 (automatic): see dk_gemm_route (gemm.hip)
bool dk_gemm256v4_eligible(const GemmParams& p) {
  if (p.conv || !dk_gemm256v3_eligible(p)) return false;
  if (p.N % 256 != 0) return false;
  // 32-bit byte offsets of the W pieces: 255 rows
  return (size_t)p.ldw * 2 * 256 < (1ull << 31);
}

// tile height and tiles as routed (dk_gemm_route: gemm256v3.hip's height rule, 256-row tiles where 224-row ones would straddle a row segment)
int dk_launch_gemm256v4(const GemmParams& p, const GemmParams* p2, const GemmRoute& r, hipStream_t stream) {
  static DkDeviceOnce attr_once;
  if (attr_once.first()) {
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_gemm256v4_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize, V4_LDS_BYTES));
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_gemm256v4_kernel<7>, hipFuncAttributeMaxDynamicSharedMemorySize, V4_LDS_BYTES));
    attr_once.mark();
  }
  double work = 2.0 * (double)p.M * (double)p.N * (double)p.K;
  if (p2) work += 2.0 * (double)p2->M * (double)p2->N * (double)p2->K;
  dk_prof_begin(0, work, stream);
  // ... in the lab with warm weights.  Inside the model (weights from HBM) the start skew is flat: 58.78 / 58.81 against 58.86 / 58.94 ms per FLUX
  // step (profiles/r05_gemm_v4_start_skew.log) -- the automatic choice keeps it off; dk_tune_set("gemm_skew", n) turns it on
  const int tiles = r.tiles_a + r.tiles_b;
  const int skew = tiles <= r.n_cu || g_dk_v4_skew < 0 ? 0 : g_dk_v4_skew;
  if (r.tile_rows == 224)
    hipLaunchKernelGGL(dk_gemm256v4_kernel<7>, dim3(tiles), dim3(256), V4_LDS_BYTES, stream, p, p2 ? *p2 : p, r.tiles_a, r.tiles_b, skew);
  else
    hipLaunchKernelGGL(dk_gemm256v4_kernel<8>, dim3(tiles), dim3(256), V4_LDS_BYTES, stream, p, p2 ? *p2 : p, r.tiles_a, r.tiles_b, skew);
  dk_prof_end(stream);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}
