// Producers of MX-fp6 activations for the W4A6 GEMM (gemm256f4a6.hip): OCP E2M3 elements with one E8M0 scale per row and 32 consecutive
// columns -- the siblings of fp8_ops.hip's two producers, whose row jobs, memory schedule, fused LayerNorm-modulate and fp32 statistics these
// repeat statement for statement.  What differs is the last step:
//   format   weights.py: quantize_activation_mxfp6 is the definition; dk_mx6_quantize8 below is held to it bit for bit.  The scale is
//            dk_mx8_quantize8's with 7.5 in the place of 448; a block that holds an Inf or a NaN leaves as scale byte 0xFF and codes 0.
//   packing  a lane's 8 rounded codes are 48 bits (shifts and ORs); the 4 lanes of a quad hold the 24 bytes of one (row, 32-K block), which is
//            exactly one MFMA lane's operand (profiles/mxfp6_probe.log: element e in bits [6 e, 6 e + 6) of registers 0 .. 5, lane (r, q) =
//            row r, K [32 q, +32) of the K-tile).  Eight quad broadcasts (DPP) collect them; lane 0 of the quad stores registers 0 .. 3 with one
//            16-byte store, lane 1 registers 4, 5 with one 8-byte store.
//   order    fragment order, the mirror of pack_mxfp4 (weights.py: pack_activation_mxfp6): 16 rows = one fragment row of 16 * ldo bytes; K-tile t of
//            it = 1536 bytes: the 16-byte parts of the 64 MFMA lanes at (q * 16 + r) * 16, then their 8-byte parts at 1024 + (q * 16 + r) * 8.
//            The GEMM copies a fragment with linear LDS-DMA and reads a lane's operand with one aligned b128 and one aligned b64 LDS read.
//   pad      the rows behind the last one, up to a whole group of 16, are written as zeros (no scale bytes): the GEMM never predicates its loads.
// Scale bytes go to the dk_mx_scale_index side array of the MX-fp8 buffers: it already is the GEMM's order for this side -- a wave's 128 rows of a
// K-tile are 512 contiguous bytes, lane (r, q) gets the bytes of its eight 16-row fragments.
#include "dk_kernels.h"

struct Mx6Job {
  const bf16_t* x;
  const bf16_t *shift, *scale;  // null: plain quantisation (no LayerNorm)
  int ldx, M, mod_stride, seg_len, x_seg_len, x_seg_stride;
  Mx8Out o;
};

// maximum over the 4 lanes of a quad of a non-negative float's bit pattern (monotonic, and Inf / NaN patterns stay on top: fmaxf would drop a NaN)
__device__ __forceinline__ unsigned dk_quad_umax(unsigned v) {
  v = max(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));  // quad_perm [1,0,3,2]
  return max(v, (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));  // quad_perm [2,3,0,1]
}
// Quantise the 8 values this lane holds of a 32-element block shared by 4 ADJACENT lanes: the 8 E2M3 codes as 48 bits (lo: bits 0 .. 31, hi: bits
// 32 .. 47, element 0 in the low bits) and the block's E8M0 byte.  Rounding: |v| * 2^(127 - e) <= 7.5 (1 + 2^-23) is exact; adding and subtracting
// 1.5 * 2^(23 - s) rounds it to nearest even on multiples of 2^-s, s = 3 below 2 (subnormals and the first binade share the step), 2 below 4, 1 above;
// a carry into the next binade lands on a grid point; above 7.5 saturates.
__device__ __forceinline__ void dk_mx6_quantize8(const float* v, unsigned& lo, unsigned& hi, unsigned& e8m0) {
  unsigned am = 0u;
#pragma unroll
  for (int e = 0; e < 8; ++e) am = max(am, __float_as_uint(v[e]) & 0x7FFFFFFFu);
  am = dk_quad_umax(am);
  const bool bad = am >= 0x7F800000u;
  const float t = __uint_as_float(am) * __uint_as_float(0x3E088889u);  // fp32(1 / 7.5), the host's constant
  unsigned e = (__float_as_uint(t) + 0x7FFFFFu) >> 23;                 // ceil(log2 t) + 127
  e = e < 1u ? 1u : (e > 254u ? 254u : e);
  const float inv = __uint_as_float((254u - e) << 23);  // 2^(127 - e); e = 254: 0, every element becomes 0
  unsigned long long bits = 0ull;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float a = fminf(fabsf(v[i]) * inv, 8.0f);
    const float magic = a < 2.0f ? 1572864.0f : (a < 4.0f ? 3145728.0f : 6291456.0f);
    float r = a + magic;
    asm volatile("" : "+v"(r));  // (the sum must round to fp32 before the difference)
    r = fminf(r - magic, 7.5f);
    unsigned code = r < 1.0f ? (unsigned)(r * 8.0f) : (__float_as_uint(r) >> 20) - (126u << 3);
    code |= (v[i] < 0.f && code != 0u) ? 32u : 0u;
    bits |= (unsigned long long)(bad ? 0u : code) << (6 * i);
  }
  lo = (unsigned)bits;
  hi = (unsigned)(bits >> 32);
  e8m0 = bad ? 255u : e;
}

static_assert(sizeof(Mx6Job) % 8 == 0 && alignof(Mx6Job) == 8, "job b follows job a without padding in the kernarg segment");
template <int NCH, bool LN>
__global__ __launch_bounds__(256) void dk_rows_to_mx6_kernel(Mx6Job ja, Mx6Job jb, int blocks_a, int h, float eps) {
  const bool first = (int)blockIdx.x < blocks_a;
  typedef const __attribute__((address_space(4))) Mx6Job karg_job_t;  // one scalar base pointer, see gemm256v3.hip
  const __attribute__((address_space(4))) char* kbase = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
  karg_job_t& j = *(karg_job_t*)(kbase + (first ? 0 : sizeof(Mx6Job)));
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = ((int)blockIdx.x - (first ? 0 : blocks_a)) * 4 + wave;
  const int j_M = j.M;
  if (m >= ((j_M + 15) & ~15)) return;
  const bool pad = m >= j_M;       // a row behind the last one: zeros
  const int mm = pad ? j_M - 1 : m;
  const size_t xrow = (size_t)((mm / j.x_seg_len) * j.x_seg_stride + (mm % j.x_seg_len)) * j.ldx;
  const int nchunks = h >> 3;  // a multiple of 16: every quad of lanes holds whole 32-element blocks, every 16 lanes whole K-tiles
  const int xbytes = pad ? 0 : h * 2;  // (a pad row reads nothing: every load returns zeros)
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(j.x + xrow), 0, xbytes, 0x00020000);
  u32x4 raw[NCH], rs[NCH], rc[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) raw[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, (lane + 64 * i) * 16, 0, 0);
  if (LN) {
    const size_t mod = (size_t)(mm / j.seg_len) * j.mod_stride;
    const __amdgpu_buffer_rsrc_t rsh = __builtin_amdgcn_make_buffer_rsrc((void*)(j.shift + mod), 0, xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsc = __builtin_amdgcn_make_buffer_rsrc((void*)(j.scale + mod), 0, xbytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      rs[i] = __builtin_amdgcn_raw_buffer_load_b128(rsh, (lane + 64 * i) * 16, 0, 0);
      rc[i] = __builtin_amdgcn_raw_buffer_load_b128(rsc, (lane + 64 * i) * 16, 0, 0);
    }
  }
  __builtin_amdgcn_sched_barrier(0);  // (keeps the shift / scale loads above the reductions)
  float mean = 0.f, rstd = 0.f;
  if (LN) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v0, v1;
        unpack2bf(raw[i][e], v0, v1);
        sum += v0 + v1;  // (zeros past the row end)
      }
    }
    mean = wave_sum(sum) / (float)h;
    __builtin_amdgcn_sched_barrier(0);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const bool live = lane + 64 * i < nchunks;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v0, v1;
        asm volatile("" : "+v"(raw[i][e]));  // (opaque: the unpacked row of the first pass must not stay live)
        unpack2bf(raw[i][e], v0, v1);
        const float d0 = live ? v0 - mean : 0.f, d1 = live ? v1 - mean : 0.f;
        sq += d0 * d0;
        sq += d1 * d1;
      }
    }
    rstd = rsqrtf(wave_sum(sq) / (float)h + eps);
  }
  const unsigned orow = (unsigned)(j.o.row0 + (mm / j.o.seg_len) * j.o.seg_stride + (mm % j.o.seg_len) + (m - mm));
  const unsigned col0 = (unsigned)j.o.col0, n_blk128 = (unsigned)j.o.n_blk128;
  unsigned char* __restrict__ scales = j.o.scales;
  // K-tile 0 of this row's fragment row
  unsigned char* __restrict__ frow = j.o.out + (size_t)(orow >> 4) * 16u * (size_t)j.o.ldo + (size_t)(col0 >> 7) * 1536u;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    __builtin_amdgcn_sched_barrier(0);
    const int c = lane + 64 * i;  // (the exchanges below run for every lane of the wave: no divergence above them)
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (LN) asm volatile("" : "+v"(raw[i][e]));
      unpack2bf(raw[i][e], v[2 * e], v[2 * e + 1]);
      if (LN) {
        float s0, s1, c0, c1;
        unpack2bf(rs[i][e], s0, s1);
        unpack2bf(rc[i][e], c0, c1);
        // the bf16 value dk_ln_modulate_kernel would have stored (same expression, same rounding), then quantised
        v[2 * e] = pad ? 0.f : round_bf16((v[2 * e] - mean) * rstd * round_bf16(1.0f + c0) + s0);
        v[2 * e + 1] = pad ? 0.f : round_bf16((v[2 * e + 1] - mean) * rstd * round_bf16(1.0f + c1) + s1);
      }
    }
    unsigned lo, hi, e8;
    dk_mx6_quantize8(v, lo, hi, e8);
    // the quad's four 48-bit pieces -> the block's six registers
#define MX6_QUAD(V, S) (unsigned)__builtin_amdgcn_update_dpp(0, (int)(V), (S) * 0x55, 0xF, 0xF, false)  // quad_perm [S,S,S,S]
    const unsigned L[4] = {MX6_QUAD(lo, 0), MX6_QUAD(lo, 1), MX6_QUAD(lo, 2), MX6_QUAD(lo, 3)};
    const unsigned H[4] = {MX6_QUAD(hi, 0), MX6_QUAD(hi, 1), MX6_QUAD(hi, 2), MX6_QUAD(hi, 3)};
#undef MX6_QUAD
    const int kb = c >> 2;  // 32-K block of the row: K-tile kb >> 2, MFMA lane (orow & 15, kb & 3) of it
    unsigned char* frag = frow + (size_t)(kb >> 2) * 1536u;
    const unsigned ml = (unsigned)(kb & 3) * 16u + (orow & 15u);
    if (c < nchunks && (lane & 3) == 0) {
      *(u32x4*)(frag + ml * 16u) = u32x4{L[0], H[0] | (L[1] << 16), (L[1] >> 16) | (H[1] << 16), L[2]};
      if (!pad) scales[dk_mx_scale_index(orow, (col0 >> 5) + (unsigned)kb, n_blk128)] = (unsigned char)e8;
    }
    if (c < nchunks && (lane & 3) == 1) *(u32x2*)(frag + 1024u + ml * 8u) = u32x2{H[2] | (L[3] << 16), (L[3] >> 16) | (H[3] << 16)};
  }
}

static int launch_mx6_jobs(const Mx6Job& a, const Mx6Job& b, int h, float eps, bool ln, hipStream_t stream) {
  DK_REQUIRE(h % 128 == 0 && h <= 4096, "row length must be a multiple of 128 (one K-tile of the W4A6 GEMM) and <= 4096");
  for (const Mx6Job* j : {&a, &b}) {
    if (j->M == 0) continue;
    DK_REQUIRE(j->x && j->o.out && j->o.scales, "null pointer");
    DK_REQUIRE(j->ldx % 8 == 0 && (!ln || j->mod_stride % 8 == 0), "bf16 strides must keep 16-byte alignment");
    DK_REQUIRE(j->o.ldo % 96 == 0 && j->o.col0 % 128 == 0 && (j->o.col0 + h) / 128 * 96 <= j->o.ldo && ((uintptr_t)j->o.out & 15) == 0,
               "fp6 output: pitch a multiple of 96 bytes (whole K-tiles), column offset a multiple of 128, 16-byte aligned");
    DK_REQUIRE(j->o.seg_len > 0 && j->x_seg_len > 0 && (!ln || j->seg_len > 0), "segment lengths must be positive");
    DK_REQUIRE(j->o.row0 % 16 == 0 && (j->M <= j->o.seg_len || (j->o.seg_len % 16 == 0 && j->o.seg_stride % 16 == 0)),
               "fp6 output: row ranges start on 16-row fragment rows");
    const long last = (long)j->o.row0 + (long)((j->M - 1) / j->o.seg_len) * j->o.seg_stride + (j->M - 1) % j->o.seg_len;
    DK_REQUIRE(last < (long)j->o.n_blk128 * 128, "fp6 output rows exceed the scale array");
  }
  const int blocks_a = ((a.M + 15) / 16 * 16) / 4, blocks_b = ((b.M + 15) / 16 * 16) / 4;
  dim3 grid(blocks_a + blocks_b), block(256);
  const int nch = (h / 8 + 63) / 64;
#define MX_CASE(N)                                                                                                   \
  case N:                                                                                                            \
    if (ln) hipLaunchKernelGGL((dk_rows_to_mx6_kernel<N, true>), grid, block, 0, stream, a, b, blocks_a, h, eps);    \
    else hipLaunchKernelGGL((dk_rows_to_mx6_kernel<N, false>), grid, block, 0, stream, a, b, blocks_a, h, eps);      \
    break;
  switch (nch) {
    MX_CASE(1) MX_CASE(2) MX_CASE(3) MX_CASE(4) MX_CASE(5) MX_CASE(6) MX_CASE(7) MX_CASE(8)
    default: DK_REQUIRE(false, "unsupported row length");
  }
#undef MX_CASE
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}

static Mx6Job mx6_job(const bf16_t* x, int ldx, int M, const bf16_t* shift, const bf16_t* scale, int mod_stride, int seg_len, int x_seg_len,
                      int x_seg_stride, const Mx8Out& o) {
  Mx6Job j;
  j.x = x; j.shift = shift; j.scale = scale; j.ldx = ldx; j.M = M; j.mod_stride = mod_stride; j.seg_len = seg_len;
  j.x_seg_len = x_seg_len; j.x_seg_stride = x_seg_stride; j.o = o;
  return j;
}
static Mx6Job mx6_none() {
  Mx8Out o;
  o.out = nullptr; o.scales = nullptr; o.ldo = 96; o.n_blk128 = 1; o.row0 = 0; o.seg_len = 1; o.seg_stride = 0; o.col0 = 0;
  return mx6_job(nullptr, 8, 0, nullptr, nullptr, 8, 1, 1, 0, o);
}

int dk_launch_quantize_mx6(const bf16_t* x, int ldx, int x_seg_len, int x_seg_stride, int M, int h, const Mx8Out& o, hipStream_t stream) {
  return launch_mx6_jobs(mx6_job(x, ldx, M, nullptr, nullptr, 8, 1, x_seg_len > 0 ? x_seg_len : M, x_seg_stride, o), mx6_none(), h, 0.f, false, stream);
}
// two row sets in one launch: the image and the text rows of a double block (the engine's pair, as dk_launch_ln_modulate2_mx8)
int dk_launch_ln_modulate2_mx6(const bf16_t* x0, int M0, const bf16_t* shift0, const bf16_t* scale0, int seg0, const Mx8Out& o0,
                               const bf16_t* x1, int M1, const bf16_t* shift1, const bf16_t* scale1, int seg1, const Mx8Out& o1, int ldx, int h,
                               int mod_stride, int x_seg_stride, float eps, hipStream_t stream) {
  DK_REQUIRE(shift0 && scale0 && shift1 && scale1, "shift / scale missing");
  return launch_mx6_jobs(mx6_job(x0, ldx, M0, shift0, scale0, mod_stride, seg0, seg0, x_seg_stride, o0),
                         mx6_job(x1, ldx, M1, shift1, scale1, mod_stride, seg1, seg1, x_seg_stride, o1), h, eps, true, stream);
}
int dk_launch_ln_modulate_mx6(const bf16_t* x, int ldx, int M, int h, const bf16_t* shift, const bf16_t* scale, int mod_stride, int seg_len,
                              int x_seg_len, int x_seg_stride, float eps, const Mx8Out& o, hipStream_t stream) {
  DK_REQUIRE(shift && scale, "shift / scale missing");
  return launch_mx6_jobs(mx6_job(x, ldx, M, shift, scale, mod_stride, seg_len, x_seg_len, x_seg_stride, o), mx6_none(), h, eps, true, stream);
}
