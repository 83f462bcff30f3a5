// HBM-bound kernels of the MMDiT step: adaptive LayerNorm modulation, per-head QK-RMSNorm + RoPE,
// timestep embedding / modulation-vector prep, RoPE table, patchify, and the fused
// x0-prediction + CFG + Euler update.  All bf16 traffic is moved as 16-byte vectors.
#include "dk_kernels.h"

// ---------------------------------------------------------------------------------------------
// AdaLN modulation: out = bf16( LN(x) * bf16(1 + scale[b]) + shift[b] )
// reference: affine_transform, python/src/diffusionkit/mlx/mmdit.py:958-972 (fused batch-1 form:
// mx.fast.layer_norm(x, 1 + scale, shift, eps)); LayerNorm :838-849 (no affine, eps 1e-6).
// One wave per row, row kept in registers (two-pass variance), 4 rows per workgroup.
// ---------------------------------------------------------------------------------------------
// One launch serves up to two jobs (the image and the text stream of a double block, mmdit.py:568-675: the text
// stream's 256 rows would otherwise run alone on the chip): blocks [0, blocks_a) belong to job a, the rest to job b.
struct LnJob {
  const bf16_t* x;
  bf16_t* out;
  const bf16_t *shift, *scale;
  int ldx, ldo, M, mod_stride, seg_len, x_seg_len, x_seg_stride;
};
// Every load of the row -- its NCH chunks, then the shift and scale chunks -- is issued unconditionally and back to back before
// the first use: one memory round trip per wave.  Guarding each chunk with `if (c < nchunks)` compiled to branch / load /
// s_waitcnt vmcnt(0) per chunk, twelve dependent round trips at h = 3072.  The loads and the store are buffer instructions
// whose resource spans exactly one row (h * 2 bytes from a scalar row base): lanes past the row end read zeros and their stores
// are dropped, one 32-bit offset register serves all three arrays, and the row stays in its packed bf16 form (unpacked again
// in each pass) so the kernel holds 12 * NCH data registers.
static_assert(sizeof(LnJob) % 8 == 0 && alignof(LnJob) == 8, "job b follows job a without padding in the kernarg segment");
// DUAL (MMDiT-X, the image stream of a dual-attention block): a job carries a second (shift, scale, out) triple, and the row -- loaded and
// reduced once -- leaves twice, out2 = bf16( LN(x) * bf16(1 + scale2[b]) + shift2[b] ) from the same registers with the same expression and
// rounding.  A job without one (the text stream riding in the same launch) has out2 null and shift2 / scale2 = its first pair: the loads
// stay unconditional, the second store is skipped on a wave-uniform test.  The plain instantiations do not see any of this.
struct LnJob2 : LnJob {
  bf16_t* out2;
  const bf16_t *shift2, *scale2;
};
static_assert(sizeof(LnJob2) % 8 == 0 && alignof(LnJob2) == 8, "job b follows job a without padding in the kernarg segment");
// ADD (ControlNet residuals, dk_mmdit_set_control_taps): a job carries a tap t, [M, ldt] dense rows in the element type, and an fp32 scalar s.  Row
// m becomes x' = round( fmaf(s, t[m], x) ) -- fp32, one rounding to the element type -- BEFORE anything else: the tap chunks are loaded in the
// row's round trip, x' goes back over x through the row's own resource, and the two reductions and the modulated store run on x' from the
// same registers.  A job without a tap (the text stream riding in the same launch) has t null: a tap resource of zero bytes, and the add
// and the write-back are skipped on a wave-uniform test.  The plain and the DUAL instantiations do not see any of this.
// The tap's row map (FLUX ControlNet taps, dk_mmdit_set_flux_control_taps): of every tseg logical rows the first t0 have no tap (the text rows of
// a joint stream) and row s >= t0 of group b takes tap row b * (tseg - t0) + (s - t0).  A row without a tap is a job without one, decided per
// wave: the zero-byte resource, no add, no write-back.  (tseg = M, t0 = 0: row m takes tap row m, the SD3 form.)
struct LnJobT : LnJob {
  const bf16_t* t;
  float s;
  int ldt, tseg, t0;
};
static_assert(sizeof(LnJobT) % 8 == 0 && alignof(LnJobT) == 8, "job b follows job a without padding in the kernarg segment");
template <bool DUAL, bool ADD = false> struct LnJobOf { typedef LnJob type; };
template <> struct LnJobOf<true, false> { typedef LnJob2 type; };
template <> struct LnJobOf<false, true> { typedef LnJobT type; };
template <int NCH, bool DUAL = false, bool ADD = false>
__global__ __launch_bounds__(256) void dk_ln_modulate_kernel(typename LnJobOf<DUAL, ADD>::type ja, typename LnJobOf<DUAL, ADD>::type jb, int blocks_a, int h, float eps) {
  static_assert(!(DUAL && ADD), "one of the two cases at a time");
  typedef typename LnJobOf<DUAL, ADD>::type Job;
  const bool first = (int)blockIdx.x < blocks_a;
  // one scalar base pointer into the kernarg segment (`first ? ja : jb` copies both jobs to scratch, see gemm256v3.hip)
  typedef const __attribute__((address_space(4))) Job karg_job_t;
  const __attribute__((address_space(4))) char* kbase = (const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr();
  karg_job_t& j = *(karg_job_t*)(kbase + (first ? 0 : sizeof(Job)));
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (uniform: row bases live in SGPRs)
  const int m = ((int)blockIdx.x - (first ? 0 : blocks_a)) * 4 + wave;
  if (m >= j.M) return;
  const size_t xrow = (size_t)((m / j.x_seg_len) * j.x_seg_stride + (m % j.x_seg_len)) * j.ldx;
  const size_t mod = (size_t)(m / j.seg_len) * j.mod_stride;
  const int nchunks = h >> 3;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(j.x + xrow), 0, h * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsh = __builtin_amdgcn_make_buffer_rsrc((void*)(j.shift + mod), 0, h * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsc = __builtin_amdgcn_make_buffer_rsrc((void*)(j.scale + mod), 0, h * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)(j.out + (size_t)m * j.ldo), 0, h * 2, 0x00020000);
  u32x4 raw[NCH], rs[NCH], rc[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) raw[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, (lane + 64 * i) * 16, 0, 0);
  // the tap (ADD): its loads follow the row's, ahead of shift / scale -- the add needs only these two; a plain kernel keeps one register
  constexpr int NCHT = ADD ? NCH : 1;
  u32x4 rt[NCHT];
  bool tapped = false;
  if constexpr (ADD) {
    tapped = j.t != nullptr;
    size_t trow = 0;
    if (tapped) {  // (m is wave-uniform, and so is everything here: scalar arithmetic)
      const int ts = m % j.tseg;
      tapped = ts >= j.t0;
      if (tapped) trow = (size_t)((m / j.tseg) * (j.tseg - j.t0) + (ts - j.t0)) * j.ldt;
    }
    // (a job or a row without a tap: a resource of zero bytes at the row -- every lane reads zeros, and no tap row is addressed)
    const __amdgpu_buffer_rsrc_t rtap =
        __builtin_amdgcn_make_buffer_rsrc((void*)(tapped ? j.t + trow : j.x + xrow), 0, tapped ? h * 2 : 0, 0x00020000);
#pragma unroll
    for (int i = 0; i < NCH; ++i) rt[i] = __builtin_amdgcn_raw_buffer_load_b128(rtap, (lane + 64 * i) * 16, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    rs[i] = __builtin_amdgcn_raw_buffer_load_b128(rsh, (lane + 64 * i) * 16, 0, 0);
    rc[i] = __builtin_amdgcn_raw_buffer_load_b128(rsc, (lane + 64 * i) * 16, 0, 0);
  }
  // the second triple (DUAL): its loads join the same round trip; a plain kernel keeps one register of each array, never touched
  constexpr int NCH2 = DUAL ? NCH : 1;
  u32x4 rs2[NCH2], rc2[NCH2];
  __amdgpu_buffer_rsrc_t ro2 = ro;
  bool second = false;
  if constexpr (DUAL) {
    const __amdgpu_buffer_rsrc_t rsh2 = __builtin_amdgcn_make_buffer_rsrc((void*)(j.shift2 + mod), 0, h * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsc2 = __builtin_amdgcn_make_buffer_rsrc((void*)(j.scale2 + mod), 0, h * 2, 0x00020000);
    second = j.out2 != nullptr;
    // (a job without a second output: a resource of zero bytes at the first output's row -- nothing can be stored through it)
    ro2 = __builtin_amdgcn_make_buffer_rsrc((void*)((second ? j.out2 : j.out) + (size_t)m * j.ldo), 0, second ? h * 2 : 0, 0x00020000);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      rs2[i] = __builtin_amdgcn_raw_buffer_load_b128(rsh2, (lane + 64 * i) * 16, 0, 0);
      rc2[i] = __builtin_amdgcn_raw_buffer_load_b128(rsc2, (lane + 64 * i) * 16, 0, 0);
    }
  }
  __builtin_amdgcn_sched_barrier(0);  // (without it the scheduler sinks the shift / scale loads below the two reductions)
  if constexpr (ADD) {
    if (tapped) {  // (wave-uniform)
      const float s = j.s;
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v0, v1, t0, t1;
          unpack2(raw[i][e], v0, v1);
          unpack2(rt[i][e], t0, t1);
          raw[i][e] = pack2(__builtin_fmaf(s, t0, v0), __builtin_fmaf(s, t1, v1));  // (zeros past the row end stay zeros)
        }
        __builtin_amdgcn_raw_buffer_store_b128(raw[i], rx, (lane + 64 * i) * 16, 0, 0);  // (past the row end: dropped)
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v0, v1;
      unpack2(raw[i][e], v0, v1);
      sum += v0 + v1;  // (zeros past the row end)
    }
  }
  const float mean = wave_sum(sum) / (float)h;
  __builtin_amdgcn_sched_barrier(0);  // (this one and the next two keep each pass's unpacked values out of the others' live ranges)
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const bool live = lane + 64 * i < nchunks;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v0, v1;
      asm volatile("" : "+v"(raw[i][e]));  // (opaque: else the unpacked row of pass 1 is kept live, 8 registers per chunk instead of 4)
      unpack2(raw[i][e], v0, v1);
      const float d0 = live ? v0 - mean : 0.f, d1 = live ? v1 - mean : 0.f;  // (masked before the product: sq += d * d stays one fma)
      sq += d0 * d0;
      sq += d1 * d1;
    }
  }
  const float rstd = rsqrtf(wave_sum(sq) / (float)h + eps);
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    __builtin_amdgcn_sched_barrier(0);
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v0, v1, s0, s1, c0, c1;
      asm volatile("" : "+v"(raw[i][e]));  // (and v - mean of pass 2 likewise)
      unpack2(raw[i][e], v0, v1);
      unpack2(rs[i][e], s0, s1);
      unpack2(rc[i][e], c0, c1);
      const float y0 = (v0 - mean) * rstd * round_act(1.0f + c0) + s0;
      const float y1 = (v1 - mean) * rstd * round_act(1.0f + c1) + s1;
      o[e] = pack2(y0, y1);
    }
    __builtin_amdgcn_raw_buffer_store_b128(o, ro, (lane + 64 * i) * 16, 0, 0);
    if constexpr (DUAL) {
      if (second) {  // (wave-uniform)
        u32x4 o2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v0, v1, s0, s1, c0, c1;
          unpack2(raw[i][e], v0, v1);
          unpack2(rs2[i][e], s0, s1);
          unpack2(rc2[i][e], c0, c1);
          const float y0 = (v0 - mean) * rstd * round_act(1.0f + c0) + s0;
          const float y1 = (v1 - mean) * rstd * round_act(1.0f + c1) + s1;
          o2[e] = pack2(y0, y1);
        }
        __builtin_amdgcn_raw_buffer_store_b128(o2, ro2, (lane + 64 * i) * 16, 0, 0);
      }
    }
  }
}

static int launch_ln_jobs(const LnJob& a, const LnJob& b, int h, float eps, hipStream_t stream) {
  DK_REQUIRE(h % 8 == 0 && h <= 4096, "hidden size must be a multiple of 8 and <= 4096");
  for (const LnJob* j : {&a, &b})
    DK_REQUIRE(j->M == 0 || (j->ldx % 8 == 0 && j->ldo % 8 == 0 && j->mod_stride % 8 == 0), "strides must keep 16-byte alignment");
  const int blocks_a = (a.M + 3) / 4, blocks_b = (b.M + 3) / 4;
  dim3 grid(blocks_a + blocks_b), block(256);
  const int nch = (h / 8 + 63) / 64;
#define LN_CASE(N)                                                                                         \
  case N:                                                                                                  \
    hipLaunchKernelGGL(dk_ln_modulate_kernel<N>, grid, block, 0, stream, a, b, blocks_a, h, eps);          \
    break;
  switch (nch) {
    LN_CASE(1) LN_CASE(2) LN_CASE(3) LN_CASE(4) LN_CASE(5) LN_CASE(6) LN_CASE(7) LN_CASE(8)
    default: DK_REQUIRE(false, "unsupported hidden size");
  }
#undef LN_CASE
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}
static LnJob ln_job(const bf16_t* x, int ldx, bf16_t* out, int ldo, int M, const bf16_t* shift, const bf16_t* scale, int mod_stride,
                    int seg_len, int x_seg_len, int x_seg_stride) {
  LnJob j;
  j.x = x; j.out = out; j.shift = shift; j.scale = scale; j.ldx = ldx; j.ldo = ldo; j.M = M; j.mod_stride = mod_stride;
  j.seg_len = seg_len; j.x_seg_len = x_seg_len; j.x_seg_stride = x_seg_stride;
  return j;
}
int dk_launch_ln_modulate(const bf16_t* x, int ldx, bf16_t* out, int ldo, int M, int h, const bf16_t* shift,
                          const bf16_t* scale, int mod_stride, int seg_len, int x_seg_len, int x_seg_stride, float eps,
                          hipStream_t stream) {
  LnJob none = ln_job(nullptr, 8, nullptr, 8, 0, nullptr, nullptr, 8, 1, 1, 0);
  return launch_ln_jobs(ln_job(x, ldx, out, ldo, M, shift, scale, mod_stride, seg_len, x_seg_len, x_seg_stride), none, h, eps, stream);
}
// the DUAL instantiations: job a with its two triples, job b plain (M == 0: absent)
static int launch_ln_jobs_dual(const LnJob2& a, const LnJob2& b, int h, float eps, hipStream_t stream) {
  DK_REQUIRE(h % 8 == 0 && h <= 4096, "hidden size must be a multiple of 8 and <= 4096");
  for (const LnJob2* j : {&a, &b})
    DK_REQUIRE(j->M == 0 || (j->ldx % 8 == 0 && j->ldo % 8 == 0 && j->mod_stride % 8 == 0), "strides must keep 16-byte alignment");
  const int blocks_a = (a.M + 3) / 4, blocks_b = (b.M + 3) / 4;
  dim3 grid(blocks_a + blocks_b), block(256);
  const int nch = (h / 8 + 63) / 64;
#define LN_CASE(N)                                                                                               \
  case N:                                                                                                        \
    hipLaunchKernelGGL((dk_ln_modulate_kernel<N, true>), grid, block, 0, stream, a, b, blocks_a, h, eps);        \
    break;
  switch (nch) {
    LN_CASE(1) LN_CASE(2) LN_CASE(3) LN_CASE(4) LN_CASE(5) LN_CASE(6) LN_CASE(7) LN_CASE(8)
    default: DK_REQUIRE(false, "unsupported hidden size");
  }
#undef LN_CASE
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}
static LnJob2 ln_job2(const LnJob& j, bf16_t* out2, const bf16_t* shift2, const bf16_t* scale2) {
  LnJob2 d;
  static_cast<LnJob&>(d) = j;
  d.out2 = out2; d.shift2 = out2 ? shift2 : j.shift; d.scale2 = out2 ? scale2 : j.scale;
  return d;
}
// ... of which the first leaves twice (MMDiT-X dual-attention block: out0 under (shift0, scale0), out0b under (shift0b, scale0b)); M1 == 0:
// no second row set (x_seg_stride1: its own segment stride -- the engine's two streams share one, S)
int dk_launch_ln_modulate2x(const bf16_t* x0, bf16_t* out0, bf16_t* out0b, int M0, const bf16_t* shift0, const bf16_t* scale0,
                            const bf16_t* shift0b, const bf16_t* scale0b, int seg0, const bf16_t* x1, bf16_t* out1, int M1,
                            const bf16_t* shift1, const bf16_t* scale1, int seg1, int ldx, int ldo, int h, int mod_stride, int x_seg_stride,
                            int x_seg_stride1, float eps, hipStream_t stream) {
  DK_REQUIRE(x0 && out0 && out0b && shift0 && scale0 && shift0b && scale0b && M0 > 0 && seg0 > 0, "ln_modulate2x: the dual job needs both triples");
  DK_REQUIRE(M1 == 0 || (x1 && out1 && shift1 && scale1 && seg1 > 0), "ln_modulate2x: bad second row set");
  const LnJob b = M1 > 0 ? ln_job(x1, ldx, out1, ldo, M1, shift1, scale1, mod_stride, seg1, seg1, x_seg_stride1)
                         : ln_job(nullptr, 8, nullptr, 8, 0, nullptr, nullptr, 8, 1, 1, 0);
  return launch_ln_jobs_dual(ln_job2(ln_job(x0, ldx, out0, ldo, M0, shift0, scale0, mod_stride, seg0, seg0, x_seg_stride), out0b, shift0b, scale0b),
                             ln_job2(b, nullptr, nullptr, nullptr), h, eps, stream);
}
// the ADD instantiations: job a with its tap, job b plain (M == 0: absent)
static int launch_ln_jobs_add(const LnJobT& a, const LnJobT& b, int h, float eps, hipStream_t stream) {
  DK_REQUIRE(h % 8 == 0 && h <= 4096, "hidden size must be a multiple of 8 and <= 4096");
  for (const LnJobT* j : {&a, &b})
    DK_REQUIRE(j->M == 0 || (j->ldx % 8 == 0 && j->ldo % 8 == 0 && j->mod_stride % 8 == 0), "strides must keep 16-byte alignment");
  const int blocks_a = (a.M + 3) / 4, blocks_b = (b.M + 3) / 4;
  dim3 grid(blocks_a + blocks_b), block(256);
  const int nch = (h / 8 + 63) / 64;
#define LN_CASE(N)                                                                                                      \
  case N:                                                                                                               \
    hipLaunchKernelGGL((dk_ln_modulate_kernel<N, false, true>), grid, block, 0, stream, a, b, blocks_a, h, eps);        \
    break;
  switch (nch) {
    LN_CASE(1) LN_CASE(2) LN_CASE(3) LN_CASE(4) LN_CASE(5) LN_CASE(6) LN_CASE(7) LN_CASE(8)
    default: DK_REQUIRE(false, "unsupported hidden size");
  }
#undef LN_CASE
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}
// (tseg == 0: every row of the job, row m onto tap row m)
static LnJobT ln_job_tap(const LnJob& j, const bf16_t* t, int ldt, float s, int tseg = 0, int t0 = 0) {
  LnJobT d;
  static_cast<LnJob&>(d) = j;
  d.t = t; d.s = t ? s : 0.f; d.ldt = t ? ldt : 8;
  d.tseg = t && tseg > 0 ? tseg : (j.M > 0 ? j.M : 1); d.t0 = t && tseg > 0 ? t0 : 0;
  return d;
}
// ... of which the first takes a residual first (ControlNet taps): x0 <- round(x0 + s * tap) in place, row m of the dense [M0, ldt] tap onto
// logical row m of x0, and out0 is the modulated LayerNorm of the new rows; the second row set is plain (M1 == 0: none)
int dk_launch_ln_modulate2_add(bf16_t* x0, const bf16_t* tap, int ldt, float s, bf16_t* out0, int M0, const bf16_t* shift0, const bf16_t* scale0,
                               int seg0, const bf16_t* x1, bf16_t* out1, int M1, const bf16_t* shift1, const bf16_t* scale1, int seg1, int ldx,
                               int ldo, int h, int mod_stride, int x_seg_stride, int x_seg_stride1, float eps, hipStream_t stream) {
  DK_REQUIRE(x0 && tap && out0 && shift0 && scale0 && M0 > 0 && seg0 > 0, "ln_modulate2_add: the first row set needs its tap");
  DK_REQUIRE(ldt >= h && ldt % 8 == 0 && ((uintptr_t)tap & 15) == 0, "ln_modulate2_add: the tap's rows must be 16-byte aligned and hold h elements");
  DK_REQUIRE(M1 == 0 || (x1 && out1 && shift1 && scale1 && seg1 > 0), "ln_modulate2_add: bad second row set");
  const LnJob b = M1 > 0 ? ln_job(x1, ldx, out1, ldo, M1, shift1, scale1, mod_stride, seg1, seg1, x_seg_stride1)
                         : ln_job(nullptr, 8, nullptr, 8, 0, nullptr, nullptr, 8, 1, 1, 0);
  return launch_ln_jobs_add(ln_job_tap(ln_job(x0, ldx, out0, ldo, M0, shift0, scale0, mod_stride, seg0, seg0, x_seg_stride), tap, ldt, s),
                            ln_job_tap(b, nullptr, 0, 0.f), h, eps, stream);
}
#ifndef DK_ELEM_F16  // (the FLUX family has no fp16 path)
// ONE job over a joint stream, of which only some rows take the residual (FLUX ControlNet taps): of every tap_seg logical rows the first tap_first
// (the text rows) are plain -- neither added to nor written back -- and row s >= tap_first of group b takes row b * (tap_seg - tap_first) +
// (s - tap_first) of the dense [(M / tap_seg) * (tap_seg - tap_first), ldt] tap; no tap row exists for a text row and none is addressed.
// tap_first == 0: every row (the final layer's image rows, x at the first image row with x_seg_len = tap_seg = S_i, x_seg_stride = S)
int dk_launch_ln_modulate_add_joint(bf16_t* x, int ldx, const bf16_t* tap, int ldt, float s, int tap_seg, int tap_first, bf16_t* out, int ldo, int M,
                                    int h, const bf16_t* shift, const bf16_t* scale, int mod_stride, int seg_len, int x_seg_len, int x_seg_stride,
                                    float eps, hipStream_t stream) {
  DK_REQUIRE(x && tap && out && shift && scale && M > 0 && seg_len > 0 && x_seg_len > 0, "ln_modulate_add_joint: null or empty argument");
  DK_REQUIRE(ldt >= h && ldt % 8 == 0 && ((uintptr_t)tap & 15) == 0, "ln_modulate_add_joint: the tap's rows must be 16-byte aligned and hold h elements");
  DK_REQUIRE(tap_seg > 0 && tap_first >= 0 && tap_first < tap_seg && M % tap_seg == 0,
             "ln_modulate_add_joint: the rows are whole groups of tap_seg, of which the first tap_first (fewer than tap_seg) take no tap");
  const LnJob none = ln_job(nullptr, 8, nullptr, 8, 0, nullptr, nullptr, 8, 1, 1, 0);
  return launch_ln_jobs_add(ln_job_tap(ln_job(x, ldx, out, ldo, M, shift, scale, mod_stride, seg_len, x_seg_len, x_seg_stride), tap, ldt, s, tap_seg, tap_first),
                            ln_job_tap(none, nullptr, 0, 0.f), h, eps, stream);
}
#endif
// two row sets (image / text stream) of the same hidden size in one launch
int dk_launch_ln_modulate2(const bf16_t* x0, bf16_t* out0, int M0, const bf16_t* shift0, const bf16_t* scale0, int seg0, const bf16_t* x1,
                           bf16_t* out1, int M1, const bf16_t* shift1, const bf16_t* scale1, int seg1, int ldx, int ldo, int h,
                           int mod_stride, int x_seg_stride, float eps, hipStream_t stream) {
  return launch_ln_jobs(ln_job(x0, ldx, out0, ldo, M0, shift0, scale0, mod_stride, seg0, seg0, x_seg_stride),
                        ln_job(x1, ldx, out1, ldo, M1, shift1, scale1, mod_stride, seg1, seg1, x_seg_stride), h, eps, stream);
}

// ---------------------------------------------------------------------------------------------
// In-place per-head RMSNorm (learned weight) followed by RoPE on the q and k column groups of a
// token-major QKV buffer.  reference: QKNorm python/src/diffusionkit/mlx/mmdit.py:754-764
// (nn.RMSNorm eps 1e-6, one rounding), RoPE.apply :934-942 (adjacent pairs, fp32, one rounding).
// D/8 lanes cooperate on one (row, head, q|k) item; rope == nullptr skips the rotation,
// qw == nullptr skips the norm.
// ---------------------------------------------------------------------------------------------
struct QkJob {  // (two jobs per launch like LnJob)
  bf16_t* qkv;
  const bf16_t *qw, *kw;
  int rows, row_seg_len, row_seg_stride, pos_off;
};
template <int D>
__global__ __launch_bounds__(256) void dk_qk_norm_rope_kernel(QkJob ja, QkJob jb, int blocks_a, int ld, int q_off, int k_off, int H, float eps,
                                                              const float* __restrict__ rope, int k_only) {
  const bool first = (int)blockIdx.x < blocks_a;
  const QkJob& jj = first ? ja : jb;
  bf16_t* __restrict__ qkv = jj.qkv;
  const bf16_t* __restrict__ qw = jj.qw;
  const bf16_t* __restrict__ kw = jj.kw;
  const int rows = jj.rows, row_seg_len = jj.row_seg_len, row_seg_stride = jj.row_seg_stride, pos_off = jj.pos_off;
  constexpr int LPI = D / 8;  // lanes per item
  // 32-bit index arithmetic (rows * 2H * LPI < 2^31, checked by the launcher): 64-bit divisions cost more VALU
  // work than the 16 bytes this lane moves
  const unsigned gid = (blockIdx.x - (first ? 0u : (unsigned)blocks_a)) * 256u + threadIdx.x;
  const unsigned item = gid / LPI;
  const int sub = (int)(gid % LPI);
  // k_only: the queries are normalised / rotated inside the attention kernel's Q load, this pass touches the keys
  const unsigned per_row = (k_only ? 1u : 2u) * (unsigned)H;
  const unsigned nitems = (unsigned)rows * per_row;
  const bool active = item < nitems;
  const unsigned it = active ? item : nitems - 1;
  const int m = (int)(it / per_row);
  const int rem = (int)(it - (unsigned)m * per_row);
  const int which = k_only ? 1 : (rem >= H ? 1 : 0), head = k_only ? rem : rem - which * H;
  const int seg = m / row_seg_len, pos_in = m % row_seg_len;
  bf16_t* ptr = qkv + (size_t)(seg * row_seg_stride + pos_in) * ld + (which ? k_off : q_off) + head * D + sub * 8;
  const u32x4 raw = *(const u32x4*)ptr;
  float v[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) unpack2(raw[e], v[2 * e], v[2 * e + 1]);
  const bf16_t* w = which ? kw : qw;
  if (w != nullptr) {
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) ss += v[e] * v[e];
#pragma unroll
    for (int o = LPI / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float r = rsqrtf(ss / (float)D + eps);
    const u32x4 wr = *(const u32x4*)(w + sub * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float w0, w1;
      unpack2(wr[e], w0, w1);
      v[2 * e] = round_act(v[2 * e] * r * w0);
      v[2 * e + 1] = round_act(v[2 * e + 1] * r * w1);
    }
  }
  if (rope != nullptr) {
    const float* tab = rope + ((size_t)(pos_off + pos_in) * (D / 2) + sub * 4) * 2;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float c = tab[2 * e], s = tab[2 * e + 1];
      const float xe = v[2 * e], xo = v[2 * e + 1];
      v[2 * e] = c * xe - s * xo;
      v[2 * e + 1] = s * xe + c * xo;
    }
  }
  if (active) {
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pack2(v[2 * e], v[2 * e + 1]);
    *(u32x4*)ptr = o;
  }
}

static int launch_qk_jobs(const QkJob& a, const QkJob& b, int ld, int q_off, int k_off, int H, int D, float eps, const float* rope,
                          hipStream_t stream, int k_only = 0) {
  DK_REQUIRE(D == 64 || D == 128, "head_dim must be 64 or 128");
  DK_REQUIRE(ld % 8 == 0 && q_off % 8 == 0 && k_off % 8 == 0, "alignment");
  const int per_row = (k_only ? 1 : 2) * H;
  const long ta = (long)a.rows * per_row * (D / 8), tb = (long)b.rows * per_row * (D / 8);
  DK_REQUIRE(ta + tb < (1L << 31) - 512, "qk_norm_rope: rows * 2H * D/8 must stay below 2^31");
  const int blocks_a = (int)((ta + 255) / 256), blocks_b = (int)((tb + 255) / 256);
  dim3 grid(blocks_a + blocks_b), block(256);
  if (D == 128)
    hipLaunchKernelGGL(dk_qk_norm_rope_kernel<128>, grid, block, 0, stream, a, b, blocks_a, ld, q_off, k_off, H, eps, rope, k_only);
  else
    hipLaunchKernelGGL(dk_qk_norm_rope_kernel<64>, grid, block, 0, stream, a, b, blocks_a, ld, q_off, k_off, H, eps, rope, k_only);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}
int dk_launch_qk_norm_rope(bf16_t* qkv, int ld, int q_off, int k_off, int rows, int H, int D, const bf16_t* qw,
                           const bf16_t* kw, float eps, const float* rope, int row_seg_len, int row_seg_stride, int pos_off,
                           int S_pos, hipStream_t stream, int k_only) {
  (void)S_pos;
  if (qw == nullptr && kw == nullptr && rope == nullptr) return 0;  // (a key weight alone is work: dk_qk_norm_rope_bf16 with q_weight NULL, no table)
  QkJob a{qkv, qw, kw, rows, row_seg_len, row_seg_stride, pos_off}, none{nullptr, nullptr, nullptr, 0, 1, 0, 0};
  return launch_qk_jobs(a, none, ld, q_off, k_off, H, D, eps, rope, stream, k_only);
}
// the two streams of a double block (same buffer geometry, own weights / row segments / positions) in one launch
int dk_launch_qk_norm_rope2(bf16_t* qkv0, int rows0, const bf16_t* qw0, const bf16_t* kw0, int seg0, int pos0, bf16_t* qkv1, int rows1,
                            const bf16_t* qw1, const bf16_t* kw1, int seg1, int pos1, int ld, int q_off, int k_off, int H, int D,
                            float eps, const float* rope, int row_seg_stride, hipStream_t stream, int k_only) {
  if (qw0 == nullptr && kw0 == nullptr && qw1 == nullptr && kw1 == nullptr && rope == nullptr) return 0;
  QkJob a{qkv0, qw0, kw0, rows0, seg0, row_seg_stride, pos0}, b{qkv1, qw1, kw1, rows1, seg1, row_seg_stride, pos1};
  return launch_qk_jobs(a, b, ld, q_off, k_off, H, D, eps, rope, stream, k_only);
}

// ---------------------------------------------------------------------------------------------
// small elementwise helpers
// ---------------------------------------------------------------------------------------------
__global__ void dk_silu_kernel(const bf16_t* x, bf16_t* y, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = from_f32(silu_f(to_f32(x[i])));
}
int dk_launch_silu(const bf16_t* x, bf16_t* y, long n, hipStream_t stream) {
  hipLaunchKernelGGL(dk_silu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, y, n);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}

// y[r, :] = bf16(a[r, :] + b[r / (rows / b_rows) , :])   (used for vec = y_embed[b] + t_embed[step])
__global__ void dk_add_kernel(const bf16_t* a, const bf16_t* b, int a_rows, int b_rows, bf16_t* y, int rows, int cols) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)rows * cols) return;
  const int r = (int)(i / cols), c = (int)(i % cols);
  // a is indexed by r % a_rows (batch row), b by r / a_rows (timestep row)
  y[i] = from_f32(to_f32(a[(size_t)(r % a_rows) * cols + c]) + to_f32(b[(size_t)min(r / a_rows, b_rows - 1) * cols + c]));
}
int dk_launch_add(const bf16_t* a, const bf16_t* b, int b_rows, bf16_t* y, int rows, int cols, hipStream_t stream) {
  const int a_rows = rows / b_rows;
  const long n = (long)rows * cols;
  hipLaunchKernelGGL(dk_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a, b, a_rows, b_rows, y, rows, cols);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}

__device__ __forceinline__ float round_to(float v, int dt) {
  if (dt == 0) return round_bf16(v);
  if (dt == 1) return (float)(_Float16)v;
  return v;
}
// Sinusoidal timestep embedding evaluated in the reference's config.dtype
// (python/src/diffusionkit/mlx/mmdit.py:379-389, quirk Q2): out[i, :] = [cos(args), sin(args)].
__global__ void dk_timestep_embedding_kernel(const float* t, int n, int dim, float max_period, int dt, bf16_t* out) {
  const int i = blockIdx.x, j = threadIdx.x;
  const int half = dim / 2;
  if (i >= n || j >= half) return;
  const float ar = round_to((float)j, dt);
  const float freq = round_to(expf(-logf(max_period) * ar / (float)half), dt);
  const float arg = round_to(round_to(t[i], dt) * freq, dt);
  out[(size_t)i * dim + j] = from_f32(round_to(cosf(arg), dt));
  out[(size_t)i * dim + half + j] = from_f32(round_to(sinf(arg), dt));
}
int dk_launch_timestep_embedding(const float* t, int n, int rep, int dim, float max_period, int embed_dtype, bf16_t* out,
                                 hipStream_t stream) {
  (void)rep;
  DK_REQUIRE(dim % 2 == 0 && dim / 2 <= 1024, "frequency_embed_dim");
  hipLaunchKernelGGL(dk_timestep_embedding_kernel, dim3(n), dim3(dim / 2), 0, stream, t, n, dim, max_period, embed_dtype, out);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------
// The noise of the stochastic samplers (no reference counterpart; the definition is sampler.philox4x32_10 / philox_normal_reference).
// Philox4x32-10 (Salmon et al., SC'11), counter (q & 0xffffffff, q >> 32, draw, stream), key (seed & 0xffffffff, seed >> 32); a block
// (o0, o1, o2, o3) gives four normals by Box-Muller on 24-bit uniforms, pairs (o0, o1) -> z0, z1 and (o2, o3) -> z2, z3, and element r of an image
// takes z[r % 4] of quad q = r / 4.  Every thread runs the ten rounds of its own quad and keeps one of the four normals: the four threads of a quad
// repeat each other's block (about forty 32-bit multiplies each) instead of exchanging it, so that a value depends on (seed, q, draw, stream, r % 4)
// alone -- not on which lanes of a wave are live, nor on the launch that asks -- and the operator and the step kernel share this one function.
// u = ((o_a >> 8) + 1) 2^-24 is exact in fp32 and never 0; the angle is taken in half turns, 2 (o_b >> 8) 2^-24, exact too, through sinpif / cospif.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float philox_normal(unsigned long long seed, unsigned long long q, unsigned draw, unsigned stream, int k) {
  unsigned c0 = (unsigned)q, c1 = (unsigned)(q >> 32), c2 = draw, c3 = stream;
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0, c1 = l1, c2 = h0 ^ c3 ^ k1, c3 = l0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  const unsigned oa = (k & 2) ? c2 : c0, ob = (k & 2) ? c3 : c1;
  const float u = (float)((oa >> 8) + 1u) * 0x1p-24f;
  const float turns = (float)(ob >> 8) * 0x1p-23f;
  const float rad = sqrtf(-2.0f * logf(u));
  return rad * ((k & 1) ? sinpif(turns) : cospif(turns));
}

#ifndef DK_ELEM_F16  // (fp32 / bf16-only helpers: one copy)
// out f32 [n_img, n_per_img]: row j holds the normals of seeds[j] from quad quad_offset on (dk_philox_normal_f32; n_per_img % 4 == 0)
__global__ void dk_philox_normal_kernel(float* out, const unsigned long long* seeds, long n_img, long n_per_img, unsigned draw, unsigned stream,
                                        unsigned long long quad_offset) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_img * n_per_img) return;
  const long img = i / n_per_img, r = i % n_per_img;
  out[i] = philox_normal(seeds[img], quad_offset + (unsigned long long)(r >> 2), draw, stream, (int)(r & 3));
}
int dk_launch_philox_normal(float* out, const unsigned long long* seeds, int n_img, long n_per_img, unsigned draw, unsigned stream,
                            unsigned long long quad_offset, hipStream_t st) {
  const long n = (long)n_img * n_per_img;
  DK_REQUIRE(n > 0 && (n + 255) / 256 <= 0x7fffffffL, "philox_normal: size");
  hipLaunchKernelGGL(dk_philox_normal_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out, seeds, (long)n_img, n_per_img, draw, stream,
                     quad_offset);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}
// RoPE cos/sin table [S, D/2, 2] for the joint [text, image] sequence
// (python/src/diffusionkit/mlx/mmdit.py:865-911, quirk Q14).
struct RopeAxes { int dim[4]; int n; };
// the grids behind the text rows: segment i holds gh[i] * gw[i] rows at positions (index[i], row, col), rows and columns counted from 0 in
// every segment (one segment at index 0: the image; FLUX.1 Kontext's reference image is a second one at index 1)
#define DK_ROPE_MAX_SEG 4
struct RopeSegs { int gh[DK_ROPE_MAX_SEG], gw[DK_ROPE_MAX_SEG], index[DK_ROPE_MAX_SEG]; int n; };
__global__ void dk_rope_table_kernel(float* table, int S_txt, RopeSegs sg, RopeAxes ax, float theta, int half) {
  const int s = blockIdx.x, pi = threadIdx.x;
  if (pi >= half) return;
  float pos[4] = {0.f, 0.f, 0.f, 0.f};
  if (s >= S_txt) {
    int idx = s - S_txt, g = 0;
    while (g < sg.n - 1 && idx >= sg.gh[g] * sg.gw[g]) {
      idx -= sg.gh[g] * sg.gw[g];
      ++g;
    }
    pos[0] = (float)sg.index[g];
    pos[1] = (float)(idx / sg.gw[g]);
    pos[2] = (float)(idx % sg.gw[g]);
  }
  int a = 0, local = pi;
  while (a < ax.n - 1 && local >= ax.dim[a] / 2) {
    local -= ax.dim[a] / 2;
    ++a;
  }
  const float scale = (float)(2 * local) / (float)ax.dim[a];
  const float omega = 1.0f / powf(theta, scale);
  const float ang = pos[a] * omega;
  table[((size_t)s * half + pi) * 2 + 0] = cosf(ang);
  table[((size_t)s * half + pi) * 2 + 1] = sinf(ang);
}
int dk_launch_rope_table_segments(float* table, int S_txt, int n_seg, const int* seg, const int* axes, int n_axes, float theta,
                                  hipStream_t stream) {
  DK_REQUIRE(table != nullptr && seg != nullptr && axes != nullptr, "null argument");
  DK_REQUIRE(n_axes >= 1 && n_axes <= 4, "rope axes");
  DK_REQUIRE(n_seg >= 1 && n_seg <= DK_ROPE_MAX_SEG, "rope table: 1 to 4 grid segments");
  DK_REQUIRE(S_txt >= 0, "rope table: negative text length");
  RopeAxes ax;
  RopeSegs sg;
  int half = 0;
  long S = S_txt;
  for (int i = 0; i < 4; ++i) ax.dim[i] = 0;
  for (int i = 0; i < n_axes; ++i) {
    ax.dim[i] = axes[i];
    half += axes[i] / 2;
  }
  ax.n = n_axes;
  for (int i = 0; i < DK_ROPE_MAX_SEG; ++i) sg.gh[i] = sg.gw[i] = sg.index[i] = 0;
  for (int i = 0; i < n_seg; ++i) {
    DK_REQUIRE(seg[3 * i] > 0 && seg[3 * i + 1] > 0, "rope table: every grid segment needs positive sides");
    sg.gh[i] = seg[3 * i]; sg.gw[i] = seg[3 * i + 1]; sg.index[i] = seg[3 * i + 2];
    S += (long)sg.gh[i] * sg.gw[i];
  }
  sg.n = n_seg;
  DK_REQUIRE(half >= 1 && half <= 1024 && S >= 1 && S <= 0x7fffffffL, "rope table: size");
  hipLaunchKernelGGL(dk_rope_table_kernel, dim3((unsigned)S), dim3(((half + 63) / 64) * 64), 0, stream, table, S_txt, sg, ax, theta, half);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}
int dk_launch_rope_table(float* table, int S_txt, int gh, int gw, const int* axes, int n_axes, float theta, hipStream_t stream) {
  const int seg[3] = {gh, gw, 0};
  return dk_launch_rope_table_segments(table, S_txt, 1, seg, axes, n_axes, theta, stream);
}

__global__ void dk_f32_to_bf16_kernel(const float* x, bf16_t* y, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = f2bf(x[i]);
}
int dk_launch_f32_to_bf16(const float* x, bf16_t* y, long n, hipStream_t stream) {
  hipLaunchKernelGGL(dk_f32_to_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, y, n);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}
__global__ void dk_affine_f32_kernel(const float* x, float* y, long n, float a, float b) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = x[i] * a + b;
}
int dk_launch_affine_f32(const float* x, float* y, long n, float a, float b, hipStream_t stream) {
  hipLaunchKernelGGL(dk_affine_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, y, n, a, b);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}

// Inpainting mask, pixels -> latent cells: u8 [n_mask, H, W] (255 = repaint, 0 = keep) -> f32 [n_mask, H / f, W / f], the integer sum of
// an f x f block over f * f * 255 by a true division: an all-0 block is exactly 0.0f, an all-255 block exactly 1.0f.
__global__ void dk_mask_to_latent_kernel(const unsigned char* mask, float* out, int n_mask, int H, int W, int f) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int Hl = H / f, Wl = W / f;
  if (i >= (long)n_mask * Hl * Wl) return;
  const int xx = (int)(i % Wl), yy = (int)(i / Wl % Hl), n = (int)(i / ((long)Hl * Wl));
  const unsigned char* blk = mask + ((size_t)n * H + (size_t)yy * f) * W + (size_t)xx * f;
  int sum = 0;
  for (int r = 0; r < f; ++r)
    for (int c = 0; c < f; ++c) sum += blk[(size_t)r * W + c];
  out[i] = (float)sum / (float)(f * f * 255);
}
int dk_launch_mask_to_latent(const unsigned char* mask, float* out, int n_mask, int H, int W, int f, hipStream_t stream) {
  const long n = (long)n_mask * (H / f) * (W / f);
  hipLaunchKernelGGL(dk_mask_to_latent_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, mask, out, n_mask, H, W, f);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}

// Inpainting paste-back in pixel space: out = (uint8)(w * dec + (1 - w) * orig + 0.5f), w = mask / 255.0f, one thread per pixel.
// w == 1 gives the decoder's byte, w == 0 the original's.  Contraction is off so that the bytes are those of the plain fp32 expression
// (a fused multiply-add rounds once less and can land on the other side of a truncation boundary).
__global__ void dk_image_composite_u8_kernel(const unsigned char* dec, const unsigned char* orig, const unsigned char* mask,
                                             unsigned char* out, int B, long HW, int orig_per_image, int mask_per_image) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= HW * B) return;
  const long pix = i % HW;
  const float w = (float)mask[mask_per_image ? i : pix] / 255.0f;
  const unsigned char* o = orig + (orig_per_image ? i : pix) * 3;
  for (int c = 0; c < 3; ++c) out[i * 3 + c] = (unsigned char)(w * (float)dec[i * 3 + c] + (1.0f - w) * (float)o[c] + 0.5f);
}
int dk_launch_image_composite_u8(const unsigned char* dec, const unsigned char* orig, const unsigned char* mask, unsigned char* out, int B,
                                 int H, int W, int orig_per_image, int mask_per_image, hipStream_t stream) {
  const long HW = (long)H * W;
  hipLaunchKernelGGL(dk_image_composite_u8_kernel, dim3((unsigned)((HW * B + 255) / 256)), dim3(256), 0, stream, dec, orig, mask, out, B,
                     HW, orig_per_image, mask_per_image);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}

// Channel-concatenated conditioning (FLUX.1 Fill): the image the model may look at, out = a * (1 - m) with a = u8 / 255 * 2 - 1 (read_image's
// statement) and m = mask / 255, one thread per element.  Contraction is off: every operation rounds on its own, as numpy's float32 does.
__global__ void dk_image_mask_out_f32_kernel(const unsigned char* image, const unsigned char* mask, float* out, long n_elem, long HW,
                                             int mask_per_image) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_elem) return;
  const long pix = i / 3;
  const float a = (float)image[i] / 255.0f * 2.0f - 1.0f;
  const float m = (float)mask[mask_per_image ? pix : pix % HW] / 255.0f;
  out[i] = a * (1.0f - m);
}
int dk_launch_image_mask_out_f32(const unsigned char* image, const unsigned char* mask, float* out, int n, int H, int W, int mask_per_image,
                                 hipStream_t stream) {
  const long HW = (long)H * W, n_elem = HW * 3 * n;
  DK_REQUIRE(n_elem > 0 && (n_elem + 255) / 256 <= 0x7fffffffL, "image_mask_out: size");
  hipLaunchKernelGGL(dk_image_mask_out_f32_kernel, dim3((unsigned)((n_elem + 255) / 256)), dim3(256), 0, stream, image, mask, out, n_elem, HW,
                     mask_per_image);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}

// ... and its token rows: z f32 [n, Hl, Wl, C] (+ mask u8 [n_mask, 8 Hl, 8 Wl]) -> bf16 [n, S_i, p*p*C (+ 64*p*p)], one thread per output
// element, consecutive threads along the feature axis.  Columns [0, p*p*C): the latent's patch, features (c, ph, pw) -- dk_latent_to_tokens'
// FLUX order and rounding.  Columns behind them: the mask's 8 x 8 pixel-unshuffle to 64 channels at latent resolution (channel 8 * py + px),
// through the same patchify: column p*p*C + (8 * py + px) * p*p + ph * p + pw of token (ti, tj) = bf16(mask[(ti*p + ph) * 8 + py,
// (tj*p + pw) * 8 + px] / 255).  A null mask writes the latent columns only (FLUX.1 Canny / Depth).
__global__ void dk_fill_condition_tokens_kernel(const float* z, const unsigned char* mask, bf16_t* tok, long n_out, int mask_per_image, int Hl,
                                                int Wl, int C, int p, int Fo) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_out) return;
  const int gw = Wl / p, S_i = (Hl / p) * gw, pp = p * p, Fz = pp * C;
  const int f = (int)(i % Fo);
  const long row = i / Fo;
  const int t = (int)(row % S_i), img = (int)(row / S_i);
  const int g = f < Fz ? f : f - Fz;  // (channel, ph, pw) of the latent, or of the unshuffled mask
  const int ch = g / pp, yy = (t / gw) * p + (g / p) % p, xx = (t % gw) * p + g % p;
  float v;
  if (f < Fz) {
    v = z[(((size_t)img * Hl + yy) * Wl + xx) * C + ch];
  } else {
    const size_t W8 = (size_t)Wl * 8;
    v = (float)mask[((size_t)(mask_per_image ? img : 0) * Hl * 8 + (size_t)yy * 8 + ch / 8) * W8 + (size_t)xx * 8 + ch % 8] / 255.0f;
  }
  tok[i] = f2bf(v);
}
int dk_launch_fill_condition_tokens(const float* z, const unsigned char* mask, bf16_t* tok, int n, int mask_per_image, int Hl, int Wl, int C,
                                    int p, hipStream_t stream) {
  const int Fo = p * p * C + (mask ? 64 * p * p : 0);
  const long n_out = (long)n * (Hl / p) * (Wl / p) * Fo;
  DK_REQUIRE(n_out > 0 && (n_out + 255) / 256 <= 0x7fffffffL, "fill_condition_tokens: size");
  hipLaunchKernelGGL(dk_fill_condition_tokens_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, stream, z, mask, tok, n_out,
                     mask_per_image, Hl, Wl, C, p, Fo);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}
#endif  // !DK_ELEM_F16

// ---------------------------------------------------------------------------------------------
// Patchify: latent [n_img, Hl, Wl, C] fp32 -> tokens [n_img*dup, S_i, p*p*C] bf16.
// reshape_order=1: FLUX space-to-depth, features (c, ph, pw) (mmdit.py:292-300);
// reshape_order=0: SD3 strided conv taps, features (ph, pw, c) (mmdit.py:285-290).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int patch_feature(int c, int ph, int pw, int C, int p, int reshape_order) {
  return reshape_order ? (c * p * p + ph * p + pw) : ((ph * p + pw) * C + c);
}
// The statements the patchify and step kernels share, written once.  The index r of an element inside its image's latent (long, or int where
// the caller has checked the range) -> its cell, token and feature, and the token grid's sizes ...
struct StepCell {
  int img, yy, xx, t, f, S_i, F;
};
template <class I>
__device__ __forceinline__ StepCell step_cell(int img, I r, int Hl, int Wl, int C, int p, int reshape_order) {
  StepCell k;
  k.img = img;
  const int c = (int)(r % C);
  r /= C;
  k.xx = (int)(r % Wl), k.yy = (int)(r / Wl);
  const int gw = Wl / p;
  k.S_i = (Hl / p) * gw, k.F = p * p * C;
  k.t = (k.yy / p) * gw + (k.xx / p);
  k.f = patch_feature(c, k.yy % p, k.xx % p, C, p, reshape_order);
  return k;
}
// ... the x0 prediction of batch row `row` at the element's token and feature: the value the denoiser saw minus sigma times the model's output
// (this one and the blend take the cell's fields one by one: handed the StepCell, the moments kernel and the masked step kernels come out of
// the compiler with their instructions in another order, and the objects' .text is held byte for byte, scripts/device_code_diff.py) ...
__device__ __forceinline__ float step_den(const bf16_t* model_out, int ld_out, int row, int S_i, int t, int f, float xb, float sigma) {
  return xb - to_f32(model_out[((size_t)row * S_i + t) * ld_out + f]) * sigma;
}
// ... the inpainting blend of the updated value with the known region re-noised to sigma_next (dk_euler_step_kernel's comment) ...
__device__ __forceinline__ float step_blend(float xn, long i, int img, int yy, int xx, int Hl, int Wl, float sigma_next, const float* x_orig,
                                            const float* noise, const float* mask, int mask_per_image) {
  const float m = mask[(mask_per_image ? (long)img * Hl * Wl : 0) + (long)yy * Wl + xx];
  const float known = sigma_next * noise[i] + (1.0f - sigma_next) * x_orig[i];
  return m * xn + (1.0f - m) * known;
}
// ... and the store of the updated value: x in fp32, its rounding into the tokens of the prompt row and, under CFG, of the negative row.
__device__ __forceinline__ void step_store(float* x, bf16_t* tok, long i, float xn, const StepCell& k, int n_img, int cfg_on) {
  x[i] = xn;
  const bf16_t nb = from_f32(xn);
  tok[((size_t)k.img * k.S_i + k.t) * k.F + k.f] = nb;
  if (cfg_on) tok[((size_t)(n_img + k.img) * k.S_i + k.t) * k.F + k.f] = nb;
}
__global__ void dk_latent_to_tokens_kernel(const float* x, bf16_t* tok, int n_img, int dup, int Hl, int Wl, int C, int p,
                                           int reshape_order) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per_img = (long)Hl * Wl * C;
  if (i >= per_img * n_img) return;
  const StepCell k = step_cell((int)(i / per_img), i % per_img, Hl, Wl, C, p, reshape_order);
  const bf16_t v = from_f32(x[i]);
  for (int d = 0; d < dup; ++d) tok[((size_t)(d * n_img + k.img) * k.S_i + k.t) * k.F + k.f] = v;
}
int dk_launch_latent_to_tokens(const float* x, bf16_t* tok, int n_img, int dup, int Hl, int Wl, int C, int p, int reshape_order,
                               hipStream_t stream) {
  const long n = (long)n_img * Hl * Wl * C;
  hipLaunchKernelGGL(dk_latent_to_tokens_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, tok, n_img, dup, Hl,
                     Wl, C, p, reshape_order);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Fused step-loop tail: unpatchify + x0 prediction + CFG + Euler update + re-patchify.
// reference: CFGDenoiser.__call__ python/src/diffusionkit/mlx/__init__.py:691-719
// (x_bf16 - out*sigma in fp32; neg + w*(text - neg)), to_d :756, sample_euler :778-781;
// unpack/unpatchify mmdit.py:304-321, 975-988.  x stays fp32 (quirk Q6).
// MASKED (inpainting, no reference counterpart): the updated latent is blended with the known region re-noised to sigma_next,
//   known = sigma_next * noise + (1 - sigma_next) * x_orig,  x = m * x_new + (1 - m) * known,
// m = mask[img or 0][yy][xx] in [0, 1], the same for the C channels of a cell.  The two-product form is exact at both ends whatever
// is contracted into FMAs: m == 1 gives x_new, m == 0 gives known, and sigma_next == 0 makes known = x_orig, bit for bit for finite inputs -- but
// for the sign of a zero: the vanishing product is +-0, and -0 + (+0) = +0, so a value of -0.0f at an exact end may come out as +0.0f.
// The tokens are the rounding of the blended value.  MASKED = false: the mask operands are not read, same arithmetic as before.
// ---------------------------------------------------------------------------------------------
template <bool MASKED>
__global__ void dk_euler_step_kernel(float* x, const bf16_t* model_out, int ld_out, bf16_t* tok, int n_img, int cfg_on, int Hl,
                                     int Wl, int C, int p, int reshape_order, float sigma, float sigma_next, float cfg_weight,
                                     const float* x_orig, const float* noise, const float* mask, int mask_per_image) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per_img = (long)Hl * Wl * C;
  if (i >= per_img * n_img) return;
  const StepCell k = step_cell((int)(i / per_img), i % per_img, Hl, Wl, C, p, reshape_order);
  const float xv = x[i];
  const float xb = round_act(xv);  // the value the denoiser saw
  float den = step_den(model_out, ld_out, k.img, k.S_i, k.t, k.f, xb, sigma);
  if (cfg_on) {
    const float den_neg = step_den(model_out, ld_out, n_img + k.img, k.S_i, k.t, k.f, xb, sigma);
    den = den_neg + cfg_weight * (den - den_neg);
  }
  const float d = (xv - den) / sigma;
  float xn = xv + d * (sigma_next - sigma);
  if constexpr (MASKED) {
    xn = step_blend(xn, i, k.img, k.yy, k.xx, Hl, Wl, sigma_next, x_orig, noise, mask, mask_per_image);
  }
  step_store(x, tok, i, xn, k, n_img, cfg_on);
}

// ---------------------------------------------------------------------------------------------
// Second-order samplers (Heun, Adams-Bashforth 2; no reference counterpart): the step-loop tail above with the update written as a
// coefficient row over one fp32 history buffer H shaped like the latent,
//   d = (x - den) / sigma,    x' = cx * x + cd * d + ch * H,    H' = hx * x + hd * d,
// den formed as dk_euler_step_kernel forms it (step_den on the same round_act; the same CFG combine and rounding points).  The host writes
// the rows (sampler.step_plan); sigma is the sigma the model was evaluated at, sigma_next the one the row's result lives at (only the
// blend reads it).  reads_h == 0: H is not read (the caller never initialises it) and ch is ignored; writes_h == 0: H is not written.
// A first-order row -- reads_h == 0 and cx == 1 -- is evaluated as the Euler expression itself, x + d * cd: with cd = sigma_next - sigma
// (the fp32 difference dk_euler_step_kernel takes on the device) it is that kernel's statement on that kernel's operands, so x and the
// tokens are its bits whether or not the compiler contracts the product into the sum; cx * x + d * cd would depend on which of the two
// products a contraction swallows.  H' is taken from x BEFORE the update.
// MASKED: dk_euler_step_kernel's two-product blend (step_blend) behind the update, known at sigma_next, with the same exact ends.
// ---------------------------------------------------------------------------------------------
struct LmsRow {
  float cx, cd, ch, hx, hd;
  int reads_h, writes_h;
};
// Guidance modes (include/dk_hip.h; no reference counterpart).  GMODE = DK_GUIDE_CFG is the kernel as it was: gd is not read.  With c = den
// of the prompt row and u = den of the negative row, formed as above:
//   RESCALE  g = u + w (c - u),  den = g * s                      s = scal[2 img]               (s == 1.0f: the CFG step bit for bit)
//   APG      D = (c - u) [+ beta * M],  den = c + (w - 1)(a D - b c)   (a, b) = scal[2 img], scal[2 img + 1]
// The per-image scalars come from the moments pass below, which forms c, u, g and D by the same expressions.  M (fp32, shaped like the latent)
// follows hist's discipline: read only under reads_m, written (M' = D) only under writes_m, each element by the thread that read it.
// Skip-layer guidance (SLG, include/dk_hip.h: dk_slg_cfg_step): model_out holds a third row group [2 n_img, 3 n_img), the evaluation with blocks
// skipped; with k its x0 prediction, formed by step_den like c and u, the mode's den takes one more term, den + slg_scale * (c - k).  The tokens
// are stored as ever, in the two live copies.  SLG = false is the kernel as it was: the third group and slg_scale are not read.
enum { DK_GUIDE_CFG = 0, DK_GUIDE_RESCALE = 1, DK_GUIDE_APG = 2 };
struct GuideArgs {
  const float* scal;
  float* m;
  float beta;
  int reads_m, writes_m;
  float slg_scale;  // (in the struct's tail padding: the argument layout of every instantiation stays)
};
// Stochastic samplers (include/dk_hip.h: dk_noisy_cfg_step): behind the update and in front of the blend, x' takes cn * xi, xi =
// philox_normal(seeds[img], r / 4, draw, 0, r % 4) with r the element's index inside its image -- the operator's function on the operator's
// arguments, formed in registers: no noise buffer is read or written.  The term lives in kernels of its own, dk_lms_noisy_step_kernel, whose body is
// the text of dk_lms_step_kernel's (lms_step_body.inc): the argument layout and the instructions of that kernel's instantiations stay.
struct NoiseArgs {
  float cn;
  const unsigned long long* seeds;
  unsigned draw;
};
template <bool MASKED, int GMODE = DK_GUIDE_CFG, bool SLG = false>
__global__ void dk_lms_step_kernel(float* x, const bf16_t* model_out, int ld_out, bf16_t* tok, int n_img, int cfg_on, int Hl, int Wl,
                                   int C, int p, int reshape_order, float sigma, float sigma_next, float cfg_weight, float* hist,
                                   LmsRow row, const float* x_orig, const float* noise, const float* mask, int mask_per_image,
                                   GuideArgs gd) {
  constexpr bool NOISY = false;
  constexpr NoiseArgs nz = {};  // (named by the included text, never read)
#include "lms_step_body.inc"
}
template <bool MASKED, int GMODE, bool SLG>
__global__ void dk_lms_noisy_step_kernel(float* x, const bf16_t* model_out, int ld_out, bf16_t* tok, int n_img, int cfg_on, int Hl, int Wl,
                                         int C, int p, int reshape_order, float sigma, float sigma_next, float cfg_weight, float* hist,
                                         LmsRow row, const float* x_orig, const float* noise, const float* mask, int mask_per_image,
                                         GuideArgs gd, NoiseArgs nz) {
  constexpr bool NOISY = true;
#include "lms_step_body.inc"
}

// ---------------------------------------------------------------------------------------------
// Guidance moments (no reference counterpart): the per-image sums the guided step needs, and the scalars they end in.
// Pass 1: grid (nb, n_img), 256 threads -- a workgroup never leaves its image.  Thread t of block b takes the elements b * 256 + t,
// + nb * 256, ... of the image, in that order, forms c and u by step_den, g or D as dk_lms_step_kernel does, and adds its terms in fp32; wave_sum
// folds the lanes in a fixed butterfly; the four wave partials go through LDS and thread 0 adds them in fp64, in wave order, into
// part[img][b][4].  RESCALE: (sum c, sum g, sum c^2, sum g^2); APG: (sum D^2, sum D c, sum c^2, 0).
// Pass 2: one wave per image, lane l adds blocks l, l + 64, ... in that order in fp64, a fixed butterfly folds the lanes, lane 0 writes
//   RESCALE  s = phi * std(c) / std(g) + (1 - phi)   (std(g) == 0: s = 1; phi == 0: s = 1.0f exactly)
//   APG      a = min(1, r / |D|) (r <= 0 or |D| == 0: 1),   b = (1 - eta) a <D, c> / <c, c>  (<c, c> == 0: 0)
// as scal[2 img], scal[2 img + 1].  No atomics: the same bits on every run.  The workspace: part (fp64) [n_img][nb][4], then scal (fp32)
// [n_img][2]; every element read is written first.
// ---------------------------------------------------------------------------------------------
static inline int guide_blocks(long per_img) {
  const long nb = (per_img + 1023) / 1024;
  return (int)(nb < 1 ? 1 : nb > 1024 ? 1024 : nb);
}
size_t dk_guidance_workspace_size(int n_img, int Hl, int Wl, int C) {
  const long per_img = (long)Hl * Wl * C;
  return (size_t)n_img * guide_blocks(per_img) * 4 * sizeof(double) + (size_t)n_img * 2 * sizeof(float);
}
template <int GMODE>
__global__ __launch_bounds__(256) void dk_guide_moments_kernel(const float* x, const bf16_t* model_out, int ld_out, int n_img, int Hl, int Wl,
                                                               int C, int p, int reshape_order, float sigma, float cfg_weight,
                                                               const float* m, float beta, int reads_m, double* part) {
  __shared__ float wpart[4][4];
  const int img = blockIdx.y, nb = gridDim.x;
  const int per_img = Hl * Wl * C;  // (< 2^31: checked by the launcher)
  const int gw = Wl / p, S_i = (Hl / p) * gw;  // (step_cell's S_i, taken in front of the loop: inside it the instructions move)
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int j = (int)blockIdx.x * 256 + (int)threadIdx.x; j < per_img; j += nb * 256) {
    const long i = (long)img * per_img + j;
    const StepCell k = step_cell(img, j, Hl, Wl, C, p, reshape_order);
    const float xb = round_act(x[i]);
    const float den = step_den(model_out, ld_out, img, S_i, k.t, k.f, xb, sigma);
    const float den_neg = step_den(model_out, ld_out, n_img + img, S_i, k.t, k.f, xb, sigma);
    if constexpr (GMODE == DK_GUIDE_RESCALE) {
      const float g = den_neg + cfg_weight * (den - den_neg);
      s0 += den;
      s1 += g;
      s2 += den * den;
      s3 += g * g;
    } else {
      float dl = den - den_neg;
      if (reads_m) dl = dl + beta * m[i];
      s0 += dl * dl;
      s1 += dl * den;
      s2 += den * den;
    }
  }
  s0 = wave_sum(s0);
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  s3 = wave_sum(s3);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    wpart[wave][0] = s0;
    wpart[wave][1] = s1;
    wpart[wave][2] = s2;
    wpart[wave][3] = s3;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    double acc = (double)wpart[0][k];
    for (int w = 1; w < 4; ++w) acc += (double)wpart[w][k];
    part[((size_t)img * nb + blockIdx.x) * 4 + k] = acc;
  }
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int GMODE>
__global__ __launch_bounds__(64) void dk_guide_fold_kernel(const double* part, float* scal, int nb, double n_elem, float phi, float eta,
                                                           float thr) {
  const int img = blockIdx.x, lane = threadIdx.x;
  const double* pp = part + (size_t)img * nb * 4;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = lane; b < nb; b += 64) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += pp[(size_t)b * 4 + k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = wave_sum_f64(s[k]);
  if (lane != 0) return;
  float o0, o1 = 0.f;
  if constexpr (GMODE == DK_GUIDE_RESCALE) {
    const double mc = s[0] / n_elem, mg = s[1] / n_elem;
    double vc = s[2] / n_elem - mc * mc, vg = s[3] / n_elem - mg * mg;
    vc = vc > 0.0 ? vc : 0.0;
    vg = vg > 0.0 ? vg : 0.0;
    o0 = (phi == 0.f || !(vg > 0.0)) ? 1.0f : (float)((double)phi * sqrt(vc / vg) + (1.0 - (double)phi));
  } else {
    const double nd = sqrt(s[0]);
    const double a = (thr > 0.f && nd > 0.0 && (double)thr < nd) ? (double)thr / nd : 1.0;
    o0 = (float)a;
    o1 = s[2] > 0.0 ? (float)((1.0 - (double)eta) * a * s[1] / s[2]) : 0.0f;
  }
  *(float2*)(scal + 2 * img) = make_float2(o0, o1);
}
// The one launcher of the step tail (StepParams, dk_elem_launchers.h): the Euler kernel without a row, else the row kernel of the block's
// (masked, mode), behind the two moments launches under modes 1 and 2.  What an instantiation does not read (the blend operands unmasked, gd
// under mode 0) is passed as the block holds it.  The instantiations are named in the order the object has always held them: its .text is
// compared byte for byte across host-only changes (scripts/device_code_diff.py).  The skip-layer forms of the row kernel come behind them, and the
// noisy kernel's twelve (masked x mode x skip-layer) behind those.
int dk_launch_step(const StepParams& s, hipStream_t stream) {
  const long per_img = (long)s.Hl * s.Wl * s.C;
  const long n = (long)s.n_img * per_img;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (!s.has_row) {
    const auto kernel = !s.masked ? dk_euler_step_kernel<false> : dk_euler_step_kernel<true>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, s.x, s.model_out, s.ld_out, s.tok, s.n_img, s.cfg_on, s.Hl, s.Wl, s.C, s.p,
                       s.reshape_order, s.sigma, s.sigma_next, s.cfg_weight, s.x_orig, s.noise, s.mask, (int)s.mask_per_image);
    DK_CHECK_HIP(hipGetLastError());
    return 0;
  }
  auto kernel = s.masked ? dk_lms_step_kernel<true> : dk_lms_step_kernel<false>;
  float* scal = nullptr;
  if (s.mode != DK_GUIDE_CFG) {
    void* const workspace = s.workspace;
    DK_REQUIRE(per_img < (1L << 31) - 1024L * 256, "the latent of one image must hold fewer than 2^31 elements");
    DK_REQUIRE(((uintptr_t)workspace & 7) == 0, "the guidance workspace must be 8-byte aligned");
    const int nb = guide_blocks(per_img);
    double* part = (double*)workspace;
    scal = (float*)(part + (size_t)s.n_img * nb * 4);
    const dim3 mgrid((unsigned)nb, (unsigned)s.n_img);
    const bool rescale = s.mode == DK_GUIDE_RESCALE;
    auto moments = dk_guide_moments_kernel<DK_GUIDE_RESCALE>;
    auto fold = dk_guide_fold_kernel<DK_GUIDE_RESCALE>;
    if (!rescale) moments = dk_guide_moments_kernel<DK_GUIDE_APG>, fold = dk_guide_fold_kernel<DK_GUIDE_APG>;
    if (rescale)
      kernel = s.masked ? dk_lms_step_kernel<true, DK_GUIDE_RESCALE> : dk_lms_step_kernel<false, DK_GUIDE_RESCALE>;
    else
      kernel = s.masked ? dk_lms_step_kernel<true, DK_GUIDE_APG> : dk_lms_step_kernel<false, DK_GUIDE_APG>;
    hipLaunchKernelGGL(moments, mgrid, dim3(256), 0, stream, s.x, s.model_out, s.ld_out, s.n_img, s.Hl, s.Wl, s.C, s.p, s.reshape_order, s.sigma,
                       s.cfg_weight, s.m, s.beta, (int)s.reads_m, part);
    DK_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(fold, dim3(s.n_img), dim3(64), 0, stream, part, scal, nb, (double)per_img, s.phi, s.eta, s.r);
    DK_CHECK_HIP(hipGetLastError());
  }
  if (s.slg) {  // (the moments above read rows [0, 2 n_img) and are the mode's own)
    if (s.mode == DK_GUIDE_CFG)
      kernel = s.masked ? dk_lms_step_kernel<true, DK_GUIDE_CFG, true> : dk_lms_step_kernel<false, DK_GUIDE_CFG, true>;
    else if (s.mode == DK_GUIDE_RESCALE)
      kernel = s.masked ? dk_lms_step_kernel<true, DK_GUIDE_RESCALE, true> : dk_lms_step_kernel<false, DK_GUIDE_RESCALE, true>;
    else
      kernel = s.masked ? dk_lms_step_kernel<true, DK_GUIDE_APG, true> : dk_lms_step_kernel<false, DK_GUIDE_APG, true>;
  }
  const LmsRow row = {s.cx, s.cd, s.ch, s.hx, s.hd, s.reads_h, s.writes_h};
  const GuideArgs gd = {scal, s.m, s.beta, s.reads_m, s.writes_m, s.slg_scale};
  if (s.cn != 0.0f) {  // (the row carries a noise term: the same case of the noisy kernel, behind the same moments; cn == 0 is the launch below)
#define DK_NOISY(MODE) {{dk_lms_noisy_step_kernel<false, MODE, false>, dk_lms_noisy_step_kernel<false, MODE, true>}, \
                        {dk_lms_noisy_step_kernel<true, MODE, false>, dk_lms_noisy_step_kernel<true, MODE, true>}}
    static const decltype(&dk_lms_noisy_step_kernel<false, DK_GUIDE_CFG, false>) noisy[3][2][2] = {DK_NOISY(DK_GUIDE_CFG), DK_NOISY(DK_GUIDE_RESCALE),
                                                                                                  DK_NOISY(DK_GUIDE_APG)};
#undef DK_NOISY
    const NoiseArgs nz = {s.cn, s.seeds, (unsigned)s.draw};
    hipLaunchKernelGGL(noisy[s.mode][s.masked][s.slg], grid, dim3(256), 0, stream, s.x, s.model_out, s.ld_out, s.tok, s.n_img, s.cfg_on, s.Hl, s.Wl, s.C,
                       s.p, s.reshape_order, s.sigma, s.sigma_next, s.cfg_weight, s.hist, row, s.x_orig, s.noise, s.mask, (int)s.mask_per_image, gd, nz);
    DK_CHECK_HIP(hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, s.x, s.model_out, s.ld_out, s.tok, s.n_img, s.cfg_on, s.Hl, s.Wl, s.C, s.p, s.reshape_order,
                     s.sigma, s.sigma_next, s.cfg_weight, s.hist, row, s.x_orig, s.noise, s.mask, (int)s.mask_per_image, gd);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------
// First-block cache (include/dk_hip.h; no reference counterpart): what block 0 did to the image rows of the joint stream, compared
// with what it did in the last computed step, and the cached effect of the blocks behind it.  fp32 arithmetic, one rounding to the
// element type per stored value.
// Probe: one wave per image row, 4 rows per workgroup, the row's three operands loaded up front as in dk_ln_modulate_kernel (buffer
// loads whose resource spans one row: lanes past the row end read zeros, their stores are dropped).  d holds X0's row on entry and
// D_cur = round(x - d) on return; (num, den) = (sum |D_cur - D_ref|, sum |D_ref|) of the row: each lane adds its elements in index order,
// wave_sum folds the lanes in a fixed butterfly -- no atomics, the same bits on every run.  A null d_ref is a resource of zero bytes: it
// reads as zeros, den = 0.
// ---------------------------------------------------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(256) void dk_block_probe_kernel(const bf16_t* x, int ldx, int x_seg_len, int x_seg_stride, bf16_t* d,
                                                             const bf16_t* d_ref, float* row_partials, int M, int h) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = (int)blockIdx.x * 4 + wave;
  if (m >= M) return;
  const size_t xrow = (size_t)((m / x_seg_len) * x_seg_stride + (m % x_seg_len)) * ldx;
  bf16_t* drow = d + (size_t)m * h;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(x + xrow), 0, h * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc((void*)drow, 0, h * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rr =
      __builtin_amdgcn_make_buffer_rsrc(d_ref ? (void*)(d_ref + (size_t)m * h) : (void*)drow, 0, d_ref ? h * 2 : 0, 0x00020000);
  u32x4 a[NCH], p[NCH], r[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) a[i] = __builtin_amdgcn_raw_buffer_load_b128(rx, (lane + 64 * i) * 16, 0, 0);
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    p[i] = __builtin_amdgcn_raw_buffer_load_b128(rd, (lane + 64 * i) * 16, 0, 0);
    r[i] = __builtin_amdgcn_raw_buffer_load_b128(rr, (lane + 64 * i) * 16, 0, 0);
  }
  __builtin_amdgcn_sched_barrier(0);  // (without it the scheduler sinks some of the loads of d below the first stores to it)
  float num = 0.f, den = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float a0, a1, p0, p1, r0, r1, d0, d1;
      unpack2(a[i][e], a0, a1);
      unpack2(p[i][e], p0, p1);
      unpack2(r[i][e], r0, r1);
      o[e] = pack2(a0 - p0, a1 - p1);
      unpack2(o[e], d0, d1);  // (the stored, rounded difference is what is compared)
      num += fabsf(d0 - r0);
      num += fabsf(d1 - r1);
      den += fabsf(r0);
      den += fabsf(r1);
    }
    __builtin_amdgcn_raw_buffer_store_b128(o, rd, (lane + 64 * i) * 16, 0, 0);
  }
  num = wave_sum(num);
  den = wave_sum(den);
  if (lane == 0) {
    row_partials[2 * (size_t)m] = num;
    row_partials[2 * (size_t)m + 1] = den;
  }
}
// ... and the rows of one batch row: one wave per batch row, lane l adds rows l, l + 64, ... in that order, wave_sum folds the lanes
__global__ __launch_bounds__(64) void dk_block_probe_fold_kernel(const float* row_partials, float* probe, int rows_per_batch) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* p = row_partials + 2 * (size_t)b * rows_per_batch;
  float num = 0.f, den = 0.f;
  int r = lane;
  for (; r + 7 * 64 < rows_per_batch; r += 8 * 64) {  // (eight independent loads in flight, the additions in the same order as one by one)
    float2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *(const float2*)(p + 2 * (size_t)(r + 64 * u));
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      num += v[u].x;
      den += v[u].y;
    }
  }
  for (; r < rows_per_batch; r += 64) {
    num += p[2 * (size_t)r];
    den += p[2 * (size_t)r + 1];
  }
  num = wave_sum(num);
  den = wave_sum(den);
  if (lane == 0) {
    probe[2 * b] = num;
    probe[2 * b + 1] = den;
  }
}
static int check_block_rows(const void* x, int ldx, int x_seg_len, const void* dense, int M, int h) {
  DK_REQUIRE(h > 0 && h % 8 == 0 && h <= 4096, "hidden size must be a multiple of 8 (rows move as 16-byte vectors) and <= 4096");
  DK_REQUIRE(x != nullptr && dense != nullptr && M > 0 && x_seg_len > 0, "null / empty argument");
  DK_REQUIRE(ldx % 8 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)dense & 15) == 0, "rows must keep 16-byte alignment");
  return 0;
}
int dk_launch_block_probe(const bf16_t* x, int ldx, int x_seg_len, int x_seg_stride, bf16_t* d, const bf16_t* d_ref, float* row_partials,
                          float* probe, int M, int h, int rows_per_batch, hipStream_t stream) {
  if (const int rc = check_block_rows(x, ldx, x_seg_len, d, M, h)) return rc;
  DK_REQUIRE(row_partials != nullptr && probe != nullptr && ((uintptr_t)d_ref & 15) == 0 && ((uintptr_t)row_partials & 7) == 0,
             "null / misaligned argument");
  DK_REQUIRE(rows_per_batch > 0 && M % rows_per_batch == 0, "the rows must be whole batch rows of rows_per_batch rows");
  dim3 grid((M + 3) / 4), block(256);
#define PROBE_CASE(N)                                                                                                                   \
  case N:                                                                                                                               \
    hipLaunchKernelGGL(dk_block_probe_kernel<N>, grid, block, 0, stream, x, ldx, x_seg_len, x_seg_stride, d, d_ref, row_partials, M, h); \
    break;
  switch ((h / 8 + 63) / 64) {
    PROBE_CASE(1) PROBE_CASE(2) PROBE_CASE(3) PROBE_CASE(4) PROBE_CASE(5) PROBE_CASE(6) PROBE_CASE(7) PROBE_CASE(8)
    default: DK_REQUIRE(false, "unsupported hidden size");
  }
#undef PROBE_CASE
  DK_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(dk_block_probe_fold_kernel, dim3(M / rows_per_batch), dim3(64), 0, stream, row_partials, probe, rows_per_batch);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}

// REUSE false: r = round(x - r), in place over the saved X1 (x is read only); true: x = round(x + r).  One 16-byte chunk per thread;
// x through the row map, r dense [M, h].
template <bool REUSE>
__global__ __launch_bounds__(256) void dk_block_residual_kernel(bf16_t* x, int ldx, int x_seg_len, int x_seg_stride, bf16_t* r, int M, int cpr) {
  const unsigned gid = blockIdx.x * 256u + threadIdx.x;  // (32-bit: M * cpr < 2^31, checked by the launcher)
  if (gid >= (unsigned)M * (unsigned)cpr) return;
  const int m = (int)(gid / (unsigned)cpr), c = (int)(gid - (unsigned)m * (unsigned)cpr);
  bf16_t* xp = x + (size_t)((m / x_seg_len) * x_seg_stride + (m % x_seg_len)) * ldx + c * 8;
  bf16_t* rp = r + ((size_t)m * cpr + c) * 8;
  const u32x4 a = *(const u32x4*)xp, b = *(const u32x4*)rp;
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float a0, a1, b0, b1;
    unpack2(a[e], a0, a1);
    unpack2(b[e], b0, b1);
    o[e] = REUSE ? pack2(a0 + b0, a1 + b1) : pack2(a0 - b0, a1 - b1);
  }
  *(u32x4*)(REUSE ? xp : rp) = o;
}
int dk_launch_block_residual(bf16_t* x, int ldx, int x_seg_len, int x_seg_stride, bf16_t* r, int M, int h, bool reuse, hipStream_t stream) {
  if (const int rc = check_block_rows(x, ldx, x_seg_len, r, M, h)) return rc;
  const int cpr = h / 8;
  DK_REQUIRE((long)M * cpr < (1L << 31) - 256, "block_residual: rows * h / 8 must stay below 2^31");
  dim3 grid((unsigned)(((long)M * cpr + 255) / 256)), block(256);
  if (reuse)
    hipLaunchKernelGGL(dk_block_residual_kernel<true>, grid, block, 0, stream, x, ldx, x_seg_len, x_seg_stride, r, M, cpr);
  else
    hipLaunchKernelGGL(dk_block_residual_kernel<false>, grid, block, 0, stream, x, ldx, x_seg_len, x_seg_stride, r, M, cpr);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------
// FlowEdit (include/dk_hip.h: dk_flowedit_step; Kulikov et al. 2024; no reference counterpart): the step of an edit loop whose state Z starts at
// the encoded source image x_src and moves by the difference of two evaluations of the model, one on a noised source Zs with the source prompt
// and one on Zt = Zs + (Z - x_src) with the target prompt,
//   Z' = Z + c (V_tar - V_src),   xi = philox_normal(seeds[img], r / 4, draw, stream 1, r % 4),
//   Zs = (1 - sigma_in) x_src + sigma_in xi,   Zt = Zs + (Z' - x_src),
// V the model's output itself, under CFG neg + w (pos - neg) with a weight per side.  Batch rows of model_out and tok, n_img each:
// [src | tar] or [src+ | tar+ | src- | tar-].  prime: model_out is not read and Z is neither changed nor written (the launch that forms the
// first inputs).  Zs and Zt leave in fp32 (zs_out may be null) and, rounded, as the tokens of the source and target rows -- under CFG of both
// copies, dk_latent_to_tokens's layout for 2 n_img images.
// One thread per Philox quad: the four elements r .. r + 3 are four channels of one cell (C % 4 == 0), so the fp32 operands move as 16-byte
// accesses, the ten rounds run once per quad instead of once per element, and with the SD3 patch order (features (ph, pw, c)) the four
// features are neighbours too: one 8-byte access per batch row.  FLUX's order (c, ph, pw) spreads them p * p apart: four 2-byte accesses
// inside one token's row.  Z + c * 0 and Zs + 0 are exact: equal source and target rows with equal weights leave Z's bits, and Z == x_src
// gives Zt the bits of Zs (but for the sign of a zero).
// ---------------------------------------------------------------------------------------------
struct FlowEditArgs {
  float w_src, w_tar, c, sigma_in;
  const unsigned long long* seeds;
  unsigned draw;
  int prime;
};
struct Quad16 {
  bf16_t v[4];
};
// the four features of a quad in batch row `row`: f0, f0 + fs, ...; fs == 1 takes them in one access (8-byte aligned: the launcher's checks)
__device__ __forceinline__ void flowedit_load(const bf16_t* base, int fs, float* o) {
  if (fs == 1) {
    const Quad16 q = *(const Quad16*)__builtin_assume_aligned(base, 8);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = to_f32(q.v[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = to_f32(base[j * fs]);
  }
}
__device__ __forceinline__ void flowedit_store(bf16_t* base, int fs, const Quad16& q) {
  if (fs == 1) {
    *(Quad16*)__builtin_assume_aligned(base, 8) = q;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) base[j * fs] = q.v[j];
  }
}
__global__ __launch_bounds__(256) void dk_flowedit_step_kernel(float* z, const float* x_src, const bf16_t* model_out, int ld_out, bf16_t* tok,
                                                               float* zs_out, float* zt_out, int n_img, int cfg_on, int Hl, int Wl, int C, int p,
                                                               int reshape_order, FlowEditArgs a) {
  const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long quads_per_img = (long)Hl * Wl * C / 4;
  if (q >= quads_per_img * n_img) return;
  const int img = (int)(q / quads_per_img);
  const long qi = q % quads_per_img;
  const long i = q * 4;
  const StepCell k = step_cell(img, qi * 4, Hl, Wl, C, p, reshape_order);  // (of the quad's first element; the other three: the next channels)
  const int fs = reshape_order ? p * p : 1;
  const float4 xs = *(const float4*)(x_src + i);
  float4 zv = *(const float4*)(z + i);
  float zz[4] = {zv.x, zv.y, zv.z, zv.w};
  const float xx[4] = {xs.x, xs.y, xs.z, xs.w};
  if (!a.prime) {
    const size_t at = ((size_t)img * k.S_i + k.t) * ld_out + k.f, group = (size_t)n_img * k.S_i * ld_out;  // (row b: at + b * group)
    float vs[4], vt[4];
    flowedit_load(model_out + at, fs, vs);
    flowedit_load(model_out + at + group, fs, vt);
    if (cfg_on) {
      float ns[4], nt[4];
      flowedit_load(model_out + at + 2 * group, fs, ns);
      flowedit_load(model_out + at + 3 * group, fs, nt);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        vs[j] = ns[j] + a.w_src * (vs[j] - ns[j]);
        vt[j] = nt[j] + a.w_tar * (vt[j] - nt[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) zz[j] = zz[j] + a.c * (vt[j] - vs[j]);
    *(float4*)(z + i) = make_float4(zz[0], zz[1], zz[2], zz[3]);
  }
  const unsigned long long seed = a.seeds[img];
  const float keep = 1.0f - a.sigma_in;
  float zs[4], zt[4];
  Quad16 ts, tt;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float xi = philox_normal(seed, (unsigned long long)qi, a.draw, 1u, j);
    zs[j] = keep * xx[j] + a.sigma_in * xi;
    zt[j] = zs[j] + (zz[j] - xx[j]);
    ts.v[j] = from_f32(zs[j]);
    tt.v[j] = from_f32(zt[j]);
  }
  if (zs_out) *(float4*)(zs_out + i) = make_float4(zs[0], zs[1], zs[2], zs[3]);
  *(float4*)(zt_out + i) = make_float4(zt[0], zt[1], zt[2], zt[3]);
  const size_t tat = ((size_t)img * k.S_i + k.t) * k.F + k.f, tgroup = (size_t)n_img * k.S_i * k.F;
  flowedit_store(tok + tat, fs, ts);
  flowedit_store(tok + tat + tgroup, fs, tt);
  if (cfg_on) {
    flowedit_store(tok + tat + 2 * tgroup, fs, ts);
    flowedit_store(tok + tat + 3 * tgroup, fs, tt);
  }
}
int dk_launch_flowedit_step(const FlowEditParams& s, hipStream_t stream) {
  const long n_quads = (long)s.n_img * s.Hl * s.Wl * s.C / 4;
  DK_REQUIRE((n_quads + 255) / 256 <= 0x7fffffffL, "flowedit_step: size");
  const FlowEditArgs a = {s.w_src, s.w_tar, s.c, s.sigma_in, s.seeds, (unsigned)s.draw, s.prime};
  hipLaunchKernelGGL(dk_flowedit_step_kernel, dim3((unsigned)((n_quads + 255) / 256)), dim3(256), 0, stream, s.z, s.x_src, s.model_out, s.ld_out, s.tok,
                     s.zs_out, s.zt_out, s.n_img, s.cfg_on, s.Hl, s.Wl, s.C, s.p, s.reshape_order, a);
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}
