// Joint text/image attention forward for gfx950: entry point and kernel choice.
//
// Replaces the four mx.fast.scaled_dot_product_attention call sites of the reference
// (python/src/diffusionkit/mlx/mmdit.py:562,643,687,736): softmax(q k^T * scale) v, no mask, non-causal, over the concatenated
// [text, image] sequence.  The reference materialises the [H, S, S] score tensor in the activation dtype (quirk Q4); here scores
// stay fp32 in registers (flash-style, they never leave the CU).
//
// Layout: q/k/v are read in place from the token-major projection output (row stride ld, head h at column h*D), the output is
// written token-major so the o-projection GEMM consumes it directly -- no [B,H,S,D] transposes exist anywhere.
//
// Kernels: attention2.hip (VALU-lean, deferred rescale, 4 waves of 32 queries; D = 64, short sequences, and the only one with a score
// bias) and attention4.hip (the two waves of a SIMD in opposite matrix / vector phases; D = 128, the default on long sequences).
// Round 5 moved what no default path takes to profiles/lab_kernels/ (README there): the software-pipelined D = 128 kernel with its
// balanced stream-K-like launch (attention3_pipelined.hip: 908 / 961 / 978 TF against attention4's 1018 / 1053 / 1078 on FLUX B1 /
// FLUX-dev B1 / FLUX B4), the D = 64 form with two query blocks per wave and the pipelined D = 64 patch (rounds 2-4: all within +-6 %
// of the lean kernel, which is bound by VALU issue, profiles/r04_sd3_pmc.md).
#include "dk_kernels.h"

int g_dk_attn_mode = -1;  // dk_tune_set("attn", v): -1 (default) automatic; 4 = dk_attn2 (4 waves); 9 = dk_attn4 (8 waves, D = 128 only);
                          // 10 = dk_attn5 (one wave per SIMD, asm tile loop; D = 128, S % 256 == 0: other shapes fall back to 9)
int g_dk_attn5_split = -1;  // dk_tune_set("attn_split", v): -1 automatic (needs the workspace), 0 never, 2 .. 4 that many key ranges for the last round's blocks
int g_dk_attn5_track = -1;  // dk_tune_set("attn_track", v): -1 / 0 automatic (the rule below); 1: the one-wave-per-SIMD kernel always keeps its running row maximum

// The largest bound on |scale * q.k| (natural units) under which attention5.hip runs its tile loop WITHOUT the running row maximum: 2 B log2(e) <= 64.
// That body (scripts/gen_attn5.py, program(track=False)) takes the offset m of a row once, from the maximum of the row's first key tile, and forms
// p = 2^((s - m) log2 e) for every key.  With |s| <= B for every score of the launch, m included:
//   * s - m <= 2 B, so p <= 2^(2 B log2 e) <= 2^64, and the row sum l <= S * 2^64 < 2^96 for any S < 2^32 -- fp32 holds 2^127, and so does bf16 (same exponent);
//   * s - m >= -2 B, so no probability falls below 2^-64 (fp32 and bf16 normals reach 2^-126): nothing is flushed that the tracked body would keep,
//     and l >= the first tile's maximum's own p = 1: the final 1 / l is at most 1;
//   * the accumulators hold at most l * max|v| < 2^96 * 2^16 for bf16 values below 2^16.
// softmax does not depend on the offset beyond rounding, so the two bodies agree to the rounding of p (bf16) and of the fp32 sums.  The key-range jobs
// of a split launch leave their own m per row, and dk_attn5_merge_kernel weights the partials by 2^(m_i - max m) <= 1 as before.
static constexpr float DK_ATTN5_UNTRACKED_MAX_ARG = 64.0f;
static constexpr float DK_LOG2E = 1.44269504088896340736f;

// Every decision and argument check of one call (AttnRoute, dk_kernels.h): a pure function of its arguments and the three knobs above -- no HIP call.
// ws_bytes: size of the caller's region for the partial results of the key-split workgroups (0: none)
int dk_attention_route(const AttnParams& p, size_t ws_bytes, int n_cu, AttnRoute& r) {
  DK_REQUIRE(p.D == 128 || p.D == 64, "head_dim must be 64 or 128");
  DK_REQUIRE(p.S > 0 && p.B > 0 && p.H > 0, "empty attention");
  DK_REQUIRE(p.ld % 8 == 0 && p.ldo % 4 == 0, "row strides must keep 16-byte alignment");
  DK_REQUIRE(n_cu > 0, "compute unit count");
  if (p.ident_from != 0) {  // identity attention (AttnParams::ident_from): attention2.hip's IDENT case, bf16 and fp16
    DK_REQUIRE(p.D == 64, "identity attention: head_dim must be 64");
    DK_REQUIRE(p.bias == nullptr, "identity attention: no score bias");
    DK_REQUIRE(p.O8 == nullptr, "identity attention: no MX-fp8 copy of the output");
    DK_REQUIRE(p.ident_from >= 1 && p.ident_from < p.S, "identity attention: 1 <= ident_from < S");
  }
  // automatic choice (kernel lab, profiles/archive/r01_attention_lab.md, r02_attn_bench.log, r03_attention_phase_alternating.md): D = 128 on
  // long sequences: the phase-alternating kernel; otherwise the VALU-lean kernel with 4 waves (D = 64: 842 TF against 773 / 823 for the
  // pipelined forms).  A score bias (text encoders) is only implemented by the lean kernel
  // (round 6, profiles/r06_attention_short_sequences.log: at FLUX's 512 x 512 sequence, S = 1280, the one-wave-per-SIMD kernel wins 16 - 26 % on batches -- 240+
  //  workgroups: a round of the CUs -- and ties on one image in the lab, where the model, with the fused query prologue, measured it 1.6 % per step
  //  behind the lean kernel: below 2048 tokens it takes the launches that fill at least three quarters of a round; at S = 768 the two tie)
  const long blocks = (long)p.B * p.H * ((p.S + 255) / 256);
  const bool long5 = p.D == 128 && (p.S >= 2048 || (p.S >= 1024 && blocks * 4 >= 3L * n_cu));
  int mode = p.bias != nullptr ? 4 : g_dk_attn_mode < 0 ? (long5 ? 10 : 4) : g_dk_attn_mode;
  if (p.dtype != DK_DTYPE_BF16) {  // fp16 (SD3 family): the lean kernel, whatever dk_tune_set("attn", 9 / 10) names -- those kernels are bf16 only
    DK_REQUIRE(p.dtype == DK_DTYPE_F16 && p.D == 64 && p.bias == nullptr && p.O8 == nullptr, "fp16 attention: head_dim 64, no score bias, no MX-fp8 copy");
    mode = 4;
  }
  if (p.ident_from != 0) mode = 4;  // identity attention: the lean kernel's template case, whatever the "attn" knob says
  if (mode == 10 && !dk_attention5_eligible(p)) mode = 9;
  if (p.O8 != nullptr && p.o8_split != 0) {
    DK_REQUIRE(p.o8_split > 0 && p.o8_split < p.S && p.o8_txt_row0 >= p.B * (p.S - p.o8_split), "MX-fp8 copy: text rows behind the image rows");
    if (mode == 10) mode = 9;  // (attention5.hip writes the joint row order only)
  }
  if (mode == 9 && p.D != 128) mode = 4;  // (the phase-alternating kernel is D = 128 only)
  DK_REQUIRE(mode == 4 || mode == 9 || mode == 10, "unknown attention variant (4: lean kernel, 9: phase-alternating kernel, 10: one-wave-per-SIMD kernel)");
  DK_REQUIRE((size_t)p.S * p.ld * 2 < (1ull << 32), "one batch row of QKV must span < 4 GiB");
  if (p.bias != nullptr)  // text encoders: D = 64, short sequences
    DK_REQUIRE(p.ldb % 64 == 0 && p.ldb >= p.S && ((uintptr_t)p.bias & 7) == 0 && p.bias_head_stride % 4 == 0,
               "attention bias: row stride must be a multiple of 64 >= S, 8-byte aligned");
  r = AttnRoute{};
  r.kernel = mode;
  r.n_cu = n_cu;
  r.qfuse = p.bias == nullptr && (p.qn_a != nullptr || p.q_rope != nullptr);  // (the score-bias form has no fused query load)
  if (r.qfuse) DK_REQUIRE(p.qn_a == nullptr || p.qn_b != nullptr, "qn_b missing (pass qn_a twice for one weight)");
  r.blocks = r.whole = (int)blocks;
  r.split = 1;
  // Kernel 10, one workgroup per CU: a launch of nb blocks runs in ceil(nb / n_cu) rounds, the last one with nb % n_cu blocks.  Those blocks are split
  // into s key ranges each (every range a multiple of four tiles, at least twelve) when that shortens the last round: it then takes
  // ceil(tail * s / n_cu) / s of a block's time.  The partial results go through the caller's region and dk_attn5_merge_kernel.
  const int tail = r.blocks % n_cu;
  if (mode == 10 && tail > 0 && p.O8 == nullptr && g_dk_attn5_split != 0) {
    // (measured, profiles/r05_attention5_lab.log: a workgroup costs ~14 us + 1.66 us per tile, and a last round on 152 of 256 CUs runs faster
    //  than a full one -- FLUX, one image, gains nothing from three ranges in two sub-rounds; a tail that fits the CUs in ONE sub-round does:
    //  batch 4: 96 blocks x 2)
    for (int s = 2; s <= 4 && r.split == 1; ++s) {
      if ((p.S / 256) / s < 3) break;  // >= 12 tiles per range
      if (g_dk_attn5_split > 0 ? s == g_dk_attn5_split : (tail * s <= n_cu && tail * s * 10 >= n_cu * 6)) r.split = s;
    }
    if (ws_bytes < (size_t)tail * r.split * DK_ATTN5_JOB_BYTES) r.split = 1;
    if (r.split > 1) r.whole = r.blocks - tail, r.jobs = tail * r.split;
  }
  // Kernel 10's body without the running row maximum (the derivation stands at DK_ATTN5_UNTRACKED_MAX_ARG): only for a launch this kernel takes anyway,
  // with the fused query load (the one instantiation built: every model launch of the bf16 FLUX path), under a bound the caller gave.  No bound, a larger
  // one (or a NaN), the knob at 1, the plain Q load: the tracked body, as before.
  DK_REQUIRE(!(p.score_bound < 0.f), "score_bound: a bound on |scale * q.k| is positive (0: unknown)");
  r.untracked = mode == 10 && r.qfuse && g_dk_attn5_track != 1 && p.score_bound > 0.f && 2.0f * p.score_bound * DK_LOG2E <= DK_ATTN5_UNTRACKED_MAX_ARG;
  // only the D = 128 kernels 9 and 10 write the MX-fp8 copy themselves: the bf16 output of the lean kernel is quantised behind it
  r.quantize = p.O8 == nullptr || mode != 4 ? 0 : p.o8_split != 0 ? 2 : 1;
  r.launches = 1 + (r.jobs > 0) + (r.quantize != 0);
  return 0;
}

// ws: the caller's region for the partial results of attention5.hip's key-split workgroups (AttnWs, dk_kernels.h)
int dk_launch_attention(const AttnParams& p_in, AttnWs ws, hipStream_t stream) {
  AttnRoute r;
  if (const int rc = dk_attention_route(p_in, ws.p != nullptr ? ws.bytes : 0, dk_device_cu_count(), r)) return rc;
  AttnParams p = p_in;
  if (p.bal_ws == nullptr) p.bal_ws = ws.p;
  double work = 4.0 * (double)p.B * p.H * (double)p.S * (double)p.S * p.D;
  if (p.ident_from != 0) {  // the tiles the query blocks walk (dk_ident_walk): 128 queries x 64 keys each
    long tiles = 0;
    for (int q0 = 0; q0 < p.S; q0 += 128) {
      const IdentWalk w = dk_ident_walk(q0, p.S, p.ident_from);
      tiles += w.n_lo + w.n_hi;
    }
    work = 4.0 * (double)p.B * p.H * (double)tiles * 128.0 * 64.0 * p.D;
  }
  dk_prof_begin(2, work, stream);
  const int rc = r.kernel == 10 ? dk_launch_attention5(p, r, ws.p, stream) : r.kernel == 9 ? dk_launch_attention4(p, stream) : dk_launch_attention2(p, 4, stream);
  dk_prof_end(stream);
  if (rc) return rc;
  DK_CHECK_HIP(hipGetLastError());
  if (r.quantize == 2) {  // text rows of every batch row -> [o8_txt_row0, ...), image rows -> [0, B * S_i)
    const int S_t = p.o8_split, S_i = p.S - S_t;
    Mx8Out o_txt{p.O8, p.O8_scales, p.o8_ld, p.o8_nblk, p.o8_txt_row0, p.B * S_t, 0, 0}, o_img{p.O8, p.O8_scales, p.o8_ld, p.o8_nblk, 0, p.B * S_i, 0, 0};
    return dk_launch_quantize2_mx8(p.O + (size_t)S_t * p.ldo, S_i, p.B * S_i, o_img, p.O, S_t, p.B * S_t, o_txt, p.ldo, p.S, p.H * p.D, stream);
  }
  if (r.quantize == 1) {
    Mx8Out o8{p.O8, p.O8_scales, p.o8_ld, p.o8_nblk, 0, p.B * p.S, 0, 0};
    return dk_launch_quantize_mx8(p.O, p.ldo, p.B * p.S, 0, p.B * p.S, p.H * p.D, o8, stream);
  }
  return 0;
}
