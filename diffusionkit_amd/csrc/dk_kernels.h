// Internal launcher declarations shared by the kernel translation units and the C-ABI layer.
#pragma once
#include "../../include/dk_hip.h"
#include "dk_common.h"
#include "dk_ksplit.h"

// ---- GEMM / implicit-GEMM conv ---------------------------------------------------------
// C[m, n] = epi(alpha * sum_k A[m, k] * W[n, k] + bias[n])   (bf16 in, fp32 accumulate, bf16 out)
// Logical row m maps to physical row (m / seg_len) * seg_stride + (m % seg_len); this is how a
// stream (text rows / image rows of a joint [B, S, h] buffer) is addressed without copies.
// epilogue codes: DK_EPI_* in include/dk_hip.h

struct GemmParams {
  const bf16_t* A;
  const bf16_t* W;
  bf16_t* C;
  const bf16_t* bias;  // [N] or null
  const bf16_t* gate;  // [n_batch, gate_stride] or null
  const bf16_t* res;   // same row mapping as C, leading dim ldr
  int M, N, K;
  int lda, ldc, ldr;
  int ldw;  // row stride of W in elements (>= K; a padded stride avoids L2-channel camping on power-of-two K)
  int a_seg_len, a_seg_stride;
  int c_seg_len, c_seg_stride;
  int r_seg_len, r_seg_stride;
  int gate_seg_len, gate_stride;
  float alpha;
  int epi;
  // implicit-GEMM 3x3 conv (pad 1, stride 1) over NHWC input; M = cB*cH*cW output pixels,
  // K = 9*cC. If ups != 0 the conv input is the nearest-neighbour x2 upsampling of the stored
  // [cB, cH/2, cW/2, cC] tensor (vae.py:20-25 folded into the gather); ups == 2: stride-2 conv over the stored
  // [cB, 2*cH, 2*cW, cC] tensor padded by one zero row / column at the bottom / right (vae.py:141-143).
  int conv;
  int cB, cH, cW, cC, ups;
  const bf16_t* zeros;  // >= 128 B of zeros (padding taps)
  void* workspace;      // optional K-split workspace (dk_gemm_split_workspace_bytes()), else null
  size_t workspace_bytes;
  // optional column split (256^2 kernel only): output columns >= n_split go to C2 (leading dim ldc2, same row
  // map as C, column index rebased to 0) with epilogue epi2 -- the fused linear1 of the single-stream blocks
  // (q/k/v projection | fc1 + GELU over one read of the modulated activations, mmdit.py:693-751)
  int n_split;
  bf16_t* C2;
  int ldc2;
  int epi2;
  // optional QKNorm + RoPE of the KEY columns (mmdit.py:754-764, 934-942) inside the tail of a q / k / v projection on the 256^2
  // kernel (bias-only epilogue): columns [kn_col0, kn_col1) -- multiples of 256 -- are heads of kn_D (128 or 64) columns; a row's
  // head is normalised with weight kn_w [kn_D] and rotated by the cos / sin table kn_rope [S_pos, kn_D / 2, 2] (null: no rotation)
  // at position kn_pos_off + (row % kn_seg_len).  Same arithmetic and rounding points as dk_qk_norm_rope_kernel.  Null kn_w: off.
  // (a launch that does not reach the 256^2 kernel runs dk_launch_qk_norm_rope on its output instead: gemm.hip)
  const bf16_t* kn_w;
  const float* kn_rope;
  int kn_col0, kn_col1, kn_D, kn_pos_off, kn_seg_len;
  float kn_eps;
  // round 4: the QUERY columns [qn_col0, qn_col1) the same way with their own weight qn_w (same head size, table, positions, eps) -- the
  // attention kernel then loads finished queries.  Needs kn_w; null qn_w: queries untouched
  const bf16_t* qn_w;
  int qn_col0, qn_col1;
  // element type of A, W, C, bias, gate, res and the norm weights: DK_DTYPE_BF16 (0) or DK_DTYPE_F16 (1: Linears and the conv form on the 128^2
  // kernel and gemm256v3.hip only -- the route never names gemm256v4.hip)
  int dtype;
};
int dk_launch_gemm(const GemmParams& p, hipStream_t stream);
// two problems with the same N, K, epilogue in one launch (image + text stream of a double block); falls
// back to two launches when the pair is not eligible for the grouped kernel
int dk_launch_gemm_pair(const GemmParams& p0, const GemmParams& p1, hipStream_t stream);
// dk_tune_set knobs of the routing (gemm.hip)
extern int g_dk_gemm_mode;
extern int g_dk_v3_split;       // remainder-wave K split (-1 auto, 0 off, 1 whenever possible)
extern int g_dk_pair_split_nk;  // see route_pair
extern int g_dk_v3_split_min;   // ... saved K-tile steps below which an all-remainder Linear stays whole (-1: default)
extern int g_dk_v3_mf;          // wave-tile height in 16-row fragments (-1 auto, 8 = 256-row tiles, 7 = 224-row tiles)
extern int g_dk_v4_auto;
extern int g_dk_v4_skew;  // gemm256v4.hip

// How the tiles beyond the last full wave of the CUs are cut along K (gemm256v3.hip's SplitArgs): n_dp whole tiles, then n_rem tiles in S
// pieces each, the finisher's ks K-tiles first.  n_rem == 0: no split (S = 1, ks = all K-tiles).
struct SplitPlan {
  int n_dp, n_rem, S, ks;
};
// the split of `tiles` tiles of nk K-tiles each on n_cu CUs (gemm.hip; the fp8 kernel's split takes it too)
SplitPlan dk_plan_split(int tiles, int nk, bool have_ws, int n_cu, bool linear);
// the caller's K-split workspace is usable (never with the fused key QKNorm: a cut tile's finisher has no second pass over its row sums)
template <class P>
bool dk_ksplit_ws_ok(const P& p, const P* p2) {
  return p.workspace != nullptr && p.workspace_bytes >= DK_KSPLIT_WS_BYTES && ((uintptr_t)p.workspace & 255) == 0 && p.kn_w == nullptr &&
         (p2 == nullptr || p2->kn_w == nullptr);
}

// What one dk_launch_gemm / dk_launch_gemm_pair call launches: dk_gemm_route (gemm.hip) decides it from the problem(s), the CU count and the
// tuning knobs alone; the launchers below take it as it is, and dk_gemm_plan reports it.
struct GemmRoute {
  // the call expands into two calls: the two problems of a pair one after the other, the two column ranges of a column split on the
  // 128^2 kernel, or the projection without the fused key QKNorm followed by the stand-alone norm pass
  enum { PAIR = -1, COLUMNS = -2, KNORM = -3 };
  int kernel;     // 128: dk_gemm_bf16_kernel (128 x 128 tiles), 3: dk_gemm256v3_kernel (8 waves), 4: dk_gemm256v4_kernel (one wave per SIMD); or < 0
  int tile_rows;  // 128 / 224 / 256
  int tiles_a, tiles_b;  // output tiles of each problem (tiles_b: 0 without a second one)
  int n_cu;       // compute units the rules assumed
  SplitPlan split;  // kernel 3 only; otherwise {tiles, 0, 1, K / 64}
};
int dk_gemm_route(const GemmParams& p, const GemmParams* p2, int n_cu, GemmRoute& r);
int dk_gemm_plan_call(const GemmParams& p, const GemmParams* p2, dk_gemm_plan_t& rec);  // dk_gemm_plan: records the routes, launches nothing

// workspace of the remainder-wave K split (dk_ksplit.h: fp32 slabs + the flag region, which must be zero before the first launch; the kernels
// leave it zero)
size_t dk_gemm_split_workspace_bytes();
bool dk_gemm256v3_eligible(const GemmParams& p);  // N % 128 == 0, K % 64 == 0, any M, any row-segment maps
// gemm256v4.hip: one wave per SIMD, 256 accumulators in AGPRs, hand-scheduled asm body (N % 256 == 0, no conv / K split / half tiles)
bool dk_gemm256v4_eligible(const GemmParams& p);
int dk_launch_gemm256v4(const GemmParams& p, const GemmParams* p2, const GemmRoute& r, hipStream_t stream);

// fused key (and query) QKNorm + RoPE in the tail of a 256-column kernel (GemmParams / GemmF8Params kn_*, qn_*): whole 256-column tiles of 128- or
// 64-column heads, bias-only first output
template <class P>
bool dk_qknorm_eligible(const P& p) {
  if (p.kn_w == nullptr) return p.qn_w == nullptr;  // the query side rides on the key side's machinery
  if (p.epi != DK_EPI_BIAS || (p.kn_D != 128 && p.kn_D != 64) || p.kn_seg_len <= 0 || p.kn_col0 % 256 != 0 || p.kn_col1 % 256 != 0 || p.kn_col0 >= p.kn_col1 ||
      p.kn_col1 > (p.n_split > 0 ? p.n_split : p.N) || ((uintptr_t)p.kn_w & 15) != 0 || ((uintptr_t)p.kn_rope & 15) != 0)
    return false;
  return p.qn_w == nullptr || !(p.qn_col0 % 256 != 0 || p.qn_col1 % 256 != 0 || p.qn_col0 >= p.qn_col1 || p.qn_col1 > (p.n_split > 0 ? p.n_split : p.N) ||
                                (p.qn_col0 < p.kn_col1 && p.kn_col0 < p.qn_col1) || ((uintptr_t)p.qn_w & 15) != 0);
}

// the operands the shared tail of the 256-column kernels reads beside the accumulators (dk_gemm_tail.h; GemmParams / GemmF8Params): a column
// split on a tile boundary with its second output, residual and gate where an epilogue of either output reads them, rows of whole 16-byte
// pieces, 16-byte aligned.  (The outputs' own alignment depends on their kind: the callers check it.)
template <class P>
bool dk_gemm_tail_operands_ok(const P& p) {
  if (p.n_split % 256 != 0 || (p.n_split > 0 && (p.C2 == nullptr || p.n_split >= p.N))) return false;
  const bool res1 = p.epi == DK_EPI_GATE_RES || p.epi == DK_EPI_RES;
  const bool res2 = p.n_split > 0 && (p.epi2 == DK_EPI_GATE_RES || p.epi2 == DK_EPI_RES);
  if ((res1 || res2) && (p.res == nullptr || p.r_seg_len <= 0 || p.ldr % 8 != 0)) return false;
  if ((p.epi == DK_EPI_GATE_RES || (p.n_split > 0 && p.epi2 == DK_EPI_GATE_RES)) && (p.gate == nullptr || p.gate_seg_len <= 0)) return false;
  auto al16 = [](const void* q) { return ((uintptr_t)q & 15) == 0; };
  return al16(p.res) && al16(p.bias) && al16(p.gate) && (p.gate == nullptr || p.gate_stride % 8 == 0);
}

// ---- fp8 GEMM (gemm256f8.hip): e4m3 weights with per-output-channel fp32 scales, MX-fp8 activations -------------------
// C[m, n] = epi(wscale[n] * sum_k A[m, k] * 2^(SA[m, k / 32] - 127) * W[n, k] + bias[n]); same row-segment maps, epilogues,
// grouped launch and column split as GemmParams.  Strides of A / W and of an MX-fp8 output are in BYTES (= elements).
struct GemmF8Params {
  const unsigned char* A;   // [rows, K] e4m3, row pitch lda
  const unsigned char* SA;  // E8M0 scales of the A BUFFER (dk_mx_scale_index over its physical rows), sa_nblk 128-row blocks per K-tile
  const unsigned char* W;   // [N, K] e4m3, row pitch ldw
  const float* wscale;      // [N]
  void* C;                  // bf16 [., ldc] or, with c_mx8, e4m3 [., ldc] + scales into SC
  const bf16_t* bias;
  const bf16_t* gate;
  const bf16_t* res;
  int M, N, K;
  int lda, ldw, ldc, ldr;
  int a_seg_len, a_seg_stride, a_row0;  // a_row0: physical row of the A buffer that pointer A addresses (scale indexing)
  int sa_nblk;
  int c_seg_len, c_seg_stride;
  int r_seg_len, r_seg_stride;
  int gate_seg_len, gate_stride;
  int epi;
  int c_mx8;
  // optional column split: output columns >= n_split go to C2 (column index rebased to 0) with epilogue epi2
  int n_split;
  void* C2;
  int ldc2, epi2, c2_mx8;
  // MX-fp8 outputs: scale side array of the OUTPUT buffer, its 128-row block count, the physical row that pointer C / C2
  // addresses, and the 32-column block index of output column 0 inside that buffer's rows
  unsigned char* SC;
  int sc_nblk, c_row0, sc_kb0;
  // optional QKNorm + RoPE of the key columns in the tail (see GemmParams; bf16 first output, bias-only epilogue)
  const bf16_t* kn_w;
  const float* kn_rope;
  int kn_col0, kn_col1, kn_D, kn_pos_off, kn_seg_len;
  float kn_eps;
  const bf16_t* qn_w;  // ... and of the query columns [qn_col0, qn_col1) (see GemmParams)
  int qn_col0, qn_col1;
  // optional K-split scratch (dk_gemm_split_workspace_bytes(), the bf16 kernels' buffer: dk_ksplit.h, flag region zero between launches):
  // round 6 -- a launch of at most half a round of tiles with a long reduction is cut along K (FLUX below 1024 x 1024)
  void* workspace;
  size_t workspace_bytes;
};
bool dk_gemm256f8_eligible(const GemmF8Params& p);
int dk_launch_gemm256f8(const GemmF8Params& p, const GemmF8Params* p2, hipStream_t stream);
// bf16 rows -> MX-fp8 rows + scales (fp8_ops.hip).  x: [M, h] bf16 through the row map (seg_len, seg_stride); out row m at
// physical row out_row0 + (m / o_seg_len) * o_seg_stride + m % o_seg_len of the fp8 buffer (pitch ldo bytes, column
// offset col0, a multiple of 32).  dk_launch_ln_modulate_mx8 = dk_launch_ln_modulate with that output.
struct Mx8Out {
  unsigned char* out;  // buffer base (physical row 0, column 0)
  unsigned char* scales;
  int ldo, n_blk128, row0, seg_len, seg_stride, col0;
};
int dk_launch_quantize_mx8(const bf16_t* x, int ldx, int x_seg_len, int x_seg_stride, int M, int h, const Mx8Out& o, hipStream_t stream);
// two such jobs in one launch (the text and the image rows of a joint attention output): rows through (x_seg_len*, x_seg_stride) of x0 / x1
int dk_launch_quantize2_mx8(const bf16_t* x0, int x_seg_len0, int M0, const Mx8Out& o0, const bf16_t* x1, int x_seg_len1, int M1, const Mx8Out& o1,
                            int ldx, int x_seg_stride, int h, hipStream_t stream);
int dk_launch_ln_modulate_mx8(const bf16_t* x, int ldx, int M, int h, const bf16_t* shift, const bf16_t* scale, int mod_stride, int seg_len,
                              int x_seg_len, int x_seg_stride, float eps, const Mx8Out& o, hipStream_t stream);
int dk_launch_ln_modulate2_mx8(const bf16_t* x0, int M0, const bf16_t* shift0, const bf16_t* scale0, int seg0, const Mx8Out& o0,
                               const bf16_t* x1, int M1, const bf16_t* shift1, const bf16_t* scale1, int seg1, const Mx8Out& o1, int ldx, int h,
                               int mod_stride, int x_seg_stride, float eps, hipStream_t stream);
// dk_launch_ln_modulate over a joint stream with a residual in front of SOME rows (FLUX ControlNet taps; bf16 only, elementwise.hip): of every
// tap_seg logical rows the first tap_first are plain, row s >= tap_first of group b becomes round(fmaf(s, tap[b * (tap_seg - tap_first) + s -
// tap_first], x)) in place first; tap: dense [(M / tap_seg) * (tap_seg - tap_first), ldt]
int dk_launch_ln_modulate_add_joint(bf16_t* x, int ldx, const bf16_t* tap, int ldt, float s, int tap_seg, int tap_first, bf16_t* out, int ldo, int M,
                                    int h, const bf16_t* shift, const bf16_t* scale, int mod_stride, int seg_len, int x_seg_len, int x_seg_stride,
                                    float eps, hipStream_t stream);

// decoupled image-prompt attention (FLUX IP-Adapter; bf16, D = 128, 1 <= N <= 16; ip_attention.hip): out [B * seg_len, h] dense = softmax over the N
// keys K[b] of scale * q_n . k, times V[b]; q_n = the QK-normed, NOT rotated q columns (the first h of ldq) of rows first_row .. + seg_len - 1 of every
// batch row of qkv [B, seg_stride, ldq]; K, V: [B, N, h] at ldkv elements per row
int dk_launch_ip_attention(const bf16_t* qkv, int ldq, int seg_len, int seg_stride, int first_row, const bf16_t* qn, const bf16_t* K, const bf16_t* V,
                           int ldkv, int B, int N, int h, int D, float scale, float eps, bf16_t* out, hipStream_t stream);

// optional HIP-event timing of the dominant kernels (profile.hip); cls: 0 GEMM, 1 conv, 2 attention, 3 fp8 GEMM
void dk_prof_begin(int cls, double work, hipStream_t st);
void dk_prof_end(hipStream_t st);

// ---- attention -------------------------------------------------------------------------
struct AttnParams {
  const bf16_t* Q;  // row s of batch b: Q + (b*S + s)*ld + head*D
  const bf16_t* K;
  const bf16_t* V;
  bf16_t* O;  // O + (b*S + s)*ldo + head*D
  int B, H, S, D;
  int ld, ldo;
  float scale;
  // the caller's bound on |scale * q.k| over the whole launch, in natural units, AFTER the query transform of the Q load; 0: unknown.  A promise,
  // not checked: attention5.hip runs its tile loop without the running row maximum when the bound admits it (dk_attention_route), and a launch that
  // breaks the promise can overflow.  The engine derives it from the QKNorm weights (mmdit_engine.hip: dk_score_bound.h).  Only the route reads it.
  // (It sits in the four bytes of padding between `scale` and the pointer below: the struct is a kernel argument, and a field behind the last one
  //  would move the hidden arguments of every attention kernel -- this way their code objects stay what they were, static_assert below.)
  float score_bound = 0.f;
  // optional additive score bias (text encoders: CLIP's causal mask clip.py:83-89, T5's relative-position bias
  // t5.py:61-88): scores = scale * q.k + bias[head * bias_head_stride + q * ldb + k]; ldb a multiple of 64 >= S
  const bf16_t* bias = nullptr;
  long bias_head_stride = 0;
  int ldb = 0;
  // optional QKNorm (mmdit.py:754-764) + RoPE (:934-942) of the QUERY rows inside the kernel's Q load (the keys keep their
  // own pass, dk_launch_qk_norm_rope*(..., k_only)): rows s < qn_split use weight qn_a, the others qn_b; q_rope = the
  // [S, D/2, 2] cos/sin table indexed by s, or null
  const bf16_t* qn_a = nullptr;
  const bf16_t* qn_b = nullptr;
  int qn_split = 0;
  float qn_eps = 1e-6f;
  const float* q_rope = nullptr;
  // the caller's workspace region, filled in by dk_launch_attention when null; no shipped kernel reads it: attention4.hip's DK4_TRACE lab
  // builds stamp their trace into it (scripts/attn_trace.py)
  void* bal_ws = nullptr;
  // optional MX-fp8 copy of the output (fp8_linears: the o-projection's activation operand): row (b*S + s) of O8 at o8_ld bytes
  // per row, head h at byte column h*D; E8M0 scales of 32-column blocks in O8_scales (dk_mx_scale_index over o8_nblk 128-row
  // blocks).  dk_attn4_fwd_kernel writes it INSTEAD of O from its accumulators (values rounded to bf16 first, as the separate
  // quantiser pass over O sees them); for the other kernels dk_launch_attention runs that pass behind the launch.
  unsigned char* O8 = nullptr;
  unsigned char* O8_scales = nullptr;
  int o8_ld = 0, o8_nblk = 0;
  // row order of that copy.  o8_split == 0: row b*S + s, like O.  o8_split = S_t > 0 (the engine's double blocks with a ragged image token
  // count): the image rows of all batch rows first, row b*(S - S_t) + (s - S_t), and the text rows behind them, row o8_txt_row0 + b*S_t + s --
  // the two row ranges of the o-projections then start on 128-row scale blocks whatever S is (attention5.hip does not take such launches)
  int o8_split = 0, o8_txt_row0 = 0;
  // attention5.hip, filled in by its launcher: workgroups 0 .. a5_whole - 1 take whole query blocks; the others one of a5_split key ranges of
  // a block of the last, partial round of the CUs and leave (O / l in bf16, offset, l) in a5_ws for dk_attn5_merge_kernel
  int a5_whole = 0, a5_split = 1;
  void* a5_ws = nullptr;
  // element type of Q, K, V, O and the query-norm weights: DK_DTYPE_BF16 (0) or DK_DTYPE_F16 (1: D = 64, the lean kernel)
  int dtype = 0;
  // identity attention (perturbed-attention guidance; the lean kernel, D = 64): 0 off.  F = ident_from, 1 <= F < S: a query s < F (text) sees
  // every key; a query s >= F (image) sees the keys [0, F) and its own key s, nothing else
  int ident_from = 0;
};
static_assert(sizeof(AttnParams) == 184 && offsetof(AttnParams, score_bound) == 60, "AttnParams is a kernel argument: its size and offsets are part of every attention kernel's code");
// The 64-key tiles a 128-query block of identity attention walks, in order: tiles [0, n_lo), then [hi0, hi0 + n_hi).  A block that lies wholly
// in the image range (q0 >= F) takes the ceil(F / 64) tiles that hold text keys and the tiles that hold its own rows, cut at the end of the
// sequence -- never the same tile twice: q0 >= F is a multiple of 64, so q0 / 64 >= ceil(F / 64).  A block with a text query walks every tile.
// Shared by the kernel (attention2.hip) and the FLOP count of the launch (attention.hip).
struct IdentWalk {
  int n_lo, hi0, n_hi;
};
__host__ __device__ inline IdentWalk dk_ident_walk(int q0, int S, int F) {
  const int ntiles = (S + 63) / 64;
  if (q0 < F) return IdentWalk{ntiles, ntiles, 0};
  const int hi0 = q0 / 64;
  return IdentWalk{(F + 63) / 64, hi0, ntiles - hi0 < 2 ? ntiles - hi0 : 2};
}
// the region the key-split workgroups of attention5.hip leave their partial results in (dk_attention_workspace_bytes(); 256-byte aligned): the
// caller's own -- an engine's carve, or what dk_attention_set_workspace gave the stand-alone entries.  Empty, or too small for a launch: no split
struct AttnWs {
  void* p = nullptr;
  size_t bytes = 0;
};
// bytes one key-split job leaves in that region: 256 rows x 128 bf16 of O / l, then 256 x (exponent offset, l) in fp32 (attention5.hip's indexing
// keeps the two sizes as literals)
constexpr size_t DK_ATTN5_JOB_BYTES = 65536 + 2048;

// What one dk_launch_attention call launches: dk_attention_route (attention.hip) decides it -- and makes every argument check -- from the problem,
// the bytes of the caller's region, the CU count and the knobs "attn" / "attn_split" / "attn_track" alone; the launchers take it as it is, and
// dk_attention_plan reports it.  A key split changes the summation order: the route is part of the results.
struct AttnRoute {
  int kernel;     // in the knob's codes: 4 lean (attention2.hip), 9 phase-alternating (attention4.hip), 10 one wave per SIMD (attention5.hip)
  bool qfuse;     // QKNorm / RoPE of the queries inside the Q load
  int blocks;     // query blocks of 256 rows, B * H * ceil(S / 256): what the automatic choice counts and kernels 9 and 10 launch per workgroup
  // kernel 10 (otherwise whole = blocks, split = 1, jobs = 0): workgroups 0 .. whole - 1 take whole blocks; each of the blocks - whole others,
  // the launch's last, partial round of the CUs, is cut into `split` key ranges -- jobs = (blocks - whole) * split workgroups more, and a
  // dk_attn5_merge_kernel launch behind them when jobs > 0
  int whole, split, jobs;
  int quantize;   // MX-fp8 copy: 0 none, or the kernel writes it; 1 a quantiser pass follows; 2 the same as two row ranges (o8_split)
  int launches;   // kernel launches of the call
  int n_cu;       // compute units the rules assumed
  bool untracked;  // kernel 10: the tile loop without the running row maximum (AttnParams::score_bound admits it; knob "attn_track")
};
extern int g_dk_attn_mode, g_dk_attn5_split, g_dk_attn5_track;  // attention.hip
int dk_attention_route(const AttnParams& p, size_t ws_bytes, int n_cu, AttnRoute& r);
int dk_launch_attention(const AttnParams& p, AttnWs ws, hipStream_t stream);
// the kernels' launchers: arguments checked, kernel and split chosen by dk_attention_route
int dk_launch_attention4(const AttnParams& p, hipStream_t stream);             // attention4.hip (the waves of a SIMD in opposite phases; D = 128, no score bias)
bool dk_attention5_eligible(const AttnParams& p);                              // attention5.hip (one wave per SIMD, asm tile loop; D = 128, S % 256 == 0, no score bias)
int dk_launch_attention5(const AttnParams& p, const AttnRoute& r, void* ws, hipStream_t stream);

// ---- single-head D = 512 attention of the VAE's mid block (attention512.hip) -------------------------------
struct Attn512Params {
  const bf16_t* Q;   // [B, T, ld]
  const bf16_t* K;   // [B, T, ld]
  const bf16_t* Vt;  // TRANSPOSED values: [B, 512, Tp], rows zero-padded beyond T (dk_launch_transpose with ldy = Tp)
  bf16_t* O;         // [B, T, ldo]
  int T, Tp, B, ld, ldo;
  float scale;
  int dtype;  // element type of Q, K, Vt and O: DK_DTYPE_BF16 (0) or DK_DTYPE_F16 (1)
};

// ---- text-conditioning kernels (text_ops.hip) ---------------------------------------------------
int dk_launch_embedding(const bf16_t* table, const int* ids, const bf16_t* pos, int pos_rows, bf16_t* out, float* out_f32, int n, int dim,
                        int vocab, hipStream_t stream);
int dk_launch_layernorm(const bf16_t* x, bf16_t* out, int M, int h, const bf16_t* w, const bf16_t* b, float eps, hipStream_t stream);
int dk_launch_t5_rmsnorm(const float* x, bf16_t* out, int M, int h, const bf16_t* w, float eps, hipStream_t stream);
int dk_launch_text_elementwise(const bf16_t* a, const bf16_t* b, bf16_t* y, float* r, long n, int op, hipStream_t stream);
int dk_launch_t5_bias(const bf16_t* emb, const int* rel_bucket, int H, int S, int ld, bf16_t* out, hipStream_t stream);

// ---- elementwise / normalisation ---------------------------------------------------------
int dk_launch_rope_table(float* table, int S_txt, int gh, int gw, const int* axes, int n_axes, float theta,
                         hipStream_t stream);
// seg: [n_seg][3] = (gh, gw, index) on the host; the one-grid form above is this with the segment (gh, gw, 0)
int dk_launch_rope_table_segments(float* table, int S_txt, int n_seg, const int* seg, const int* axes, int n_axes, float theta,
                                  hipStream_t stream);
int dk_launch_f32_to_bf16(const float* x, bf16_t* y, long n, hipStream_t stream);
int dk_launch_affine_f32(const float* x, float* y, long n, float a, float b, hipStream_t stream);
// inpainting: mask u8 [n_mask, H, W] -> f32 [n_mask, H / f, W / f] (box sum / (f * f * 255)); paste-back of the kept pixels
int dk_launch_mask_to_latent(const unsigned char* mask, float* out, int n_mask, int H, int W, int f, hipStream_t stream);
int dk_launch_image_composite_u8(const unsigned char* dec, const unsigned char* orig, const unsigned char* mask, unsigned char* out, int B,
                                 int H, int W, int orig_per_image, int mask_per_image, hipStream_t stream);
// channel-concatenated conditioning (FLUX.1 Fill / Canny / Depth): the masked-out image in [-1, 1], and the bf16 condition token rows
// [n, S_i, p*p*C (+ 64*p*p with a mask)] from its latent and the mask (null: the latent columns only)
int dk_launch_image_mask_out_f32(const unsigned char* image, const unsigned char* mask, float* out, int n, int H, int W, int mask_per_image,
                                 hipStream_t stream);
int dk_launch_fill_condition_tokens(const float* z, const unsigned char* mask, bf16_t* tok, int n, int mask_per_image, int Hl, int Wl, int C,
                                    int p, hipStream_t stream);
// stochastic samplers: out f32 [n_img, n_per_img], row j the standard normals of seeds[j] (Philox4x32-10 + Box-Muller, include/dk_hip.h)
int dk_launch_philox_normal(float* out, const unsigned long long* seeds, int n_img, long n_per_img, unsigned draw, unsigned stream,
                            unsigned long long quad_offset, hipStream_t st);

// ---- launchers per element type ------------------------------------------------------------------------------
#include "dk_elem_launchers.h"
namespace dk_f16 {
#include "dk_elem_launchers.h"
}

// ---- 3x3 conv with LDS halo staging and the GroupNorm-apply + SiLU prologue (conv_halo.hip) ----------------------------------
struct ConvHaloParams {
  const bf16_t* x;        // stored input NHWC [B, H >> ups, W >> ups, C] (RAW values when gn_ss is given)
  const bf16_t* w;        // [O, ldw] K-major: column tap * C + c (tap = ky * 3 + kx), then (x2) 9 * C + c2
  const bf16_t* bias;     // [O]
  const bf16_t* bias2;    // bias of the shortcut extension, or null
  const bf16_t* res;      // residual NHWC [B, H, W, ldr], or null
  bf16_t* y;              // NHWC [B, H, W, ldy]
  const float* gn_ss;     // [B][2][C] fp32 (scale | shift) of the GroupNorm applied to x on load, or null (x is used as it is)
  int gn_silu;            // SiLU behind that GroupNorm
  const bf16_t* x2;       // 1x1 shortcut input NHWC [B, H, W, C2] (raw), or null
  int C2;
  float* stats_out;       // [B][tiles per image][G_out][2] (sum, M2 = sum of squared deviations from the tile's own mean) of the stored output, or null
  int G_out;
  float* img;             // image tail (O <= 4): clip(y / 2 + 0.5) f32 [npix, 3]
  unsigned char* u8;      // ... (x 255) truncated to uint8 [npix, 3]
  bf16_t* raw;            // ... y itself, bf16 [npix, 4]
  int out_channels;
  int B, H, W, C, O, ups, ldw, ldy, ldr;
  // element type of x, w, the biases, res, y, x2 and raw: DK_DTYPE_BF16 (0) or DK_DTYPE_F16 (1: conv_halo.hip only -- conv256v4.hip's asm body is
  // bf16, dk_conv256v4_wanted is false for fp16 whatever dk_tune_set("conv_v4", v) says).  Last field: the asm kernel's argument offsets stay.
  int dtype;
};
bool dk_conv_halo_eligible(const ConvHaloParams& p, bool img);
// GroupNorm statistics travel as (sum, M2) pairs, M2 = the sum of squared deviations from the pair's OWN mean, never as a raw sum of squares:
// E[x^2] - mean^2 in fp32 loses (mean / sigma)^2 ulps of the variance (1e-4 of it at mean / sigma = 32).  Producers sum deviations from a pivot
// (a value of the data itself) and convert; pairs of equal size are merged with the pairwise update below; dk_gn_finalize_kernel merges the chunks in fp64.
// n values summed about the pivot `pv` (s = sum (v - pv), q = sum (v - pv)^2) -> (sum, M2)
__device__ __forceinline__ void dk_gn_from_pivot(float& s, float& q, float pv, float n) {
  q -= s * s * (1.0f / n);
  q = q < 0.f ? 0.f : q;  // (not fmaxf: a NaN stays a NaN)
  s = fmaf(n, pv, s);
}
// (s, m2) of n values <- merged with (sb, mb) of as many: m2 += mb + (s - sb)^2 / 2n (commutative: both partners of a butterfly get the same bits)
__device__ __forceinline__ void dk_gn_merge_equal(float& s, float& m2, float sb, float mb, float inv_2n) {
  const float d = s - sb;
  m2 = (m2 + mb) + d * d * inv_2n;
  s += sb;
}
// conv256v4.hip: the same contract in the one-wave-per-SIMD frame (16 x 16 pixels x 256 channels per workgroup, asm body); no shortcut
// extension, no image tail.  dk_launch_conv_halo routes to it when dk_conv256v4_wanted (dk_tune_set("conv_v4", 0 | 1 | 2))
extern int g_dk_conv_v4;
bool dk_conv256v4_eligible(const ConvHaloParams& p);
bool dk_conv256v4_wanted(const ConvHaloParams& p);
int dk_launch_conv256v4(const ConvHaloParams& p, hipStream_t stream);

// ---- VAE launchers per element type (conv_halo.hip, attention512.hip, vae_ops.hip) -------------------------------------------
// dk_launch_conv_halo / dk_launch_attention512 at global scope forward to their dk_f16 twin on ConvHaloParams::dtype / Attn512Params::dtype;
// the vae_ops.hip launchers are picked by the caller.
#include "dk_vae_launchers.h"
namespace dk_f16 {
#include "dk_vae_launchers.h"
}
