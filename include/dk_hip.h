/*
 * dk_hip.h -- C ABI of libdk_hip.so: the MI355X (gfx950) denoising engine behind
 * DiffusionKit's DiffusionPipeline / FluxPipeline.
 *
 * The reference (argmaxinc/DiffusionKit, python/src/diffusionkit/mlx/) has no FFI layer: its
 * hot path is Python calling MLX ops.  This header *creates* the boundary a maintainer would
 * bind (ctypes stub in INTEGRATION.md).  Each entry point cites the reference call site it
 * replaces; paths are relative to python/src/diffusionkit/mlx/.
 *
 * Conventions
 *   - plain pointers and sizes only; device pointers are raw HIP device addresses
 *     (torch.Tensor.data_ptr()); `stream` is a hipStream_t passed as void*
 *     (torch.cuda.current_stream().cuda_stream); 0 = the null stream.
 *   - the caller owns every buffer, including the workspaces sized by *_workspace_bytes().
 *   - all activations / weights are bfloat16 (raw uint16 storage) unless a name says f32.
 *   - every function returns 0 on success, <0 on error; dk_last_error() describes the last
 *     failure of the calling thread.  Nothing throws across the ABI.
 *   - no hidden host synchronisation and no internal threads: work is enqueued on `stream`.
 *   - tensors are token-major / NHWC, exactly the layouts of the reference's MLX arrays.
 */
#ifndef DK_HIP_H
#define DK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DK_ABI_VERSION 5

int dk_abi_version(void);
const char* dk_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Operator level (one MLX op call site each).  These are what the parity tests drive.
 * ---------------------------------------------------------------------------------------- */

/* epilogues of dk_gemm_bf16 / dk_conv3x3_bf16 */
enum {
  DK_EPI_BIAS = 0,      /* C = A W^T + b                      nn.Linear, mmdit.py:56,821-832          */
  DK_EPI_BIAS_GELU = 1, /* C = gelu_erf(A W^T + b)            FFN fc1 + nn.GELU(), mmdit.py:421,835   */
  DK_EPI_GATE_RES = 2,  /* C = res + gate[b,:] * (A W^T + b)  post_sdpa gating, mmdit.py:533-548      */
  DK_EPI_RES = 3,       /* C = res + (A W^T + b)              VAE residual adds, vae.py:99,54         */
  DK_EPI_BIAS_SILU = 4  /* C = silu(A W^T + b)                embedder MLPs, mmdit.py:357-361,372-376 */
};

typedef struct dk_gemm_desc {
  const void* A;    /* [M, K] bf16, row stride lda (elements)                       */
  const void* W;    /* [N, K] bf16 contiguous (nn.Linear weight layout [out, in])   */
  void* C;          /* [M, N] bf16, row stride ldc                                  */
  const void* bias; /* [N] bf16 or NULL                                             */
  const void* gate; /* DK_EPI_GATE_RES: [n_batch, gate_stride] bf16                 */
  const void* res;  /* DK_EPI_GATE_RES / DK_EPI_RES: residual, row stride ldr       */
  int32_t M, N, K;
  int32_t lda, ldc, ldr;
  /* logical row m -> physical row (m / seg_len) * seg_stride + m % seg_len.  seg_len = M,
   * seg_stride = 0 addresses a plain matrix; (S_img, S) addresses the image rows of a joint
   * [B, S, h] buffer whose base pointer was advanced to the first image row. */
  int32_t a_seg_len, a_seg_stride;
  int32_t c_seg_len, c_seg_stride;
  int32_t r_seg_len, r_seg_stride;
  int32_t gate_seg_len; /* batch index of row m is m / gate_seg_len */
  int32_t gate_stride;
  float alpha;          /* scales the accumulator before the bias (1.0 for Linear) */
  int32_t epilogue;
  int32_t ldw;          /* row stride of W in elements; 0 = K (contiguous nn.Linear weight) */
  /* Optional scratch for the remainder-wave K split of the 256x256 kernel (large M, N % 256 == 0):
   * dk_gemm_workspace_bytes() bytes, 256-byte aligned, whose LAST 4096 bytes are zero before the first use (the
   * kernels leave them zero).  NULL = no K split.  One GEMM at a time may use a given workspace. */
  void* workspace;
  size_t workspace_bytes;
} dk_gemm_desc;

size_t dk_gemm_workspace_bytes(void);

/* nn.Linear call sites of the hot path: mmdit.py:56,358-360,373-375,432,771,777,821-832;
 * vae.py:36-39,84 */
int dk_gemm_bf16(const dk_gemm_desc* d, void* stream);

/* What dk_gemm_bf16(d) -- or, with d2 != NULL, the grouped launch the engines issue for the image and text streams of a double block -- WOULD
 * launch on the current device (ABI 5, round 6).  Host only: no kernel runs, pointers in the descriptors are not dereferenced (only their alignment
 * is looked at; `workspace` non-NULL tells the rules that the K split is available), and without a GPU the rules assume 256 compute units.  The
 * record is read from the same route the launch takes (dk_gemm_route, gemm.hip), so tests/test_dispatch_plan.py sweeps shapes over the dispatch
 * rules on the CPU.  A call that expands into several launches -- a pair that is not grouped runs as two -- reports their number in `launches`;
 * the other fields describe the last of them. */
typedef struct dk_gemm_plan_t {
  int32_t kernel;      /* 128: 128 x 128-tile kernel; 3: 256 x 256 tiles, 8 waves (gemm256v3.hip); 4: one wave per SIMD (gemm256v4.hip) */
  int32_t tile_rows;   /* 128 / 224 / 256 */
  int32_t tiles;       /* output tiles of the launch */
  int32_t workgroups;  /* grid size: a tile that is cut along K counts once per piece */
  int32_t split_tiles; /* tiles cut along K */
  int32_t k_pieces;    /* pieces per cut tile (1: none) */
  int32_t ks;          /* K steps of 64 elements a workgroup runs (the finisher piece of a cut tile) */
  int32_t n_cu;        /* compute units the rules assumed */
  int32_t launches;    /* kernel launches the call expands to */
} dk_gemm_plan_t;
int dk_gemm_plan(const dk_gemm_desc* d, const dk_gemm_desc* d2, dk_gemm_plan_t* plan);

/* The launch forms only the engines issue (dk_mmdit_forward: the q / k / v projections of the double blocks, linear1 of the single blocks), at the
 * operator level, so that each can be compared with a reference of that operation alone (tests/test_gpu_fused_ops.py).  A dk_gemm_side rides beside a
 * dk_gemm_desc and carries what the descriptor cannot say; all zero = the plain dk_gemm_bf16 call.
 *   column split: output columns >= n_split (multiple of 256) go to C2 (row stride ldc2, C's row map, column index rebased to 0) with epilogue epi2 --
 *     [q | k | v] and gelu(fc1) over one read of the activations (mmdit.py:693-751);
 *   QKNorm + RoPE (mmdit.py:754-764, 934-942) in the tile tail: the columns [kn_col0, kn_col1) are heads of kn_D (128 / 64) columns, normalised with
 *     kn_w [kn_D] and rotated by kn_rope (f32 [S_pos, kn_D / 2, 2], NULL: no rotation) at position kn_pos_off + row % kn_seg_len; qn_w: the columns
 *     [qn_col0, qn_col1) the same way with their own weight (needs kn_w).  Same arithmetic and rounding points as dk_qk_norm_rope_bf16.
 * With (d2, f2) the two problems are issued the way the engines issue the image and text stream of a double block: one grouped launch where the
 * routing rules allow it (same N, K, epilogue), two launches otherwise.  A form a 256-column kernel cannot fuse is expanded into the equivalent
 * sequence of launches (the column ranges one after the other; the projection, then the stand-alone norm pass): dk_gemm_fused_plan tells which. */
typedef struct dk_gemm_side {
  int32_t n_split;
  void* C2;
  int32_t ldc2;
  int32_t epi2;
  const void* kn_w;
  const float* kn_rope;
  int32_t kn_col0, kn_col1, kn_D, kn_pos_off, kn_seg_len;
  float kn_eps;
  const void* qn_w;
  int32_t qn_col0, qn_col1;
} dk_gemm_side;
/* f / f2 may be NULL (nothing fused); d2 NULL: one problem */
int dk_gemm_fused_bf16(const dk_gemm_desc* d, const dk_gemm_side* f, const dk_gemm_desc* d2, const dk_gemm_side* f2, void* stream);
/* dk_gemm_plan of that call: launches == 1 -- fused / grouped in one 256-column kernel; 2 -- expanded */
int dk_gemm_fused_plan(const dk_gemm_desc* d, const dk_gemm_side* f, const dk_gemm_desc* d2, const dk_gemm_side* f2, dk_gemm_plan_t* plan);

typedef struct dk_conv_desc {
  const void* x;    /* NHWC bf16 [B, H(/2), W(/2), C]; C multiple of 64              */
  const void* w;    /* [O, 3, 3, C] bf16 (MLX nn.Conv2d weight layout)               */
  void* y;          /* NHWC bf16 [B, H, W, ldy>=O]                                   */
  const void* bias; /* [O] or NULL                                                   */
  const void* res;  /* DK_EPI_RES: NHWC [B, H, W, ldr]                               */
  const void* zeros;/* >= 128 bytes of zeros on the device (padding taps)            */
  int32_t B, H, W, C, O; /* H, W are OUTPUT sizes                                     */
  int32_t ldy, ldr;
  int32_t upsample; /* 1: conv over the nearest-x2 upsampling of x (vae.py:20-25,146);
                     * 2: stride-2 conv over x = [B, 2H, 2W, C] padded by one zero row / column at the
                     *    bottom / right (the encoder's downsample, vae.py:141-143)          */
  int32_t epilogue;
} dk_conv_desc;

/* nn.Conv2d 3x3 / stride 1 / pad 1 call sites: vae.py:73,79,134,349,384 */
int dk_conv3x3_bf16(const dk_conv_desc* d, void* stream);

/* The norm -> silu -> conv sequence of ResnetBlock2D (vae.py:72-73,78-79,91-100) and of the decoder's output head
 * (conv_norm_out -> silu -> conv_out, vae.py:381,384,397-399) as ONE operator for the high-resolution stage: a 3x3 / stride 1 /
 * pad 1 convolution whose workgroups stage an 18 x 18 halo of the RAW input in LDS per 16 x 16 output tile, applying the
 * GroupNorm (as the per-channel fp32 pair from dk_groupnorm_table_bf16) and the SiLU on the way in -- the normalised tensor is
 * never written.  Optionally: + residual (the block's "+ x", vae.py:100); the 1x1 conv_shortcut of a channel-changing block
 * (vae.py:86-89,98-99) as extra reduction columns over x2 (w = [conv weight | shortcut weight], ldw = 9 C + C2 or more);
 * (sum, M2 about the tile's own mean) partials of the output per channel group for the GroupNorm that reads it next (dk_groupnorm_table_bf16
 * with x == NULL); and, for O <= 4 (conv_out), the clip / uint8 tail of decode_latents_to_image (__init__.py:581-584,525-526).
 * H, W multiples of 16; C (and C2) multiples of 64; O a multiple of 128, or <= 4 with the image tail. */
typedef struct dk_conv_gn_desc {
  const void* x;       /* NHWC bf16 [B, H(/2), W(/2), C]                                          */
  const void* w;       /* bf16 [O, ldw]: column (ky * 3 + kx) * C + c, then 9 C + c2              */
  const void* bias;    /* [O]                                                                      */
  void* y;             /* NHWC bf16 [B, H, W, ldy] (NULL with the image tail)                      */
  const void* res;     /* NHWC bf16 [B, H, W, ldr] or NULL                                         */
  const float* gn_scale_shift; /* [B, 2, C] fp32 from dk_groupnorm_table_bf16, or NULL: x as it is */
  int32_t gn_silu;
  const void* x2;      /* NHWC bf16 [B, H, W, C2] or NULL                                          */
  const void* bias2;   /* [O] or NULL                                                              */
  float* stats_partial;/* [B, (H/16)*(W/16), stats_groups, 2] fp32 or NULL                         */
  float* image_f32;    /* image tail: [B, H, W, 3] in [0, 1]                                       */
  uint8_t* image_u8;   /* ... [B, H, W, 3]                                                         */
  void* raw_bf16;      /* ... conv output, bf16 [B, H, W, 4]                                       */
  int32_t B, H, W, C, O, C2, ldw, ldy, ldr, upsample, stats_groups;
} dk_conv_gn_desc;
int dk_conv3x3_gn_bf16(const dk_conv_gn_desc* d, void* stream);
/* nn.GroupNorm statistics (vae.py:34,72,78,381) as the table dk_conv3x3_gn_bf16 applies: scale = rstd * gamma, shift =
 * beta - mean * scale, fp32 [B, 2, C].  x != NULL: statistics of x (NHWC bf16 [B, HW, C]); x == NULL: from `n_partial` partials
 * per batch row that a dk_conv3x3_gn_bf16 launch left in scratch (layout [B, n_partial, G, 2]: (sum, M2 about the tile's own mean) of
 * one 16 x 16-pixel tile each, so n_partial * 256 must equal HW -- anything else is refused).  scratch:
 * dk_groupnorm_scratch_floats(B, G) floats, or B * n_partial * G * 2 + B * G * 2 if that is more. */
int dk_groupnorm_table_bf16(const void* x, int32_t B, int64_t HW, int32_t C, int32_t G, const void* gamma, const void* beta,
                            float eps, float* scratch, int32_t n_partial, float* scale_shift, void* stream);

/* mx.fast.scaled_dot_product_attention call sites mmdit.py:562,643,687,736.
 * q/k/v: row (b*S + s) at ptr + (b*S + s)*ld + head*D; out likewise with ldo.  D in {64,128}. */
int dk_attention_bf16(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t H,
                      int32_t S, int32_t D, int32_t ld, int32_t ldo, float scale, void* stream);

/* The same by descriptor, with what the engines add to the launch (dk_mmdit_forward; tests/test_gpu_fused_ops.py):
 *   bias (NULL: none): the additive score bias of dk_attention_bias_bf16;
 *   QKNorm + RoPE of the QUERIES inside the kernel's Q load (the keys keep their own pass): token s < qn_split of every batch row is normalised with
 *     qn_a [D], the others with qn_b (both NULL: no norm), eps qn_eps, and rotated by q_rope (f32 [S, D / 2, 2] indexed by s; NULL: no rotation);
 *   O8 (NULL: none): an MX-fp8 copy of the output, row b * S + s at o8_ld bytes per row, head h at byte column h * D, E8M0 scales in O8_scales
 *     (dk_mx_scale_bytes(o8_rows, o8_ld) bytes; any B * S <= o8_rows) -- exactly dk_quantize_mx8 of the bf16 output.  The D = 128 kernels of
 *     "attn" 9 / 10 write it from their accumulators INSTEAD of `out`, which they then leave untouched; the others write `out` and quantise it. */
typedef struct dk_attention_desc {
  const void* q;
  const void* k;
  const void* v;
  void* out;
  int32_t B, H, S, D, ld, ldo;
  float scale;
  const void* bias;
  int64_t bias_head_stride;
  int32_t ldb;
  const void* qn_a;
  const void* qn_b;
  int32_t qn_split;
  float qn_eps;
  const float* q_rope;
  void* O8;
  void* O8_scales;
  int32_t o8_ld;
  int64_t o8_rows; /* rows of the buffer O8 points into (sizes its scale array) */
  /* The caller's bound on |scale * q.k| over the whole launch (natural units, behind the query transform of the Q load); 0: unknown.  Additive in
   * ABI 5 (trailing field: zero the descriptor).  A PROMISE, not checked: with 0 < score_bound, 2 * score_bound * log2(e) <= 64, the fused query
   * load and a launch the one-wave-per-SIMD kernel takes, that kernel's tile loop keeps no running row maximum (dk_attention_plan_t.untracked);
   * scores beyond the bound can then overflow.  QK-normed operands give the bound from the norm weights: max|w_q| * max|w_k| * sqrt(D) * 1.02. */
  float score_bound;
} dk_attention_desc;
int dk_attention_desc_bf16(const dk_attention_desc* d, void* stream);

/* Workspace of the attention launches THIS host thread enqueues (256-byte aligned, dk_attention_workspace_bytes() bytes; NULL: none).
 * The one-wave-per-SIMD D = 128 kernel (attention5.hip) splits the query blocks of a launch's last, partial round of the CUs along the
 * keys and merges the partial results through it.  Optional: without a workspace nothing is split (same results up to the bf16
 * rounding of the partials; FLUX 1024^2, one image: ~10 % longer attention launches).  ONE split launch at a time may use a given
 * workspace: launches that share it must be ordered on one stream.  The pointer is per host thread, not per device -- a thread that
 * moves to another device installs that device's buffer again.  Only the stand-alone dk_attention_* entries read it.  dk_mmdit_* calls
 * neither use nor move it: every engine carves its own region from its workspace and hands it to its attention launches (two engines on two
 * streams never share partial results). */
size_t dk_attention_workspace_bytes(void);
int dk_attention_set_workspace(void* workspace, size_t bytes);

/* What dk_attention_desc_bf16(d) WOULD launch on the current device with a workspace of workspace_bytes bytes (0: none) -- additive in ABI 5.
 * Host only, like dk_gemm_plan: no kernel runs, pointers are not dereferenced (only NULL-ness and alignment are looked at), the arguments are
 * checked as the launch checks them (same refusals, same dk_last_error() text), and without a GPU the rules assume 256 compute units.  The
 * record is read from the route the launch takes (dk_attention_route, attention.hip).  A key split changes the summation order, so `split` is
 * part of the results.
 * One field is an INPUT: o8_split, the engines' row order of the MX-fp8 copy, which no descriptor can name (ragged image token counts of the
 * double blocks: image rows of all batch rows first, the S_t = o8_split text rows of each behind them).  Zero it -- or the whole record -- before
 * the call for the plain order of dk_attention_desc_bf16; it is read only when d->O8 is set. */
typedef struct dk_attention_plan_t {
  int32_t kernel;    /* in the codes of dk_tune_set("attn", .): 4 lean kernel, 9 phase-alternating, 10 one wave per SIMD */
  int32_t qfuse;     /* QKNorm / RoPE of the queries inside the kernel's Q load */
  int32_t blocks;    /* query blocks of 256 rows: B * H * ceil(S / 256) */
  int32_t whole;     /* kernel 10: blocks that run whole (the others: the launch's last, partial round of the CUs); otherwise = blocks */
  int32_t split;     /* key ranges each of the other blocks is cut into (1: none) */
  int32_t jobs;      /* workgroups of those ranges: (blocks - whole) * split, 0 without a split */
  int32_t merge;     /* a merge launch follows (jobs > 0) */
  int32_t quantize;  /* MX-fp8 copy: 0 none, or the kernel writes it; 1 a quantiser pass follows; 2 the same as two row ranges (o8_split) */
  int32_t launches;  /* kernel launches the call expands to */
  int32_t n_cu;      /* compute units the rules assumed */
  int32_t o8_split;  /* INPUT, see above */
  int32_t untracked; /* kernel 10: the tile loop without the running row maximum (d->score_bound admits it and dk_tune_set("attn_track", 1) is not set) */
} dk_attention_plan_t;
int dk_attention_plan(const dk_attention_desc* d, size_t workspace_bytes, dk_attention_plan_t* plan);

/* Identity attention (additive in ABI 5; no reference counterpart -- the perturbation of perturbed-attention guidance, Ahn et al. 2024,
 * diffusers' PAGJointAttnProcessor2_0): the descriptor's attention in which, per batch row and head, with F = ident_from,
 *   a query s <  F (text)   sees every key in [0, S), as in dk_attention_desc_bf16;
 *   a query s >= F (image)  sees the keys [0, F) and its own key s, and nothing else.
 * Softmax and P.V are the plain kernel's; a masked key contributes an exact zero.  No [S, S] mask exists: the lean D = 64 kernel
 * (attention2.hip) walks, for a block of 128 image queries, the ceil(F / 64) key tiles that hold text keys and the two tiles that hold
 * the block's own rows -- 5 tiles instead of 67 at S = 154 + 4096; a block that holds a text query walks every tile.  The fused query
 * load (qn_a / qn_b / qn_split / q_rope) works as in the plain launch.  Text rows below the last multiple of 32 that is <= F are the
 * plain launch's bits; the other text rows (they share a wave with image rows) equal it to rounding.
 * Refused, nothing launched, dk_last_error() names the rule: D != 64; a score bias; an MX-fp8 copy (O8); ident_from outside [1, S).
 * The route is kernel 4 whatever dk_tune_set("attn", .) says.  _f16: fp16 elements.  dk_attention_identity_plan: host only, the same
 * checks and the record dk_attention_plan gives (f16 != 0: of the _f16 entry); plan->o8_split is not read. */
int dk_attention_identity_bf16(const dk_attention_desc* d, int32_t ident_from, void* stream);
int dk_attention_identity_f16(const dk_attention_desc* d, int32_t ident_from, void* stream);
int dk_attention_identity_plan(const dk_attention_desc* d, int32_t ident_from, int32_t f16, dk_attention_plan_t* plan);

/* Single-head attention over head_dim 512: the VAE mid block's Attention (vae.py:28-57: softmax((q / sqrt 512) k^T) v over all
 * H * W tokens), flash-style -- the [T, T] score matrix of the reference (537 MB at T = 16384) is never written.  q / k / v / out:
 * bf16 [B, T, ld] with ld == 512 EXACTLY (dense rows: the transposed copy of v is taken from a dense [T, 512] matrix; any other row
 * pitch is rejected) and ldo >= 512, a multiple of 8; vt_scratch: B * 512 * dk_attention_d512_tp(T) bf16 (the kernel reads a transposed,
 * zero-padded copy of v that this call writes there first). */
int32_t dk_attention_d512_tp(int32_t T);
int dk_attention_d512_bf16(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t T, int32_t ld, int32_t ldo,
                           float scale, void* vt_scratch, void* stream);

/* The same with an additive score bias (text encoders): CLIP's causal mask
 * (clip.py:83-89, one [S, ldb] table for every head: bias_head_stride 0) and T5's relative-position
 * bias (t5.py:61-88, [H, S, ldb]); scores = scale * q.k + bias.  ldb: multiple of 64, >= S. */
int dk_attention_bias_bf16(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t H,
                           int32_t S, int32_t D, int32_t ld, int32_t ldo, float scale, const void* bias,
                           int64_t bias_head_stride, int32_t ldb, void* stream);

/* Text-conditioning helpers (clip.py:28-120, t5.py:60-243):
 * dk_embedding_bf16: out[i,:] = table[ids[i],:] (+ pos[i % pos_rows,:]); out_bf16 and / or out_f32.
 * dk_layernorm_bf16: nn.LayerNorm with weight / bias.   dk_t5_rmsnorm_bf16: the T5 RMSNorm over the fp32 stream.
 * dk_text_elementwise: op 0 y = quick_gelu(a); 1 y = a * b; 2 r_f32 += a.
 * dk_t5_bias_bf16: out[h,q,k] = emb[rel_bucket[k - q + S - 1], h] (rel_bucket: int32 [2S-1], host-computed). */
int dk_embedding_bf16(const void* table, const int32_t* ids, const void* pos, int32_t pos_rows, void* out_bf16,
                      float* out_f32, int32_t n, int32_t dim, int32_t vocab, void* stream);
int dk_layernorm_bf16(const void* x, void* out, int32_t M, int32_t h, const void* weight, const void* bias,
                      float eps, void* stream);
int dk_t5_rmsnorm_bf16(const float* x, void* out, int32_t M, int32_t h, const void* weight, float eps, void* stream);
int dk_text_elementwise(const void* a, const void* b, void* y, float* r, int64_t n, int32_t op, void* stream);
int dk_t5_bias_bf16(const void* emb, const int32_t* rel_bucket, int32_t H, int32_t S, int32_t ld, void* out,
                    void* stream);

/* ---- fp8 path (BASELINE.json configs[3]: fp8 weights, CDNA4 block-scaled fp8 MFMA) -----------------------------------
 * Weights: OCP e4m3 [N, K] + one f32 scale per output channel.  Activations: MX-fp8 = e4m3 [rows, K] + one E8M0 scale byte
 * per row and 32 consecutive columns, the scale bytes in a side array of dk_mx_scale_bytes(rows, K) bytes whose layout is
 * private to the library (written by dk_quantize_mx8 / dk_ln_modulate_mx8 / an MX-fp8 GEMM output, read by dk_gemm_fp8;
 * tests/_fp8.py restates it).  Strides of fp8 buffers are in bytes.  No reference counterpart: the reference quantises
 * weights to 4 bits with MLX (model_io.py:728-734) and keeps fp16 / bf16 activations. */
typedef struct dk_gemm_fp8_desc {
  const void* A;        /* e4m3 [rows, K], row stride lda; logical row m -> (m / a_seg_len) * a_seg_stride + m % a_seg_len */
  const void* A_scales; /* scale side array of the BUFFER A points into                                                  */
  const void* W;        /* e4m3 [N, K], row stride ldw                                                                   */
  const float* w_scale; /* [N]                                                                                           */
  void* C;              /* bf16 [., ldc], or with c_mx8: e4m3 [., ldc] + scales into C_scales                            */
  const void* bias;     /* bf16 [N] or NULL                                                                              */
  const void* gate;     /* as dk_gemm_desc                                                                               */
  const void* res;
  int32_t M, N, K;      /* N % 256 == 0, K % 128 == 0                                                                    */
  int32_t lda, ldw, ldc, ldr;
  int32_t a_seg_len, a_seg_stride; /* M <= a_seg_len (one segment, 0: that): any M; several segments: multiples of 128  */
  int32_t a_row0;       /* physical row of its buffer that A points at (multiple of 128: a row range starts on a scale  */
                        /* block of 128 rows; it may end inside one)                                                     */
  int32_t a_rows;       /* rows of the buffer A points into (sizes its scale array)                                      */
  int32_t c_seg_len, c_seg_stride;
  int32_t r_seg_len, r_seg_stride;
  int32_t gate_seg_len, gate_stride;
  int32_t epilogue;     /* DK_EPI_*                                                                                      */
  int32_t c_mx8;        /* 1: MX-fp8 output (any M; c_row0 % 128 == 0; c_seg_len, c_seg_stride as a_seg_len, a_seg_stride) */
  void* C_scales;
  int32_t c_rows, c_row0, c_col0; /* rows of the output buffer, physical row / column (multiple of 32) that C points at  */
  /* ABI 5: optional K-split scratch, the same buffer and rules as dk_gemm_desc.workspace (dk_gemm_workspace_bytes() bytes, 256-byte aligned, last
   * 4096 bytes zero before the first use): a launch of at most half a round of 256 x 256 tiles with a long reduction is cut along K.  NULL: never. */
  void* workspace;
  size_t workspace_bytes;
} dk_gemm_fp8_desc;
int dk_gemm_fp8(const dk_gemm_fp8_desc* d, void* stream);
/* dk_gemm_side for the fp8 GEMM (the engines' fp8 blocks): the same fields, and c2_mx8 = 1: the second output of the column split leaves as MX-fp8
 * (ldc2 in bytes) into the buffer the descriptor's C_scales / c_rows / c_row0 / c_col0 describe -- the descriptor's own output stays bf16 then
 * (c_mx8 = 0).  With (d2, f2): one grouped launch of two problems with the same N, K, epilogues and split (an error otherwise: this kernel has no
 * expansion).  The fused QKNorm needs a bf16 first output. */
typedef struct dk_gemm_fp8_side {
  int32_t n_split;
  void* C2;
  int32_t ldc2;
  int32_t epi2;
  int32_t c2_mx8;
  const void* kn_w;
  const float* kn_rope;
  int32_t kn_col0, kn_col1, kn_D, kn_pos_off, kn_seg_len;
  float kn_eps;
  const void* qn_w;
  int32_t qn_col0, qn_col1;
} dk_gemm_fp8_side;
int dk_gemm_fp8_fused(const dk_gemm_fp8_desc* d, const dk_gemm_fp8_side* f, const dk_gemm_fp8_desc* d2, const dk_gemm_fp8_side* f2, void* stream);
size_t dk_mx_scale_bytes(int64_t rows, int32_t k);
/* bf16 [M, h] (row stride ldx) -> MX-fp8 rows out_row0 .. of a [out_rows, ldo] e4m3 buffer at column out_col0 (multiple of 32) */
int dk_quantize_mx8(const void* x, int32_t ldx, int32_t M, int32_t h, void* out, int32_t ldo, void* out_scales,
                    int64_t out_rows, int32_t out_row0, int32_t out_col0, void* stream);
/* dk_ln_modulate_bf16 whose output row leaves as MX-fp8 (same arithmetic, same bf16 rounding, then quantised) */
int dk_ln_modulate_mx8(const void* x, int32_t ldx, int32_t M, int32_t h, const void* shift, const void* scale,
                       int32_t mod_stride, int32_t mod_seg_len, float eps, void* out, int32_t ldo, void* out_scales,
                       int64_t out_rows, int32_t out_row0, void* stream);
/* row pitch in bytes of an fp8 matrix with k columns that is read with a long reduction (k + 128 from 8192 on, see dk_weight_pitch) */
int32_t dk_weight_pitch_fp8(int32_t k);

/* affine_transform + LayerNorm, mmdit.py:958-972, 838-849.
 * out[m,:] = LN(x[m,:]) * (1 + scale[b,:]) + shift[b,:], b = m / mod_seg_len. */
int dk_ln_modulate_bf16(const void* x, int32_t ldx, void* out, int32_t ldo, int32_t M, int32_t h,
                        const void* shift, const void* scale, int32_t mod_stride, int32_t mod_seg_len,
                        int32_t x_seg_len, int32_t x_seg_stride, float eps, void* stream);
/* One LayerNorm pass with two modulated outputs (MMDiT-X dual-attention blocks, see dk_mmdit_set_dual_attention): the M rows of x are
 * loaded and reduced once and leave twice, out_a under (shift_a, scale_a) and out_b under (shift_b, scale_b) -- each bit-identical to a
 * dk_ln_modulate_bf16 call with the same operands.  Logical row m of x is physical row (m / mod_seg_len) * x_seg_stride + m % mod_seg_len;
 * the outputs are dense [M, ldo]; modulation row b = m / mod_seg_len at b * mod_stride.  A second, plain row set (x1, out1, M1, shift1,
 * scale1, mod_seg_len1, x_seg_stride1; same ldx / ldo / mod_stride) rides in the same launch as in the engine's double blocks; M1 == 0: none. */
int dk_ln_modulate_dual_bf16(const void* x, void* out_a, void* out_b, int32_t M, const void* shift_a, const void* scale_a,
                             const void* shift_b, const void* scale_b, int32_t mod_seg_len, const void* x1, void* out1, int32_t M1,
                             const void* shift1, const void* scale1, int32_t mod_seg_len1, int32_t ldx, int32_t ldo, int32_t h,
                             int32_t mod_stride, int32_t x_seg_stride, int32_t x_seg_stride1, float eps, void* stream);
/* The LayerNorm pass with a residual tap in front (ControlNet taps, see dk_mmdit_set_control_taps): for each of the M rows of x,
 *   x'[m, :] = round_E( fmaf(s, tap[m, :], x[m, :]) )   fp32 arithmetic, one rounding to the element type E,
 * is stored back over x (in place) and out[m, :] is what dk_ln_modulate_bf16 gives for x' -- bit for bit; the tap is loaded with the row
 * and the row is read once.  tap: [M, ldt] dense rows of E, 16-byte aligned, ldt >= h and ldt % 8 == 0; row m of the tap goes with
 * LOGICAL row m of x (the row map of dk_ln_modulate_dual_bf16).  The second row set (x1 ..., M1 == 0: none) is plain: no tap, and x1 is
 * read only. */
int dk_ln_modulate_add_bf16(void* x, const void* tap, int32_t ldt, float s, void* out, int32_t M, const void* shift, const void* scale,
                            int32_t mod_seg_len, const void* x1, void* out1, int32_t M1, const void* shift1, const void* scale1,
                            int32_t mod_seg_len1, int32_t ldx, int32_t ldo, int32_t h, int32_t mod_stride, int32_t x_seg_stride,
                            int32_t x_seg_stride1, float eps, void* stream);
/* The same pass as ONE job over a joint stream of which only some rows take the residual (FLUX ControlNet taps, see
 * dk_mmdit_set_flux_control_taps; bf16 only).  Logical row m of the M rows is physical row (m / x_seg_len) * x_seg_stride + m % x_seg_len
 * of x (x_seg_len <= 0: M, dense); M is a whole number of groups of tap_seg rows.  Of every group the first tap_first rows (0 <= tap_first <
 * tap_seg: the text rows) are plain -- x is not written there, out is dk_ln_modulate_bf16's -- and row s >= tap_first of group b is first
 * rewritten in place, x' = round_bf16( fmaf(s, tap[b * (tap_seg - tap_first) + (s - tap_first), :], x) ), out = dk_ln_modulate_bf16 of x'.
 * tap: dense [(M / tap_seg) * (tap_seg - tap_first), ldt], 16-byte aligned, ldt >= h, ldt % 8 == 0: it has no rows for the plain rows and
 * nothing is read where they would be.  out: dense [M, ldo]; modulation row m / mod_seg_len at mod_stride elements (mod_seg_len <= 0: M).
 * The engine's two uses: a single block's LayerNorm (x = X, M = B S, tap_seg = S, tap_first = S_t) and the final layer's (x = X + S_t h,
 * x_seg_len = tap_seg = S_i, x_seg_stride = S, tap_first = 0).  dk_ln_modulate_add_bf16's job is the map tap_seg = M, tap_first = 0. */
int dk_ln_modulate_add_joint_bf16(void* x, int32_t ldx, const void* tap, int32_t ldt, float s, int32_t tap_seg, int32_t tap_first, void* out,
                                  int32_t ldo, int32_t M, int32_t h, const void* shift, const void* scale, int32_t mod_stride,
                                  int32_t mod_seg_len, int32_t x_seg_len, int32_t x_seg_stride, float eps, void* stream);

/* QKNorm (mmdit.py:754-764) + RoPE.apply (mmdit.py:934-942), in place on the q / k column groups
 * of a token-major QKV buffer.  q_weight/k_weight NULL = no norm; rope_table NULL = no rotation.
 * rope_table: f32 [S_pos, D/2, 2] (cos, sin); row m uses position pos_off + m % row_seg_len. */
int dk_qk_norm_rope_bf16(void* qkv, int32_t ld, int32_t q_off, int32_t k_off, int32_t rows, int32_t H,
                         int32_t D, const void* q_weight, const void* k_weight, float eps,
                         const float* rope_table, int32_t row_seg_len, int32_t row_seg_stride,
                         int32_t pos_off, void* stream);

/* RoPE.rope / _get_positions, mmdit.py:865-911: table f32 [S_txt + gh*gw, sum(axes)/2, 2] */
int dk_rope_table_f32(float* table, int32_t S_txt, int32_t gh, int32_t gw, const int32_t* axes_dim,
                      int32_t n_axes, float theta, void* stream);
/* The same table for several grids behind the text rows.  seg: host int32 [n_seg][3] = (gh, gw, index), 1 <= n_seg <= 4, positive
 * sides.  Rows: S_txt rows at position (0, 0, 0), then the gh * gw rows of every segment in order at (index, row, col), rows and
 * columns counted from 0 in each segment: table f32 [S_txt + sum gh*gw, sum(axes)/2, 2].  One segment (gh, gw, 0) is
 * dk_rope_table_f32 bit for bit (one kernel behind both).  FLUX.1 Kontext's layout is the image at index 0 and the reference image
 * at index 1 (published sampling code: prepare_kontext). */
int dk_rope_table_segments_f32(float* table, int32_t S_txt, int32_t n_seg, const int32_t* seg, const int32_t* axes_dim,
                               int32_t n_axes, float theta, void* stream);

/* TimestepAdapter.timestep_embedding, mmdit.py:379-389 (quirk Q2). embed_dtype: 0 bf16, 1 fp16, 2 fp32 */
int dk_timestep_embedding_bf16(const float* t_dev, int32_t n, int32_t dim, float max_period,
                               int32_t embed_dtype, void* out, void* stream);

/* LatentImageAdapter patchify, mmdit.py:292-300 (reshape_order=1) / :285-290 (0):
 * latent f32 [n_img,Hl,Wl,C] -> tokens bf16 [n_img*dup, S_i, p*p*C] */
int dk_latent_to_tokens(const float* x, void* tokens, int32_t n_img, int32_t dup, int32_t Hl, int32_t Wl,
                        int32_t C, int32_t p, int32_t reshape_order, void* stream);

/* One Euler step incl. unpatchify, x0 prediction, CFG and re-patchify:
 * CFGDenoiser.__call__ (__init__.py:691-719) after the MMDiT call, to_d (:756),
 * sample_euler body (:778-781), unpack/unpatchify (mmdit.py:304-321, 975-988).
 * x: f32 [n_img,Hl,Wl,C] updated in place; model_out: bf16 [n_img*(1+cfg_on), S_i, ld_out];
 * tokens: next step's patchified input. */
int dk_euler_cfg_step(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img,
                      int32_t cfg_on, int32_t Hl, int32_t Wl, int32_t C, int32_t p, int32_t reshape_order,
                      float sigma, float sigma_next, float cfg_weight, void* stream);

/* Inpainting (latent blending; no reference counterpart): dk_euler_cfg_step followed, in the same launch, by
 *   known = sigma_next * noise + (1 - sigma_next) * x_orig;  x = m * x_new + (1 - m) * known
 * x_orig (process_in of the encoded image) and noise (the draw of the start state): f32 [n_img,Hl,Wl,C] like x;
 * mask: f32 [Hl,Wl] for all images (mask_per_image = 0) or [n_img,Hl,Wl] (1), 1 = repaint, 0 = keep, the same for the C channels
 * of a cell.  Exact ends for finite inputs: m == 1 leaves dk_euler_cfg_step's bits, m == 0 gives known, and with
 * sigma_next == 0 known is x_orig (a value of -0.0f there may come out as +0.0f: the vanishing product is added as a signed zero).  tokens: the rounding of the blended value, in both CFG copies.
 * dk_euler_cfg_step_masked_f16: model_out and tokens are fp16. */
int dk_euler_cfg_step_masked(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img,
                             int32_t cfg_on, int32_t Hl, int32_t Wl, int32_t C, int32_t p, int32_t reshape_order,
                             float sigma, float sigma_next, float cfg_weight, const float* x_orig, const float* noise,
                             const float* mask, int32_t mask_per_image, void* stream);
int dk_euler_cfg_step_masked_f16(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img,
                                 int32_t cfg_on, int32_t Hl, int32_t Wl, int32_t C, int32_t p, int32_t reshape_order,
                                 float sigma, float sigma_next, float cfg_weight, const float* x_orig, const float* noise,
                                 const float* mask, int32_t mask_per_image, void* stream);

/* Second-order samplers (Heun, Adams-Bashforth 2; no reference counterpart): dk_euler_cfg_step with the update as a coefficient row over
 * one caller-owned history buffer hist (f32, shaped like x).  den is formed as dk_euler_cfg_step forms it; then
 *   d = (x - den) / sigma;   x' = cx * x + cd * d + ch * hist;   hist' = hx * x + hd * d   (x before the update)
 * sigma: the sigma of the model evaluation; sigma_next: the sigma x' lives at (read by the masked entries' blend only).
 * reads_h == 0: hist is not read (it may be uninitialised) and ch is ignored; writes_h == 0: hist is not written; hist may be null when
 * both are 0.  A row with reads_h == 0, cx == 1 and cd = sigma_next - sigma (taken in fp32) gives dk_euler_cfg_step's x and tokens bit
 * for bit.  The host computes the rows (diffusionkit_amd/sampler.py: step_plan).  Refused with a dk_last_error() text: sigma == 0, a null
 * hist under a set flag, a non-finite coefficient or sigma.
 * _masked: followed in the same launch by dk_euler_cfg_step_masked's blend with known taken at sigma_next (same operands, same exact ends).
 * _f16: model_out and tokens are fp16. */
int dk_lms_cfg_step(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on,
                    int32_t Hl, int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight,
                    float* hist, float cx, float cd, float ch, float hx, float hd, float sigma_next, int32_t reads_h,
                    int32_t writes_h, void* stream);
int dk_lms_cfg_step_f16(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on,
                        int32_t Hl, int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight,
                        float* hist, float cx, float cd, float ch, float hx, float hd, float sigma_next, int32_t reads_h,
                        int32_t writes_h, void* stream);
int dk_lms_cfg_step_masked(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on,
                           int32_t Hl, int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight,
                           float* hist, float cx, float cd, float ch, float hx, float hd, float sigma_next, int32_t reads_h,
                           int32_t writes_h, const float* x_orig, const float* noise, const float* mask,
                           int32_t mask_per_image, void* stream);
int dk_lms_cfg_step_masked_f16(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on,
                               int32_t Hl, int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight,
                               float* hist, float cx, float cd, float ch, float hx, float hd, float sigma_next, int32_t reads_h,
                               int32_t writes_h, const float* x_orig, const float* noise, const float* mask,
                               int32_t mask_per_image, void* stream);

/* Guidance modes (no reference counterpart): dk_lms_cfg_step with the combination of the two predictions chosen by mode.  With
 * c = xb - o_text * sigma and u = xb - o_neg * sigma formed as dk_lms_cfg_step forms them (fp32), w = cfg_weight, every sum and norm
 * taken per image over its Hl * Wl * C elements:
 *   mode 0 (cfg)      den = u + w (c - u): dk_lms_cfg_step / _masked itself, no other launch; workspace and m are not touched.
 *   mode 1 (rescale)  g = u + w (c - u);  s = phi * std(c) / std(g) + (1 - phi)  (s = 1 if std(g) == 0);  den = g * s.
 *                     phi == 0 gives s == 1.0f and the bits of mode 0.
 *   mode 2 (apg)      D = (c - u) + beta * m under reads_m, else c - u;  m' = D under writes_m;
 *                     a = min(1, r / |D|)  (a = 1 if r <= 0 or |D| == 0);  b = (1 - eta) a <D, c> / <c, c>  (b = 0 if <c, c> == 0);
 *                     den = c + (w - 1)(a D - b c).
 * Everything behind den is dk_lms_cfg_step's: d = (x - den) / sigma, the coefficient row, hist, the blend, the tokens in both copies.
 * x_orig, noise, mask: all null (no blend) or all set (dk_lms_cfg_step_masked's blend).
 * m: f32 shaped like x, caller-owned; read only under reads_m (it may be uninitialised otherwise), written only under writes_m, may be
 * null when both are 0; modes 0 and 1 ignore it and both flags.
 * Modes 1 and 2 run two small launches in front of the step: per-workgroup partial sums (fp32 in the lanes, a fixed butterfly over the
 * wave, fp64 from there on; a workgroup never spans two images), then one wave per image that folds them in a fixed order into the
 * scalars s or (a, b) -- no floating-point atomics, the same bits on every run.  Partials and scalars live in workspace: caller-owned
 * device memory of at least dk_guidance_workspace_bytes(n_img, Hl, Wl, C) bytes, 8-byte aligned, which need not be initialised.
 * Refused with a dk_last_error() text, nothing written: cfg_on == 0, an unknown mode, phi outside [0, 1], a non-finite phi / eta / r /
 * beta / cfg_weight, a null m under a set flag (mode 2), a null or short workspace (modes 1 and 2), and whatever dk_lms_cfg_step refuses.
 * _f16: model_out and tokens are fp16. */
size_t dk_guidance_workspace_bytes(int32_t n_img, int32_t Hl, int32_t Wl, int32_t C);
int dk_guided_cfg_step(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on, int32_t Hl,
                       int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight, float* hist, float cx,
                       float cd, float ch, float hx, float hd, float sigma_next, int32_t reads_h, int32_t writes_h,
                       const float* x_orig, const float* noise, const float* mask, int32_t mask_per_image, int32_t mode, float phi,
                       float eta, float r, float beta, int32_t reads_m, int32_t writes_m, float* m, void* workspace,
                       size_t workspace_bytes, void* stream);
int dk_guided_cfg_step_f16(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on, int32_t Hl,
                           int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight, float* hist,
                           float cx, float cd, float ch, float hx, float hd, float sigma_next, int32_t reads_h, int32_t writes_h,
                           const float* x_orig, const float* noise, const float* mask, int32_t mask_per_image, int32_t mode,
                           float phi, float eta, float r, float beta, int32_t reads_m, int32_t writes_m, float* m, void* workspace,
                           size_t workspace_bytes, void* stream);

/* Skip-layer guidance (no reference counterpart; the sampling recipe published with Stable Diffusion 3.5 medium: diffusers'
 * noise_pred += scale * (noise_pred_text - noise_pred_skip_layers), Stability's SkipLayerCFGDenoiser, restated on x0 predictions):
 * dk_guided_cfg_step on THREE row groups.  model_out is [3 * n_img, S_i, ld_out]: rows [2 n_img, 3 n_img) are the evaluation of the prompt
 * rows with blocks skipped (dk_mmdit_set_skip_layers).  With k = xb - o_skip * sigma formed like c and u (fp32) and G the mode's
 * combination of c and u exactly as above,
 *   den = G(c, u) + slg_scale * (c - k).
 * Everything else is dk_guided_cfg_step's, argument for argument: the moments launches of modes 1 and 2 read rows [0, 2 n_img), the
 * coefficient row, hist, the blend.  tokens are written in the two live copies [0, 2 n_img) only: the engine never reads the third.
 * slg_scale == 0 is accepted and gives dk_guided_cfg_step's bits in every mode for finite predictions (the term is an exact zero).
 * Refused with a dk_last_error() text, nothing written: cfg_on == 0, a non-finite slg_scale, and whatever dk_guided_cfg_step refuses.
 * Verified as arithmetic only, on synthetic weights: no SD3.5-medium checkpoint has been run here.  _f16: model_out and tokens are fp16. */
int dk_slg_cfg_step(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on, int32_t Hl, int32_t Wl,
                    int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight, float* hist, float cx, float cd,
                    float ch, float hx, float hd, float sigma_next, int32_t reads_h, int32_t writes_h, const float* x_orig,
                    const float* noise, const float* mask, int32_t mask_per_image, int32_t mode, float phi, float eta, float r,
                    float beta, int32_t reads_m, int32_t writes_m, float* m, void* workspace, size_t workspace_bytes, float slg_scale,
                    void* stream);
int dk_slg_cfg_step_f16(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on, int32_t Hl,
                        int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight, float* hist, float cx,
                        float cd, float ch, float hx, float hd, float sigma_next, int32_t reads_h, int32_t writes_h,
                        const float* x_orig, const float* noise, const float* mask, int32_t mask_per_image, int32_t mode, float phi,
                        float eta, float r, float beta, int32_t reads_m, int32_t writes_m, float* m, void* workspace,
                        size_t workspace_bytes, float slg_scale, void* stream);

/* Stochastic samplers (no reference counterpart; k-diffusion's sample_euler_ancestral_RF and diffusers'
 * FlowMatchEulerDiscreteScheduler(stochastic_sampling=True) as coefficient rows, sampler.step_plan): the noise is drawn inside the launch.
 * The generator, defined here and restated on the host by sampler.philox4x32_10 / sampler.philox_normal_reference:
 *   Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85, ten rounds of
 *     c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0));
 *   key (seed & 0xffffffff, seed >> 32), seed the image's own; counter (q & 0xffffffff, q >> 32, draw, stream), q = r / 4 with r the
 *     element's index inside its image, draw the schedule index of the row, stream a use tag (0: step noise; other values are reserved);
 *   a block (o0, o1, o2, o3) gives four normals by Box-Muller on 24-bit uniforms: u = ((o_a >> 8) + 1) 2^-24 in (0, 1], theta =
 *     2 pi (o_b >> 8) 2^-24, z_a = sqrt(-2 ln u) cos theta, z_b = sqrt(-2 ln u) sin theta, pairs (o0, o1) -> z0, z1 and (o2, o3) -> z2, z3;
 *     element r takes z[r % 4].
 * A value depends on (seed, r, draw, stream) alone: not on the image's place in the batch, on n_img, on CFG or on the element type.
 *
 * dk_philox_normal_f32: out f32 [n_img, n_per_img], row j = the normals of seeds[j] (u64 [n_img] on the device) for the quads quad_offset,
 * quad_offset + 1, ... (quad_offset reaches the counter's second word without a 2^34-element tensor).  n_per_img % 4 == 0; draw, stream >= 0. */
int dk_philox_normal_f32(float* out, const uint64_t* seeds, int32_t n_img, int64_t n_per_img, int32_t draw, int32_t stream_tag,
                         uint64_t quad_offset, void* stream);
/* dk_noisy_cfg_step: dk_slg_cfg_step's argument list, then the flags that entry implies -- guided (0: the guidance group is not read and mode
 * must be 0; the row may then run with cfg_on = 0, as FLUX does) and slg (0: two row groups, slg_scale is not read) -- and the noise term:
 *   x' = cx x + cd d [+ ch hist] + cn xi(seeds[img], draw, r),
 * behind the update and in front of the masked blend; xi is formed in registers by the function dk_philox_normal_f32 runs (stream 0, quad_offset
 * 0): no noise buffer is read or written, and x' with (cx, cd, cn) = (0, 0, 1) is that operator's output bit for bit, up to the sign of zero.
 * Every case of the row kernel is reachable: masked, the three modes, the third row group, both element types.  cn == 0 launches exactly what
 * dk_lms_cfg_step / _masked / dk_guided_cfg_step / dk_slg_cfg_step launch for the same groups -- their kernels, their bits -- and reads neither
 * seeds nor draw.  Refused with a dk_last_error() text, nothing written: a non-finite cn; cn != 0 with seeds null or draw < 0; Hl * Wl * C not
 * a multiple of 4; guided == 0 with mode != 0; and whatever the groups' own entries refuse.  _f16: model_out and tokens are fp16. */
int dk_noisy_cfg_step(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on, int32_t Hl, int32_t Wl,
                      int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight, float* hist, float cx, float cd,
                      float ch, float hx, float hd, float sigma_next, int32_t reads_h, int32_t writes_h, const float* x_orig,
                      const float* noise, const float* mask, int32_t mask_per_image, int32_t mode, float phi, float eta, float r,
                      float beta, int32_t reads_m, int32_t writes_m, float* m, void* workspace, size_t workspace_bytes, float slg_scale,
                      int32_t guided, int32_t slg, float cn, const uint64_t* seeds, int32_t draw, void* stream);
int dk_noisy_cfg_step_f16(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img, int32_t cfg_on, int32_t Hl,
                          int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float sigma, float cfg_weight, float* hist, float cx,
                          float cd, float ch, float hx, float hd, float sigma_next, int32_t reads_h, int32_t writes_h,
                          const float* x_orig, const float* noise, const float* mask, int32_t mask_per_image, int32_t mode, float phi,
                          float eta, float r, float beta, int32_t reads_m, int32_t writes_m, float* m, void* workspace,
                          size_t workspace_bytes, float slg_scale, int32_t guided, int32_t slg, float cn, const uint64_t* seeds,
                          int32_t draw, void* stream);

/* FlowEdit (Kulikov et al. 2024, "Inversion-Free Text-Based Editing Using Pre-Trained Flow Models"; no reference counterpart): the step of the
 * edit loop, one launch behind every model evaluation.  z, x_src: f32 [n_img, Hl, Wl, C] (z is read and written; x_src is the encoded source
 * image).  model_out / tokens: the engine's [prompt x n, negative x n] layout for n = 2 n_img images, the source rows first:
 *   cfg_on = 0: [src | tar],   cfg_on = 1: [src+ | tar+ | src- | tar-]   (n_img batch rows each).
 * With V the model's output (under cfg_on, neg + w (pos - neg) with w_src on the source rows and w_tar on the target rows):
 *   z'  = z + c (V_tar - V_src)                                  c = (sigma_next - sigma) / n_avg
 *   xi  = the normals of (seeds[img], element r, draw) on stream tag 1, formed in registers by the function dk_philox_normal_f32 runs
 *   Zs  = (1 - sigma_in) x_src + sigma_in xi,   Zt = Zs + (z' - x_src)
 * Zs and Zt are written in fp32 to zs_out (may be NULL) and zt_out, and rounded and patchified into the source and target rows of tokens,
 * under cfg_on into both copies, as dk_latent_to_tokens writes them.  prime = 1: model_out is not read (may be NULL) and z is neither changed
 * nor written -- the launch that forms the first inputs.  Equal source and target rows with w_src == w_tar leave the bits of z; z == x_src
 * gives zt_out the bits of zs_out, up to the sign of a zero.  Stream tag 1 keeps the draws apart from those of a stochastic sampler (tag 0).
 * Refused with a dk_last_error() text, nothing written: a null z, x_src, tokens, zt_out or seeds, or a null model_out without prime; sizes that
 * are not positive or not divisible by p; C not a multiple of 4; ld_out below p * p * C or not a multiple of 4; z, x_src, zs_out, zt_out not
 * 16-byte aligned; model_out or tokens not 8-byte aligned; a non-finite w_src, w_tar, c or sigma_in; draw < 0.  _f16: model_out and tokens
 * are fp16. */
int dk_flowedit_step(float* z, const float* x_src, const void* model_out, int32_t ld_out, void* tokens, float* zs_out, float* zt_out,
                     int32_t n_img, int32_t cfg_on, int32_t Hl, int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float w_src, float w_tar,
                     float c, float sigma_in, const uint64_t* seeds, int32_t draw, int32_t prime, void* stream);
int dk_flowedit_step_f16(float* z, const float* x_src, const void* model_out, int32_t ld_out, void* tokens, float* zs_out, float* zt_out,
                         int32_t n_img, int32_t cfg_on, int32_t Hl, int32_t Wl, int32_t C, int32_t p, int32_t reshape_order, float w_src,
                         float w_tar, float c, float sigma_in, const uint64_t* seeds, int32_t draw, int32_t prime, void* stream);

/* Inpainting mask, pixels -> latent cells: mask u8 [n_mask,H,W] (255 = repaint, 0 = keep) -> f32 [n_mask,H/f,W/f],
 * (integer sum of the f x f block) / (f * f * 255) by a true division: an all-0 block gives 0.0f, an all-255 block 1.0f.
 * H and W must be multiples of f (the pipeline passes the VAE's factor, 8). */
int dk_mask_to_latent_f32(const uint8_t* mask, float* out, int32_t n_mask, int32_t H, int32_t W, int32_t f, void* stream);

/* Inpainting paste-back: out = (uint8)(w * dec + (1 - w) * orig + 0.5f), w = mask / 255.0f, in plain fp32 (nothing fused):
 * the decoder's bytes where mask == 255, the original's where mask == 0.  dec, out: u8 [B,H,W,3]; orig: u8 [H,W,3]
 * (orig_per_image = 0) or [B,H,W,3] (1); mask: u8 [H,W] (mask_per_image = 0) or [B,H,W] (1). */
int dk_image_composite_u8(const uint8_t* dec, const uint8_t* orig, const uint8_t* mask, uint8_t* out, int32_t B,
                          int32_t H, int32_t W, int32_t orig_per_image, int32_t mask_per_image, void* stream);

/* Channel-concatenated conditioning (FLUX.1 Fill; published sampling code: prepare_fill), the image the model may look at:
 * out = a * (1 - m) with a = u8 / 255 * 2 - 1 and m = mask / 255 (not binarised; 1 = repaint), every operation rounded to fp32 on its
 * own, nothing fused: the bits of the same numpy float32 expression.  image: u8 [n,H,W,3]; mask: u8 [n_mask,H,W], n_mask = 1 (one
 * mask for every image) or n; out: f32 [n,H,W,3]. */
int dk_image_mask_out_f32(const uint8_t* image, const uint8_t* mask, float* out, int32_t n, int32_t n_mask, int32_t H, int32_t W,
                          void* stream);
/* ... and the condition's token rows (prepare_fill / prepare_control), one launch: z f32 [n,Hl,Wl,C] (the encoded, process_in'ed
 * condition latent), mask u8 [n_mask,8*Hl,8*Wl] or NULL -> tokens bf16 [n, S_i, p*p*C (+ 64*p*p with a mask)], S_i = (Hl/p)*(Wl/p).
 * Columns [0, p*p*C): the bits dk_latent_to_tokens(reshape_order = 1) writes for z, features (c, ph, pw).  Columns behind them (Fill):
 * the mask's 8 x 8 pixel-unshuffle to 64 channels at latent resolution (channel 8*py + px) through the same patchify: for token (i, j),
 * column p*p*C + p*p*(8*py + px) + p*ph + pw = bf16(mask[8*(p*i + ph) + py, 8*(p*j + pw) + px] / 255).  NULL mask: the control layout
 * (FLUX.1 Canny / Depth), the latent columns only; n_mask is then ignored. */
int dk_fill_condition_tokens(const float* z, const uint8_t* mask, void* tokens, int32_t n, int32_t n_mask, int32_t Hl, int32_t Wl,
                             int32_t C, int32_t patch, void* stream);

/* LatentFormat.process_in/out, __init__.py:729-733: y = x * a + b (f32) */
int dk_affine_f32(const float* x, float* y, int64_t n, float a, float b, void* stream);

/* ---- float16 element type (the reference's dtype for Stable Diffusion 3, config.py:77-79) ----------------------------------
 * Siblings of the *_bf16 operators above on IEEE-half tensors: same descriptors, strides in elements, 16-bit storage, fp32
 * accumulation, the same rounding points with fp16 in place of bf16.  An fp32 -> fp16 store that overflows gives +-inf, as the
 * reference's casts do (no clamp).  Every tensor a descriptor names (A, W, C, bias, gate, res, norm weights, q / k / v / out) is
 * fp16; RoPE tables, the latent and timesteps stay fp32.
 *  - GEMM: the route is the 128 x 128 kernel or the 256-column 8-wave kernel (generation 3) -- dk_gemm_plan_f16 never reports
 *    generation 4, and dk_tune_set("gemm", 10) / ("gemm_v4", v) have no effect on these launches.  The implicit-GEMM convolution
 *    (dk_conv3x3_f16) takes the same two kernels' conv forms; dk_conv3x3_plan_f16 reports its route.
 *  - Attention: head_dim 64, no score bias, no MX-fp8 copy; always the lean kernel (dk_tune_set("attn", 9 / 10) have no effect;
 *    dk_attention_plan_f16 reports the route and refuses what the launch refuses).
 *    Scores, running maximum and sum in fp32, P rounded to fp16 for the P.V product.
 *  - dk_timestep_embedding_f16: evaluated in `embed_dtype` as before, stored as fp16.
 *  - dk_euler_cfg_step_f16 / dk_latent_to_tokens_f16: model_out and tokens are fp16, the latent stays fp32. */
int dk_gemm_f16(const dk_gemm_desc* d, void* stream);
int dk_gemm_plan_f16(const dk_gemm_desc* d, const dk_gemm_desc* d2, dk_gemm_plan_t* plan);
int dk_gemm_fused_f16(const dk_gemm_desc* d, const dk_gemm_side* f, const dk_gemm_desc* d2, const dk_gemm_side* f2, void* stream);
int dk_attention_desc_f16(const dk_attention_desc* d, void* stream);
int dk_attention_plan_f16(const dk_attention_desc* d, size_t workspace_bytes, dk_attention_plan_t* plan);
int dk_ln_modulate_f16(const void* x, int32_t ldx, void* out, int32_t ldo, int32_t M, int32_t h,
                       const void* shift, const void* scale, int32_t mod_stride, int32_t mod_seg_len,
                       int32_t x_seg_len, int32_t x_seg_stride, float eps, void* stream);
int dk_ln_modulate_dual_f16(const void* x, void* out_a, void* out_b, int32_t M, const void* shift_a, const void* scale_a,
                            const void* shift_b, const void* scale_b, int32_t mod_seg_len, const void* x1, void* out1, int32_t M1,
                            const void* shift1, const void* scale1, int32_t mod_seg_len1, int32_t ldx, int32_t ldo, int32_t h,
                            int32_t mod_stride, int32_t x_seg_stride, int32_t x_seg_stride1, float eps, void* stream);
int dk_ln_modulate_add_f16(void* x, const void* tap, int32_t ldt, float s, void* out, int32_t M, const void* shift, const void* scale,
                           int32_t mod_seg_len, const void* x1, void* out1, int32_t M1, const void* shift1, const void* scale1,
                           int32_t mod_seg_len1, int32_t ldx, int32_t ldo, int32_t h, int32_t mod_stride, int32_t x_seg_stride,
                           int32_t x_seg_stride1, float eps, void* stream);
int dk_qk_norm_rope_f16(void* qkv, int32_t ld, int32_t q_off, int32_t k_off, int32_t rows, int32_t H,
                        int32_t D, const void* q_weight, const void* k_weight, float eps, const float* rope_table,
                        int32_t row_seg_len, int32_t row_seg_stride, int32_t pos_off, void* stream);
int dk_timestep_embedding_f16(const float* t_dev, int32_t n, int32_t dim, float max_period,
                              int32_t embed_dtype, void* out, void* stream);
int dk_latent_to_tokens_f16(const float* x, void* tokens, int32_t n_img, int32_t dup, int32_t Hl, int32_t Wl,
                            int32_t C, int32_t p, int32_t reshape_order, void* stream);
int dk_euler_cfg_step_f16(float* x, const void* model_out, int32_t ld_out, void* tokens, int32_t n_img,
                          int32_t cfg_on, int32_t Hl, int32_t Wl, int32_t C, int32_t p, int32_t reshape_order,
                          float sigma, float sigma_next, float cfg_weight, void* stream);

/* The VAE's operators on IEEE-half tensors (the reference decodes SD3 latents with an fp16 decoder, mlx/__init__.py:108-113,483-484):
 * same descriptors and scratch sizes as their *_bf16 siblings, every 16-bit tensor they name is fp16 (gamma / beta included), statistics, tables
 * and accumulators stay fp32, the rounding points are the same with fp16 in place of bf16.
 *  - dk_conv3x3_gn_f16: always conv_halo.hip's kernel -- the one-wave-per-SIMD frame (conv256v4.hip, generated asm body) is bf16 only, and
 *    dk_tune_set("conv_v4", v) has no effect on fp16 launches.  Image tail: raw, raw / 2 + 0.5 and img * 255 are rounded to fp16
 *    (uint8 image = truncation of the fp16 product, __init__.py:525-526).
 *  - dk_attention_d512_f16: scores, running maximum and sum in fp32, P rounded to fp16 for the P.V product.
 *  - dk_conv3x3_plan / dk_conv3x3_plan_f16: dk_gemm_plan of a dk_conv3x3_* call (host only, nothing is launched, pointers are not read). */
int dk_conv3x3_f16(const dk_conv_desc* d, void* stream);
int dk_conv3x3_plan(const dk_conv_desc* d, dk_gemm_plan_t* plan);
int dk_conv3x3_plan_f16(const dk_conv_desc* d, dk_gemm_plan_t* plan);
/* dk_conv3x3_bf16 / _f16 with the K-split scratch the VAE engines attach to their 3x3 convs -- additive in ABI 5.  `workspace`: the same buffer
 * and rules as dk_gemm_desc.workspace (dk_gemm_workspace_bytes() bytes, 256-byte aligned, LAST 4096 bytes zero before the first use; the kernels
 * leave them zero; one launch at a time may use it).  With it a convolution with O % 256 == 0 whose 256 x 256 tiles fill about half the compute
 * units (96 .. 128 tiles: an unfused 256-channel stage of a few thousand pixels) runs on gemm256v3.hip's conv form with every tile cut in two
 * along K; other shapes take the route of dk_conv3x3_bf16.  A NULL, misaligned or short workspace is refused (dk_last_error() names the rule):
 * the launch never silently runs unsplit.  dk_conv3x3_ws_plan / _plan_f16: dk_gemm_plan of that call for a workspace of workspace_bytes bytes
 * (0: none -- the answer of dk_conv3x3_plan; a size above 0 that is too small is refused as the launch refuses it). */
int dk_conv3x3_ws_bf16(const dk_conv_desc* d, void* workspace, size_t workspace_bytes, void* stream);
int dk_conv3x3_ws_f16(const dk_conv_desc* d, void* workspace, size_t workspace_bytes, void* stream);
int dk_conv3x3_ws_plan(const dk_conv_desc* d, size_t workspace_bytes, dk_gemm_plan_t* plan);
int dk_conv3x3_ws_plan_f16(const dk_conv_desc* d, size_t workspace_bytes, dk_gemm_plan_t* plan);
int dk_conv3x3_gn_f16(const dk_conv_gn_desc* d, void* stream);
int dk_groupnorm_table_f16(const void* x, int32_t B, int64_t HW, int32_t C, int32_t G, const void* gamma, const void* beta,
                           float eps, float* scratch, int32_t n_partial, float* scale_shift, void* stream);
int dk_groupnorm_f16(const void* x, void* y, int32_t B, int64_t HW, int32_t C, int32_t G, const void* gamma,
                     const void* beta, float eps, int32_t fuse_silu, float* scratch_f32, void* stream);
int dk_attention_d512_f16(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t T, int32_t ld, int32_t ldo,
                          float scale, void* vt_scratch, void* stream);
int dk_softmax_rows_f16(void* x, int32_t rows, int32_t cols, int32_t ld, void* stream);
int dk_transpose_f16(const void* x, void* y, int32_t R, int32_t C, void* stream);

/* nn.GroupNorm(pytorch_compatible=True) [+ nn.silu], vae.py:34,72,78,381,91,96,398.
 * x, y: NHWC bf16 [B, HW, C]; scratch_f32 needs dk_groupnorm_scratch_floats(B, G) floats. */
size_t dk_groupnorm_scratch_floats(int32_t B, int32_t G);
int dk_groupnorm_bf16(const void* x, void* y, int32_t B, int64_t HW, int32_t C, int32_t G, const void* gamma,
                      const void* beta, float eps, int32_t fuse_silu, float* scratch_f32, void* stream);

/* mx.softmax(scores, axis=-1), vae.py:51: in place over rows of a bf16 matrix */
int dk_softmax_rows_bf16(void* x, int32_t rows, int32_t cols, int32_t ld, void* stream);
int dk_transpose_bf16(const void* x, void* y, int32_t R, int32_t C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Model level: MMDiT (mmdit.py:22-266) and VAEDecoder (vae.py:336-401)
 * ---------------------------------------------------------------------------------------- */
typedef struct dk_mmdit_config {
  int32_t num_heads, depth_multimodal, depth_unified, hidden_size, mlp_ratio;
  int32_t vae_latent_dim, patch_size, patchify_via_reshape;
  int32_t use_qk_norm, use_rope, rope_axes_dim[4], n_rope_axes, rope_theta;
  int32_t use_pos_embed, max_latent_resolution;
  int32_t pooled_text_embed_dim, token_level_text_embed_dim, frequency_embed_dim, max_period;
  int32_t embed_dtype; /* dtype the timestep embedding is evaluated in: 0 bf16, 1 fp16, 2 fp32 */
  float layer_norm_eps;
  /* 1: the FLUX.1-dev guidance embedding (MLPEmbedder "guidance_in", mmdit.py:31-36,945-955, config.py:97-111) is added to
   * the modulation vector; needs the guidance_in.mlp.layers.{0,2}.{weight,bias} tensors and dk_mmdit_set_guidance.
   * 0 (the reference's behaviour: model_io.py:109 runs FLUX.1-dev on the schnell preset, quirk Q7): absent. */
  int32_t guidance_embed;
  /* 1: the Linear layers of the transformer blocks (q/k/v, o_proj, fc1, fc2, linear1, linear2) run on the fp8 MFMA with
   * e4m3 weights ("<name>.weight_fp8" uint8 [N, dk_weight_pitch_fp8(K)] + "<name>.wscale" f32 [N] instead of
   * "<name>.weight") and MX-fp8 activations quantised on the fly (BASELINE.json configs[3]; the reference's counterpart is
   * its 4-bit nn.QuantizedLinear checkpoints, model_io.py:728-734,772-775).  Needs head_dim 128 and a text length that is
   * one of the multiples of 128; the image token count is free (dk_mmdit_prepare).  0: bf16 weights. */
  int32_t fp8_linears;
  /* fp8 precision policy (round 5; only read with fp8_linears): the Linears of the first fp8_bf16_double_blocks double-stream blocks
   * stay bf16 ("<name>.weight", bf16 activations, the bf16 GEMM): errors made in the first blocks travel through all 57 -- measured
   * dB per step against what the blocks cost in DESIGN.md section 4.  0: every block on the fp8 path. */
  int32_t fp8_bf16_double_blocks;
} dk_mmdit_config;

typedef struct dk_mmdit dk_mmdit;

int dk_mmdit_create(const dk_mmdit_config* cfg, dk_mmdit** out);
void dk_mmdit_destroy(dk_mmdit* m);

/* Weight binding by name (model.load_weights / model.update, model_io.py:743,783).  Names follow
 * the reference module tree with the fused tensors of diffusionkit_amd/weights.py:
 *   <block>.attn.qkv.{weight,bias}, <single block>.linear2.{weight,bias}, adaLN.{weight,bias}.
 * The pointer must stay valid for the lifetime of the handle. */
int dk_mmdit_bind(dk_mmdit* m, const char* name, const void* dev_ptr);
/* number of hidden_size-wide rows of the packed adaLN output, and the row offset of one module
 * (kind 0 image stream of double block i, 1 text stream, 2 single block i, 3 final layer) */
int dk_mmdit_mod_rows(const dk_mmdit* m);
int dk_mmdit_mod_offset(const dk_mmdit* m, int32_t kind, int32_t index);
/* The bound on |scale * q.k| the engine hands the joint attention launch of a block (dk_attention_desc.score_bound): max|w_q| * max|w_k| * sqrt(D) *
 * 1.02 over the QKNorm weights of the block's streams, read from the device once, in the first dk_mmdit_prepare behind a dk_mmdit_bind.  kind 0:
 * double block `index` (both streams), 2: single block `index` (the kinds of dk_mmdit_mod_offset).  0: unknown -- no QKNorm weights, not bf16, not
 * prepared yet, or no such block.  Additive in ABI 5. */
float dk_mmdit_score_bound(const dk_mmdit* m, int32_t kind, int32_t index);

size_t dk_mmdit_workspace_bytes(const dk_mmdit* m, int32_t batch, int32_t latent_h, int32_t latent_w,
                                int32_t text_len, int32_t n_timesteps);
/* fixes the problem shape, carves the workspace, builds RoPE table / cropped pos-emb */
int dk_mmdit_prepare(dk_mmdit* m, int32_t batch, int32_t latent_h, int32_t latent_w, int32_t text_len,
                     int32_t n_timesteps, void* workspace, size_t workspace_bytes, void* stream);

/* MMDiT.cache_modulation_params(pooled_text_embeddings, timesteps), mmdit.py:77-180.
 * pooled: bf16 [batch, pooled_dim] on the device; timesteps: n host floats (already rounded to
 * the activation dtype by the caller, quirk Q1). */
int dk_mmdit_cache_modulation_params(dk_mmdit* m, const void* pooled, const float* timesteps_host,
                                     int32_t n, void* stream);
/* Guidance strength fed to the guidance embedding (configs with guidance_embed = 1; FLUX.1-dev's distilled guidance, 3.5 by
 * default): the next dk_mmdit_cache_modulation_params adds guidance_in(timestep_embedding(1000 * guidance)) to every
 * modulation vector -- the published FLUX.1-dev conditioning, which the reference's module tree declares (mmdit.py:31-36)
 * but whose call site (:219-220) it never reaches (quirk Q7). */
int dk_mmdit_set_guidance(dk_mmdit* m, float guidance);
/* ... or one strength per batch row (FlowEdit on FLUX.1-dev evaluates its source and target rows at different values): g holds n host floats,
 * n the prepared batch, so the call follows dk_mmdit_prepare, and a later dk_mmdit_prepare forgets the rows.  The next
 * dk_mmdit_cache_modulation_params embeds the n values (timestep embedding and the two guidance_in Linears at M = n) and adds row b's vector to
 * batch row b.  g == NULL or n == 0 returns to the scalar of dk_mmdit_set_guidance; with the rows unset the launches and the table are exactly
 * the scalar's.  Refused with a dk_last_error() text: a configuration without guidance_embed, an engine not yet prepared, n != batch, a
 * non-finite value. */
int dk_mmdit_set_guidance_rows(dk_mmdit* m, const float* g, int32_t n);

/* Element type of the engine: 0 = bfloat16 (default), 1 = float16.  Call after dk_mmdit_create and before the first
 * dk_mmdit_bind.  With 1 every bound weight / bias / table is fp16, every activation buffer holds fp16 (sizes unchanged), and
 * tokens, text and pooled go in and come out as fp16; the modulation table, the context_embedder hoist and the final layer
 * included.  Accepted only for SD3-family geometry -- head_dim == 64, depth_unified == 0, fp8_linears == 0 -- anything else
 * returns an error that names the rule (dk_last_error). */
int dk_mmdit_set_activation_dtype(dk_mmdit* m, int32_t dtype);

/* Step-invariant hoist of `self.context_embedder(token_level_text_embeddings)` (mmdit.py:195, recomputed by the reference
 * in every MMDiT.__call__): embeds `text` (bf16 [batch, S_t, text_dim]) once into the engine's workspace; later
 * dk_mmdit_forward calls with text == NULL copy that result into the joint stream instead of recomputing it (same values).
 * Invalidated by dk_mmdit_prepare. */
int dk_mmdit_cache_context(dk_mmdit* m, const void* text, void* stream);

/* MMDiT.__call__ (mmdit.py:188-266) between patchify and unpatchify, for cached timestep
 * `step_index` (quirk Q11: index instead of float key).
 * tokens_in: bf16 [batch, S_i, p*p*C]; text: bf16 [batch, S_t, text_dim], or NULL after dk_mmdit_cache_context;
 * tokens_out: bf16 [batch, S_i, p*p*C] (FinalLayer output). */
int dk_mmdit_forward(dk_mmdit* m, const void* tokens_in, const void* text, int32_t step_index,
                     void* tokens_out, void* stream);
/* MultiModalTransformerBlock.__call__ / UnifiedTransformerBlock.__call__ (mmdit.py:568-675, 693-751) on a caller-supplied
 * residual stream: copies x_in (bf16 [batch, S, h], the engine's joint layout: text rows first, then image rows, per batch row)
 * into the engine's stream, runs blocks [first_block, first_block + n_blocks) of the global order (double blocks
 * 0 .. depth_multimodal - 1, then the single blocks) with the modulation parameters cached for `step_index`, and copies the
 * stream to x_out.  The operator-level boundary of one reference block: the teacher-forced parity tests drive single blocks
 * of the full-size model through it (tests/test_gpu_fullsize.py). */
int dk_mmdit_run_blocks(dk_mmdit* m, const void* x_in, void* x_out, int32_t step_index, int32_t first_block,
                        int32_t n_blocks, void* stream);
/* read-only view of an internal buffer for parity taps: 0 = joint residual stream [B,S,h],
 * 1 = modulation table [n*B, rows*h], 2 = base of the engine's GEMM K-split workspace (dk_gemm_workspace_bytes() bytes:
 * the fp32 slabs, then the 4096-byte flag region, which is zero between launches); with the first-block cache on, image rows only
 * [B * S_i, h]: 3 = R, 4 = D_ref, 5 = D_cur (the probe's output, between a head and its tail; a compute tail makes it D_ref); NULL with the cache off;
 * 6 = CONDE [B, S_i, h], x_embedder's condition share (dk_mmdit_cache_condition); NULL without a condition width */
const void* dk_mmdit_debug_buffer(const dk_mmdit* m, int32_t which);

/* ---- first-block cache (opt-in; no reference counterpart) -------------------------------------------------------------------
 * A step is split into a head -- embedders, block 0, a probe of what block 0 did to the image rows -- and a tail that either
 * computes blocks 1 .. L-1 or reuses their cached effect.  All of it acts on the image rows of the joint stream X [B, S, h], in
 * the engine's element type E, fp32 arithmetic with one round-to-nearest-even to E per stored value.  With X0 the stream behind
 * the embedders, X1 behind block 0 and X_L behind the last block:
 *   D_cur = round_E(X1 - X0);  num[b] = sum |D_cur - D_ref|,  den[b] = sum |D_ref|  over the S_i * h image elements of batch row b,
 *   with D_ref the D_cur of the last COMPUTED step since the cache was reset.  The sums are fp32, built without atomics in a
 *   fixed order (per lane, per wave, per batch row): the same bits on every run and every CU count.
 *   compute tail: blocks 1 .. L-1 and the final layer as in dk_mmdit_forward; R = round_E(X_L - X1); D_ref <- D_cur.
 *   reuse tail:   image rows X <- round_E(X1 + R), text rows as block 0 left them, then the final layer; D_ref and R stay.
 * A model whose block 0 is its only block is accepted: the compute tail's block range is empty and R is all +0.
 *
 * dk_mmdit_set_block_cache: call before dk_mmdit_prepare (a prepared engine must be prepared again).  on != 0 adds three image-row
 * buffers [B * S_i, h] and the probe's per-row partial sums behind everything else in the workspace; with 0 (the default)
 * dk_mmdit_workspace_bytes, the carve and every launch of dk_mmdit_forward are what they are without the feature.
 * dk_mmdit_forward keeps working on a cache-enabled engine: it drops a pending head and leaves R / D_ref alone.
 * dk_mmdit_prepare, dk_mmdit_cache_modulation_params and dk_mmdit_reset_block_cache invalidate the cache (and a pending head).
 * None of these entries synchronises: probe_out is valid in stream order, the caller reads it. */
int dk_mmdit_set_block_cache(dk_mmdit* m, int32_t on);
int dk_mmdit_reset_block_cache(dk_mmdit* m);

/* ---- reference-image conditioning (opt-in; FLUX.1 Kontext's token layout, no counterpart in the reference) ---------------------
 * The joint sequence of every batch row becomes [text (S_t) | image (S_i) | reference (S_r)], S_r = (ref_latent_h / p) *
 * (ref_latent_w / p): the VAE-encoded reference image rides behind the image rows as extra rows of the IMAGE stream (published
 * Kontext sampling code: img = cat(img, img_cond), pred[:, :S_i]).  Inside the blocks the reference rows are image-stream rows --
 * image weights and modulation in double blocks, the one stream of single blocks, queries / keys / values of the joint attention --
 * at RoPE positions (1, row, col) of their own grid (dk_rope_table_segments_f32).  The final layer, tokens_in / tokens_out, the
 * first-block cache's probe / R / D_ref / D_cur buffers keep covering the S_i image rows only; debug buffer 0 is [B, S, h] with
 * S = S_t + S_i + S_r.
 * Verified against an fp32 / bf16-emulating oracle of this layout with synthetic weights (arithmetic parity); no Kontext checkpoint
 * has been run through it.
 *
 * dk_mmdit_set_reference_grid: call before dk_mmdit_prepare (a prepared engine must be prepared again).  (0, 0), the default, turns
 * the feature off: dk_mmdit_workspace_bytes, the carve and every launch of every entry are then what they are without it.  Refused,
 * with no state changed: a configuration without RoPE (use_rope == 0: the SD3 family has no position index to tell the reference
 * from the image), sides that are not positive multiples of patch_size, one side zero and the other not.
 * dk_mmdit_cache_reference: ref_tokens in the engine's element type, [batch, S_r, p*p*C] (per_image != 0) or [1, S_r, p*p*C]
 * (per_image == 0: one reference for every batch row), as dk_latent_to_tokens_* makes them from the reference latent.  Runs
 * x_embedder on them once into the workspace (step-invariant, like dk_mmdit_cache_context); every later forward / head copies the
 * result behind the image rows of every batch row.  Invalidated by dk_mmdit_prepare.  dk_mmdit_forward, dk_mmdit_forward_head and
 * dk_mmdit_run_blocks on an engine with a reference grid but no cached reference return an error that names the rule, never
 * launch. */
int dk_mmdit_set_reference_grid(dk_mmdit* m, int32_t ref_latent_h, int32_t ref_latent_w);
int dk_mmdit_cache_reference(dk_mmdit* m, const void* ref_tokens, int32_t per_image, void* stream);

/* ---- channel-concatenated conditioning (opt-in; FLUX.1 Fill / Canny / Depth, no counterpart in the reference) ---------------------
 * These checkpoints are FLUX.1-dev with a wider img_in: x_embedder.proj.weight is [h, F + cond_features] row-major (F = p*p*C), and
 * every model evaluation embeds cat(tokens, cond_tokens) on the feature axis (published sampling code: prepare_fill / prepare_control);
 * the model still predicts F features per token.  The condition is step-invariant, so its share of the sum is computed once,
 * CONDE[b] = cond[b] . W[:, F:]^T (no bias, rounded to bf16), and the x_embedder launch of every evaluation becomes
 * Linear(tokens [.., F], W with row stride F + cond_features, bias, DK_EPI_RES, residual = CONDE): bf16(bf16(tokens . W[:, :F]^T + bias)
 * + CONDE).  tokens_in / tokens_out, the step kernels and every other buffer keep their widths.
 * Verified against an fp32 / bf16-emulating oracle of this layout with synthetic weights (arithmetic parity); no Fill / Canny / Depth
 * checkpoint has been run through it.
 *
 * dk_mmdit_set_condition_width: call before dk_mmdit_prepare (a prepared engine must be prepared again: CONDE is one more carve).  0,
 * the default, turns the feature off: dk_mmdit_workspace_bytes, the carve and every launch are then what they are without it.
 * Refused, with no state changed: a width that is not a positive multiple of 64, a configuration with use_pos_embed != 0 (its
 * positional table holds the residual slot of the x_embedder launch), fp16 activations, a reference grid set at the same time
 * (dk_mmdit_set_reference_grid refuses the other way round).  dk_mmdit_bind cannot see sizes: the caller must make sure that the bound
 * x_embedder.proj.weight holds F + cond_features columns (MMDiTEngine checks it before binding).
 * dk_mmdit_cache_condition: cond_tokens bf16 [batch, S_i, cond_features] (per_image != 0) or [1, S_i, cond_features] (per_image == 0:
 * one condition for every batch row; one launch per batch row either way, so the bits are those of a repeated condition), as
 * dk_fill_condition_tokens makes them.  Resets the first-block cache; invalidated by dk_mmdit_prepare.  dk_mmdit_forward,
 * dk_mmdit_forward_head and dk_mmdit_run_blocks on an engine with a condition width but no cached condition return an error that
 * names the rule, never launch. */
int dk_mmdit_set_condition_width(dk_mmdit* m, int32_t cond_features);
int dk_mmdit_cache_condition(dk_mmdit* m, const void* cond_tokens, int32_t per_image, void* stream);

/* ---- MMDiT-X dual-attention blocks (opt-in; Stable Diffusion 3.5 medium, no counterpart in the reference) ---------------------------
 * The first n_blocks double blocks carry a second self-attention over the image-stream rows alone (published model definition:
 * Stability's mmditx.py x_block.attn2, diffusers' JointTransformerBlock(use_dual_attention=True)).  The image module of such a block has
 * NINE modulation rows -- shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp, shift_msa2, scale_msa2, gate_msa2: the first six
 * are the row order of every other block -- and the block computes, with n = LN(x) taken once,
 *   m1 = n (1 + scale_msa) + shift_msa  -> attn.qkv  -> the joint attention with the text stream, as in every double block
 *   m2 = n (1 + scale_msa2) + shift_msa2 -> attn2.qkv -> QK-RMSNorm (attn2's own weights, eps 1e-6) -> SDPA over the image rows of each
 *        batch row alone (same heads, head_dim and 1 / sqrt(D) scale; no text rows, no RoPE)
 *   x += gate_msa * attn.o_proj(joint attention's image rows);  x += gate_msa2 * attn2.o_proj(a2);  then the MLP half, unchanged.
 * One rounding per Linear output, modulate, norm and gated add, as in the existing block.  The text stream of a dual block and the
 * blocks i >= n_blocks are what they are without the feature.
 * Bound names, required for image streams i < n_blocks and refused (at resolve time, naming the tensor) for the others:
 *   <image block>.attn2.qkv.{weight,bias}     [3h, h] / [3h], q | k | v; the bias is FULL: attn2.k_proj keeps its bias (quirk Q9 is a
 *                                             property of the reference's `attn`; behind an RMSNorm a key bias is not a no-op)
 *   <image block>.attn2.o_proj.{weight,bias}  [h, h] / [h]
 *   <image block>.qk_norm2.{q,k}_norm.weight  [head_dim] (with use_qk_norm)
 * and adaLN.{weight,bias} holds 9 h rows for these image modules (dk_mmdit_mod_rows / dk_mmdit_mod_offset count them).
 * Verified against an fp32 / bf16-emulating oracle of this block form with synthetic weights (arithmetic parity); no SD3.5-medium
 * checkpoint has been run through it.
 *
 * dk_mmdit_set_dual_attention: legal until the weights are resolved (the first dk_mmdit_prepare).  0, the default, is the feature off:
 * the modulation table, dk_mmdit_workspace_bytes, the carve and every launch are then what they are without it; n_blocks > 0 adds XN2
 * [B S_x, h], QKV2 [B S_x, 3h] and ATT2 [B S_x, h] behind everything else in the workspace.  Refused, with no state changed and an
 * error that names the rule: n_blocks outside [0, depth_multimodal], a configuration with depth_unified > 0 or fp8_linears, an engine
 * whose weights are resolved. */
int dk_mmdit_set_dual_attention(dk_mmdit* m, int32_t n_blocks);

/* ---- Skip layers: a forked row group that sits out some double blocks (opt-in; skip-layer guidance, see dk_slg_cfg_step) ----------------
 * With B prepared batch rows, live = B - fork_rows and f = min(blocks), dk_mmdit_forward runs
 *   the embedders and the blocks g < f     on rows [0, live): rows >= live of tokens_in, of text and of the cached context are never read;
 *   the fork, in front of block f          X[live + j] = X[j] for j < fork_rows, text and image rows, one device copy in stream order;
 *   the blocks of the set                  on rows [0, live);
 *   every other block >= f, the final layer on all B rows;   tokens_out is [B, S_i, F].
 * "On rows [0, live)" is the launch sequence of a batch of `live` on the same buffers.  The modulation table is cached for B rows as
 * ever: the caller repeats the pooled rows of rows [0, fork_rows) for the fork rows.  So the fork rows are the evaluation of rows
 * [0, fork_rows) by a model that passes both streams unchanged through the blocks of the set, at the cost of the blocks they run.
 * May be called at any time after dk_mmdit_create and takes effect at the next forward; workspace size and carve do not change.
 * (NULL, 0, 0) is off, the default: every launch and every bit is then what it is without the feature.
 * Refused, with no state changed and an error that names the rule: exactly one of n_blocks and fork_rows zero (or either negative), a
 * block outside [0, depth_multimodal) or named twice, depth_unified > 0, fp8_linears, a reference grid or a condition width that is set.
 * Refused at the call, never launched: a forward with 2 * fork_rows > B, and dk_mmdit_forward_head, dk_mmdit_forward_tail and
 * dk_mmdit_run_blocks while skip layers are set.  Both element types.
 * Verified against an fp32 / emulating oracle with synthetic weights (arithmetic parity); no SD3.5-medium checkpoint has been run. */
int dk_mmdit_set_skip_layers(dk_mmdit* m, const int32_t* blocks, int32_t n_blocks, int32_t fork_rows);

/* ---- Perturbed attention: the forked row group with identity attention in some double blocks (opt-in; perturbed-attention guidance,
 * diffusers' StableDiffusion3PAGPipeline; the step entry is dk_slg_cfg_step, whose slg_scale is then the PAG scale) -------------------
 * The fork is dk_mmdit_set_skip_layers' (one function drives both).  With B prepared batch rows, live = B - fork_rows and f = min(blocks),
 * dk_mmdit_forward runs
 *   the embedders and the blocks g < f     on rows [0, live): rows >= live of tokens_in, of text and of the cached context are never read;
 *   the fork, in front of block f          X[live + j] = X[j] for j < fork_rows, one device copy in stream order;
 *   every block >= f, the final layer      on all B rows;   tokens_out is [B, S_i, F].
 * In a block of the set only the main attention differs: the plain launch runs on rows [0, live), and dk_attention_identity_* with
 * ident_from = S_t on rows [live, B) -- the same QKV / ATT buffers, base pointers advanced by `live` batch rows; one launch more per
 * perturbed block.  LN-modulate, the q/k/v projections, the key norm, the attn2 path of an MMDiT-X dual block (diffusers perturbs attn
 * only), both o-projections and the MLP stay one launch over B rows.  So the fork rows are the evaluation of rows [0, fork_rows) by a
 * model whose image queries, in the blocks of the set, attend to the text keys and to their own key.  The caller repeats the pooled rows
 * of rows [0, fork_rows) for the fork rows.  May be called at any time after dk_mmdit_create and takes effect at the next forward;
 * workspace size and carve do not change.  (NULL, 0, 0) is off, the default: every launch and every bit is then what it is without the
 * feature.
 * Refused, with no state changed and an error that names the rule: exactly one of n_blocks and fork_rows zero (or either negative), a
 * block outside [0, depth_multimodal) or named twice, depth_unified > 0, fp8_linears, a reference grid or a condition width that is
 * set, skip layers that are set (there is one fork; dk_mmdit_set_skip_layers likewise refuses while perturbed attention is set).
 * Refused at the call, never launched: a forward with 2 * fork_rows > B or a head_dim other than 64, and dk_mmdit_forward_head,
 * dk_mmdit_forward_tail and dk_mmdit_run_blocks while perturbed attention is set.  Both element types.
 * Verified against an fp32 / emulating oracle with synthetic weights (arithmetic parity); no checkpoint has been run. */
int dk_mmdit_set_perturbed_attention(dk_mmdit* m, const int32_t* blocks, int32_t n_blocks, int32_t fork_rows);

/* ---- SD3 ControlNet (opt-in; the layout of diffusers' SD3ControlNetModel, no counterpart in the reference) ---------------------------
 * Two engines.  The CONTROL-NET engine is an SD3 engine of N_c blocks without a final layer, with a second patch embedder for the
 * VAE-encoded control image and one Linear(h, h) per block; it writes N_c taps, [N_c, B, S_i, h] in the element type.  The MAIN engine
 * adds them to its image stream: with n taps and depth blocks, s * tap[floor(g * n / depth)] behind block g for g = 0 .. depth - 2 (diffusers'
 * rule, interval_control = depth / n and index int(g / interval_control), restated in integers; nothing behind the last block, whose text
 * stream is pre-only).  "Behind block g" is "in front of block g + 1": block g + 1's first LayerNorm launch becomes
 * dk_ln_modulate_add_* -- x' = round_E(fmaf(s, tap, x)), ONE rounding where the published code rounds s * tap and the sum -- and no
 * launch is added.
 * Verified against an fp32 / emulating oracle with synthetic weights (arithmetic parity); no ControlNet checkpoint has been run.
 *
 * dk_mmdit_set_control_net(m, on): legal before the first dk_mmdit_bind.  Refused unless the geometry is SD3's: use_pos_embed,
 * depth_unified == 0, no fp8_linears, no dual attention, no reference grid, no condition width.  Such an engine additionally binds
 *   pos_embed_input.proj.{weight,bias}   [h, p*p*C] / [h], packed as x_embedder.proj is
 *   controlnet_blocks.<j>.{weight,bias}  [h, h] / [h], j < depth_multimodal
 * and needs no final_layer.*; every other tensor is what an SD3 engine of that depth binds (the last block's text stream is pre-only as
 * ever: the published model runs its post-attention half, and nothing reads the result).
 * dk_mmdit_cache_control_image: after dk_mmdit_prepare.  ctrl_tokens in the element type, [batch, S_i, p*p*C] (per_image != 0) or
 * [1, S_i, p*p*C] (one control image for every batch row: one launch per batch row either way, the bits of a repeated image).  Computes
 * CONDE[b] = POS + pos_embed_input(ctrl_tokens[b]) once; every later dk_mmdit_control_forward's x_embedder launch takes CONDE in its
 * residual slot instead of POS.  Invalidated by dk_mmdit_prepare.
 * dk_mmdit_control_forward: the embedders, then blocks 0 .. N_c - 1, and behind block j one GEMM taps_out[j] = controlnet_blocks.<j>(
 * image rows) into the caller's taps_out [N_c, B, S_i, h].  dk_mmdit_forward, dk_mmdit_forward_head and dk_mmdit_forward_tail on a
 * control-net engine are refused with an error that names dk_mmdit_control_forward; dk_mmdit_run_blocks stays.
 *
 * dk_mmdit_set_control_taps(m, taps, n_taps, scale) on the MAIN engine: taps [n_taps, B, S_i, h] dense in the element type, 16-byte
 * aligned, owned by the caller and read by every later dk_mmdit_forward in stream order.  (NULL, 0, any) is off, the default: every launch
 * and every bit is then what it is without the feature.  Takes effect at the next forward; workspace size and carve do not change.
 * dk_mmdit_prepare switches the taps off (their shape was the previous problem's): set them again behind it.
 * Refused, with no state changed and an error that names the rule: a geometry other than SD3's (use_pos_embed, depth_unified == 0),
 * n_taps outside [1, depth_multimodal], fp8_linears, dual attention, a block cache, skip layers, perturbed attention, a reference grid or
 * a condition width that is set, a control-net engine.  dk_mmdit_forward_head, dk_mmdit_forward_tail and dk_mmdit_run_blocks are refused
 * while taps are set; dk_mmdit_set_block_cache(1), dk_mmdit_set_skip_layers and dk_mmdit_set_perturbed_attention likewise. */
int dk_mmdit_set_control_net(dk_mmdit* m, int32_t on);
int dk_mmdit_cache_control_image(dk_mmdit* m, const void* ctrl_tokens, int32_t per_image, void* stream);
int dk_mmdit_control_forward(dk_mmdit* m, const void* tokens_in, const void* text, int32_t step_index, void* taps_out, void* stream);
int dk_mmdit_set_control_taps(dk_mmdit* m, const void* taps, int32_t n_taps, float scale);

/* ---- FLUX ControlNet (opt-in; the layout of diffusers' FluxControlNetModel, no counterpart in the reference; bf16 only) --------------
 * The same two engines on FLUX geometry.  The entries above stay the SD3 family's and keep refusing FLUX geometry.
 *
 * dk_mmdit_set_flux_control_net(m, on): legal before the first dk_mmdit_bind.  Needs use_rope, no positional table, bf16, no fp8_linears,
 * depth_multimodal >= 1; depth_unified >= 0.  Such an engine has no final layer (and no modulation rows for one) and additionally binds
 *   controlnet_x_embedder.proj.{weight,bias}       [h, p*p*C] / [h], packed as x_embedder.proj is
 *   controlnet_blocks.<j>.{weight,bias}            [h, h] / [h], j < depth_multimodal
 *   controlnet_single_blocks.<j>.{weight,bias}     [h, h] / [h], j < depth_unified
 * dk_mmdit_cache_control_image on it computes CONDE[b] = controlnet_x_embedder(ctrl_tokens[b]) once (FLUX has no positional table, so
 * the slot is free); every dk_mmdit_control_forward's x_embedder launch adds it in its residual epilogue:
 *   image rows = round( round(x_embedder(tokens)) + round(controlnet_x_embedder(control tokens)) ).
 * dk_mmdit_control_forward writes depth_multimodal + depth_unified taps, [n, B, S_i, h], double blocks first: behind each double block
 * the tap Linear reads the image stream, behind each single block the image rows of the joint stream.
 *
 * dk_mmdit_set_flux_control_taps(m, taps, n_double_taps, n_single_taps, scale) on the MAIN engine: taps [n_double_taps + n_single_taps,
 * B, S_i, h] dense bf16, 16-byte aligned, the double blocks' taps first; either count may be 0, each is at most the model's depth of
 * that kind.  Behind block g of a kind with depth blocks and n taps the image rows take s * tap[g / ceil(depth / n)] (diffusers'
 * FluxTransformer2DModel: index_block // int(np.ceil(depth / n)); NOT the SD3 rule -- depth 4, n 3 gives 0,0,1,1 here and 0,0,1,2
 * there), the last block of each kind included.  Every add rides in the LayerNorm launch that reads those rows next, as
 * x' = round_bf16(fmaf(s, tap, x)) in place:
 *   behind double g < depth_multimodal - 1     block g + 1's first LayerNorm (dk_ln_modulate_add_bf16)
 *   behind the last double block               single block 0's LayerNorm, on the image rows of the joint stream
 *                                              (dk_ln_modulate_add_joint_bf16); the final layer's with depth_unified == 0
 *   behind single j < depth_unified - 1        single block j + 1's LayerNorm, likewise
 *   behind the last single block               the final layer's LayerNorm
 * so a tapped evaluation has the launch count of a plain one.  (NULL, 0, 0, any) is off, the default: every launch and every bit is then
 * what it is without the feature.  dk_mmdit_prepare switches the taps off.
 * Refused, with no state changed and an error that names the rule: a geometry other than FLUX's, fp8_linears (the MX-fp8 LayerNorm
 * kernels take no tap), fp16, a count outside its range, dual attention, a block cache, skip layers, perturbed attention, a reference
 * grid, a condition width, a control-net engine.  dk_mmdit_forward_head, dk_mmdit_forward_tail and dk_mmdit_run_blocks are refused while
 * taps are set.  Verified against an fp32 / emulating oracle with synthetic weights (arithmetic parity); no checkpoint has been run. */
int dk_mmdit_set_flux_control_net(dk_mmdit* m, int32_t on);
int dk_mmdit_set_flux_control_taps(dk_mmdit* m, const void* taps, int32_t n_double_taps, int32_t n_single_taps, float scale);

/* ---- FLUX IP-Adapter (opt-in; XLabs-AI flux-ip-adapter as diffusers' FluxIPAdapterJointAttnProcessor2_0 runs it, no counterpart in the
 * reference; bf16 only) -------------------------------------------------------------------------------------------------------------
 * Decoupled image-prompt attention in the double blocks: behind double block i, after fc2's gated add,
 *   x_img <- x_img + scale * softmax( q_n K_i^T / sqrt(D) ) V_i          per head, no projection, no gate
 * with q_n the block's image queries after QK-RMSNorm and BEFORE RoPE, and K_i / V_i = to_k_ip_i / to_v_ip_i of the n_tokens image-prompt
 * tokens of that batch row ([n_tokens, token_dim]: the adapter's projection of the CLIP image embedding, computed by the caller).  Single
 * blocks take nothing.
 *
 * dk_mmdit_set_ip_adapter(m, n_tokens, token_dim): legal before the weights are resolved (the first dk_mmdit_prepare); (0, 0) is off, the
 * default: workspace size, carve, every launch and every bit are then what they are without the feature.  1 <= n_tokens <= 16, token_dim a
 * multiple of 64.  The engine additionally binds, for i < depth_multimodal,
 *   ip_adapter.<i>.to_k_ip.{weight,bias}, ip_adapter.<i>.to_v_ip.{weight,bias}      [h, token_dim] / [h]
 * which must be views of ONE matrix [depth_multimodal * 2h, token_dim] (block i's to_k_ip rows at i * 2h, its to_v_ip rows h further) and
 * ONE bias laid out the same way (weights.py: pack_ip_adapter; a checkpoint without biases binds zeros).  The workspace grows by the K / V
 * cache [batch * n_tokens, depth_multimodal * 2h] and one output buffer [batch * S_i, h].
 * dk_mmdit_cache_ip_tokens(m, tokens, per_image, stream): after dk_mmdit_prepare.  tokens bf16 [batch, n_tokens, token_dim] (per_image != 0)
 * or [1, n_tokens, token_dim] (one prompt for every batch row: one GEMM launch over the stacked matrix per batch row either way, the bits of
 * a repeated prompt).  Replaces a previous cache; invalidated by dk_mmdit_prepare.
 * dk_mmdit_set_ip_scale(m, scale): 0 (the default) is off -- the plain launches and their bits.  With another scale every dk_mmdit_forward
 * runs, behind the q / k / v projection of double block i, ONE more launch (dk_ip_attention_bf16 on the raw image queries that QKV still
 * holds: the attention kernel norms and rotates in its own Q load) into the output buffer, and the add rides as x' = round_bf16(fmaf(scale,
 * ip, x)) in the LayerNorm launch that reads the image rows next -- block i + 1's first (dk_ln_modulate_add_bf16), single block 0's or, with
 * depth_unified == 0, the final layer's (dk_ln_modulate_add_joint_bf16).
 * Refused, with no state changed and an error that names the rule: SD3 geometry, fp8_linears (the MX-fp8 LayerNorm kernels take no tap),
 * fp16, a head size other than 128, a control-net engine, control taps (one tap operand per LayerNorm launch), a block cache, a reference
 * grid, a condition width, skip layers, perturbed attention, dual attention; those setters refuse an engine with an adapter in turn.
 * dk_mmdit_forward with the adapter active is refused without a cache and under dk_tune_set("attn_fuse_q", 0) or ("gemm_fuse_q", 1), which
 * leave no raw queries in QKV ("gemm_fuse_q" 1 only while the keys' fused tail is on: with "gemm_fuse_k" 0 it finishes nothing and is accepted);
 * dk_mmdit_forward_head, dk_mmdit_forward_tail and dk_mmdit_run_blocks are refused while it is active, the first two in front of their own
 * block-cache rule, so that the adapter's text is what they answer.
 * Written from the published definition and verified against an fp32 / emulating oracle with synthetic weights (arithmetic parity); no
 * checkpoint has been run. */
int dk_mmdit_set_ip_adapter(dk_mmdit* m, int32_t n_tokens, int32_t token_dim);
int dk_mmdit_cache_ip_tokens(dk_mmdit* m, const void* tokens, int32_t per_image, void* stream);
int dk_mmdit_set_ip_scale(dk_mmdit* m, float scale);
/* The kernel behind it, stand-alone.  qkv: bf16 [B, seg_stride, ldq] whose rows hold the raw q projection in their first h columns; the rows
 * read are first_row .. first_row + seg_len - 1 of every batch row and of those the first h columns -- the other rows (text) and columns (k,
 * v) are never addressed.  qn: [D] QK-norm weight.  k, v: [B, N, h] at ldkv elements per row.  out: dense [B * seg_len, h]:
 *   q_n = round_bf16(q * rsqrt(mean_D(q^2) + eps) * qn);  out[b, s, head] = round_bf16( softmax_n(scale * q_n . k[b, n, head]) @ v[b, :, head] )
 * with the scores, the exact (max-subtracted) softmax and the weighted sum in fp32.  D == 128 and 1 <= N <= 16, anything else is refused by
 * name; h % 128 == 0; pitches % 8 == 0; 16-byte aligned pointers. */
int dk_ip_attention_bf16(const void* qkv, int32_t ldq, int32_t seg_len, int32_t seg_stride, int32_t first_row, const void* qn, const void* k,
                         const void* v, int32_t ldkv, int32_t B, int32_t N, int32_t h, int32_t D, float scale, float eps, void* out, void* stream);
/* Head of step `step_index`: dk_mmdit_forward's embedder launches, block 0 and the probe.  probe_out: device float [batch][2] =
 * (num, den) per batch row; before any computed step den is 0 (and num = sum |D_cur|).  Records a pending head for step_index. */
int dk_mmdit_forward_head(dk_mmdit* m, const void* tokens_in, const void* text, int32_t step_index, float* probe_out, void* stream);
/* Tail of the pending head, which must be of the same step_index; reuse = 1 additionally needs a valid cache (a computed step since
 * the last reset).  Either violation is an error that names the rule, never a launch. */
int dk_mmdit_forward_tail(dk_mmdit* m, int32_t step_index, int32_t reuse, void* tokens_out, void* stream);
/* The two kernels behind it, stand-alone.  x: first image row of a joint stream; logical row m of M is physical row
 * (m / x_seg_len) * x_seg_stride + m % x_seg_len at ldx elements per row (the engine: x = X + S_t * h, x_seg_len = S_i, x_seg_stride = S).
 * h % 8 == 0, h <= 4096; ldx % 8 == 0; 16-byte aligned pointers.
 * dk_block_probe_*: d [M, h] dense holds X0's rows on entry and D_cur = round_E(x - d) on return; d_ref [M, h] dense or NULL (read as
 * zeros: den = 0); row_partials: float [M][2] scratch, (num, den) per row; probe: float [M / rows_per_batch][2].
 * dk_block_residual_*: reuse == 0: r [M, h] dense holds X1's rows on entry and R = round_E(x - r) on return (x is read only);
 * reuse != 0: x = round_E(x + r) (r is read only). */
int dk_block_probe_bf16(const void* x, int32_t ldx, int32_t x_seg_len, int32_t x_seg_stride, void* d, const void* d_ref,
                        float* row_partials, float* probe, int32_t M, int32_t h, int32_t rows_per_batch, void* stream);
int dk_block_probe_f16(const void* x, int32_t ldx, int32_t x_seg_len, int32_t x_seg_stride, void* d, const void* d_ref,
                       float* row_partials, float* probe, int32_t M, int32_t h, int32_t rows_per_batch, void* stream);
int dk_block_residual_bf16(void* x, int32_t ldx, int32_t x_seg_len, int32_t x_seg_stride, void* r, int32_t M, int32_t h, int32_t reuse,
                           void* stream);
int dk_block_residual_f16(void* x, int32_t ldx, int32_t x_seg_len, int32_t x_seg_stride, void* r, int32_t M, int32_t h, int32_t reuse,
                          void* stream);

typedef struct dk_vae_config {
  int32_t in_channels, out_channels, block_out_channels[4], n_blocks, layers_per_block, resnet_groups;
  float group_norm_eps;
} dk_vae_config;
typedef struct dk_vae dk_vae;
int dk_vae_create(const dk_vae_config* cfg, dk_vae** out);
void dk_vae_destroy(dk_vae* v);
/* names = reference module tree (vae.py / model_io.py:411-486), conv weights flattened to
 * [O, 9*I]; conv_in.weight zero-padded to I = 64 */
int dk_vae_bind(dk_vae* v, const char* name, const void* dev_ptr);
/* Element type of the handle (decoder or encoder): 0 = bfloat16 (the default) or 1 = float16; anything else is refused.  Call it
 * before the first dk_vae_bind: every bound tensor is then of that type, and so are the activations, `raw_bf16` of dk_vae_decode and
 * `moments_bf16` of dk_vae_encode (the f32 outputs stay f32).  A later call -- after a bind, or after an earlier dk_vae_set_dtype -- is
 * refused unless it names the type already set.  fp16 is the reference's decoder dtype for Stable Diffusion 3 (mlx/__init__.py:108-113); its
 * encoder runs in fp32 (:116), so the fp16 encoder is the closer of the two 16-bit forms, not the reference's dtype. */
int dk_vae_set_dtype(dk_vae* v, int32_t dtype);
size_t dk_vae_workspace_bytes(const dk_vae* v, int32_t batch, int32_t latent_h, int32_t latent_w);
/* VAEDecoder.__call__ (vae.py:386-401) + decode_latents_to_image (__init__.py:581-584) +
 * uint8 conversion (__init__.py:525-526).  latent: f32 [B,h,w,16];
 * image_f32: [B,8h,8w,3] in [0,1] or NULL; image_u8: [B,8h,8w,3] or NULL;
 * raw_bf16: decoder output before the clip, [B,8h,8w,4] (3 used, the fourth column is written as zero on every route) or NULL. */
int dk_vae_decode(dk_vae* v, const float* latent, int32_t batch, int32_t latent_h, int32_t latent_w,
                  float* image_f32, uint8_t* image_u8, void* raw_bf16, void* workspace,
                  size_t workspace_bytes, void* stream);

/* VAEEncoder.__call__ (vae.py:456-467) on a dk_vae created with the encoder's configuration and
 * bound to its module names (conv_in, down_blocks.{i}.resnets.{r}, down_blocks.{i}.downsample,
 * mid_blocks.{0,1,2}, conv_norm_out, conv_out).  image: f32 [B,H,W,in_channels] in [-1,1]
 * (read_image, __init__.py:536-551); moments (mean | logvar, __init__.py:588-589):
 * bf16 [B,H/8,W/8,ldm] (ldm multiple of 4, >= out_channels) and / or f32 [B,H/8,W/8,out_channels]. */
size_t dk_vae_encoder_workspace_bytes(const dk_vae* v, int32_t batch, int32_t image_h, int32_t image_w);
int dk_vae_encode(dk_vae* v, const float* image, int32_t batch, int32_t image_h, int32_t image_w,
                  void* moments_bf16, int32_t ldm, float* moments_f32, void* workspace,
                  size_t workspace_bytes, void* stream);
/* encode_image_to_latents tail (__init__.py:589-594):
 * latent = mean + exp(0.5 * clip(logvar, -30, 20)) * noise, f32 [n_pixels, latent_channels] */
int dk_latent_sample_f32(const void* moments_bf16, int32_t ldm, const float* noise, float* latent,
                         int64_t n_pixels, int32_t latent_channels, void* stream);
int dk_latent_sample_f16(const void* moments_f16, int32_t ldm, const float* noise, float* latent,
                         int64_t n_pixels, int32_t latent_channels, void* stream);  /* the same on fp16 moments (an fp16 encoder's) */

/* ------------------------------------------------------------------------------------------
 * Measurement hooks (no reference counterpart; the reference times phases with time.time(),
 * mlx/__init__.py:315-530).  When enabled, every bf16 GEMM (class 0), conv (1), attention (2) and fp8 GEMM (3) launch
 * is bracketed by HIP events on its launch stream; dk_profile_read sums elapsed time, algorithmic
 * FLOPs and launch count of one class since the last dk_profile_enable call.
 * ---------------------------------------------------------------------------------------- */
int dk_profile_enable(int32_t on);
int dk_profile_read(int32_t kernel_class, double* total_ms, double* total_flops, int64_t* launches);

/* Tuning knobs for A/B measurements (no reference counterpart); -1 = automatic (the shipped default) for every key.
 * "gemm": 128 = 128x128 tiles only, 9 = the 8-wave 256x256 kernel on every shape it accepts, 10 = the one-wave-per-SIMD 256x256 kernel
 * (asm body) on every shape IT accepts; "gemm_v4": 0 = the automatic choice never takes the latter; "gemm_skew": start skew of that kernel's
 * multi-round launches in 0.25 us steps (-1: none); "gemm_mf": 8 / 7 = 256- / 224-row
 * tiles; "gemm_split": 0 / 1 = remainder-wave K split never / whenever possible; "gemm_split_min": K-tile steps a workgroup must save before a
 * Linear of at most half a round of tiles is cut along K as a whole (default 32); "gemm_pair_nk": K-tile steps from which an image + text pair with
 * a small extra round is grouped and cut (default 24); "gemm_fuse_k" / "gemm_fuse_q": 0 / 1 = the keys' /
 * queries' QKNorm + RoPE in the q/k/v projection's tail off / on; "attn": kernel of dk_attention_bf16 (4 lean kernel,
 * 9 phase-alternating kernel: head_dim 128 only, falls back to 4 otherwise; 10 one-wave-per-SIMD kernel with the generated asm
 * tile loop: head_dim 128, S a multiple of 256 and >= 768, falls back to 9 otherwise -- the automatic choice from S = 2048 on, and from
 * S = 1024 for launches of at least three quarters of a round of 256-query blocks);
 * "attn_split": key ranges of the one-wave-per-SIMD kernel's last-round query blocks (-1 automatic, 0 never, 2..4);
 * "attn_track": 1 = that kernel keeps its running row maximum whatever score_bound a launch carries (-1 / 0 automatic);
 * "attn_fuse_q": 0 = stand-alone query QKNorm + RoPE pass; "conv_halo": 0 = VAE convolutions through the GEMM form;
 * "conv_v4": the fused VAE convolutions with >= 256 output channels on the one-wave-per-SIMD kernel (1 where one image fills the
 * CUs, 0 never, 2 wherever eligible);
 * "pitch_min_k": rows of at least this many elements are stored padded (dk_weight_pitch).
 * Returns 0, or -1 for an unknown key. */
int dk_tune_set(const char* key, int32_t value);

/* Row pitch, in elements, the engine expects for a weight matrix whose rows hold k elements and that it reads with a long
 * reduction: k itself below 8192, k + 64 from there on (the 24-30 KB row stride of the [h, 4h] "mlp.fc2.weight" of the
 * double-stream blocks and the [h, 5h] "linear2.weight" of the single-stream blocks of FLUX camps on a few memory channels;
 * the pad columns are never read).  The host packer (diffusionkit_amd/weights.py: pack_mmdit) lays those two tensors out
 * with this pitch before dk_mmdit_bind; every other tensor is dense.  No reference counterpart (mlx arrays are dense). */
int32_t dk_weight_pitch(int32_t k);

#ifdef __cplusplus
}
#endif
#endif /* DK_HIP_H */
