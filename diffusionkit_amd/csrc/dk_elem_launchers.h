// Launchers that exist once per element type (dk_common.h, element-type layer): dk_kernels.h includes this file at global scope (bf16) and
// again inside namespace dk_f16 (fp16) -- same signatures, 16-bit storage either way (bf16_t = the raw halfword).  No include guard.
// The global gemm / attention launchers forward to their dk_f16 twin on GemmParams::dtype / AttnParams::dtype; the elementwise ones are
// picked by the caller.
int dk_launch_gemm128(const GemmParams& p, const GemmRoute& r, hipStream_t stream);  // gemm.hip: 128 x 128 tiles
int dk_launch_gemm256v3(const GemmParams& p, const GemmParams* p2, const GemmRoute& r, hipStream_t stream);  // (16x16x32 MFMA K loop)
int dk_launch_attention2(const AttnParams& p, int waves, hipStream_t stream);  // attention2.hip (VALU-lean variant)
// out[m, :] = bf16( LN(x[m, :]) * bf16(1 + scale[b, :]) + shift[b, :] ), b = m / seg_len
int dk_launch_ln_modulate(const bf16_t* x, int ldx, bf16_t* out, int ldo, int M, int h,
                          const bf16_t* shift, const bf16_t* scale, int mod_stride, int seg_len,
                          int x_seg_len, int x_seg_stride, float eps, hipStream_t stream);
// in-place per-head RMSNorm (learned weight) + RoPE on the q and k column groups of a QKV buffer
int dk_launch_qk_norm_rope(bf16_t* qkv, int ld, int q_off, int k_off, int rows, int H, int D,
                           const bf16_t* qw, const bf16_t* kw, float eps, const float* rope,
                           int row_seg_len, int row_seg_stride, int pos_off, int S_pos,
                           hipStream_t stream, int k_only = 0);
// two row sets (image / text stream of a double block) per launch
int dk_launch_ln_modulate2(const bf16_t* x0, bf16_t* out0, int M0, const bf16_t* shift0, const bf16_t* scale0, int seg0, const bf16_t* x1,
                           bf16_t* out1, int M1, const bf16_t* shift1, const bf16_t* scale1, int seg1, int ldx, int ldo, int h,
                           int mod_stride, int x_seg_stride, float eps, hipStream_t stream);
// ... the first of which leaves twice, under two modulations (MMDiT-X: the image stream of a dual-attention block); M1 == 0: one row set
int dk_launch_ln_modulate2x(const bf16_t* x0, bf16_t* out0, bf16_t* out0b, int M0, const bf16_t* shift0, const bf16_t* scale0,
                            const bf16_t* shift0b, const bf16_t* scale0b, int seg0, const bf16_t* x1, bf16_t* out1, int M1,
                            const bf16_t* shift1, const bf16_t* scale1, int seg1, int ldx, int ldo, int h, int mod_stride, int x_seg_stride,
                            int x_seg_stride1, float eps, hipStream_t stream);
// ... or takes a residual first (ControlNet taps): x0 <- round(fmaf(s, tap, x0)) in place (tap: dense [M0, ldt]), out0 from the new rows
int dk_launch_ln_modulate2_add(bf16_t* x0, const bf16_t* tap, int ldt, float s, bf16_t* out0, int M0, const bf16_t* shift0, const bf16_t* scale0,
                               int seg0, const bf16_t* x1, bf16_t* out1, int M1, const bf16_t* shift1, const bf16_t* scale1, int seg1, int ldx,
                               int ldo, int h, int mod_stride, int x_seg_stride, int x_seg_stride1, float eps, hipStream_t stream);
int dk_launch_qk_norm_rope2(bf16_t* qkv0, int rows0, const bf16_t* qw0, const bf16_t* kw0, int seg0, int pos0, bf16_t* qkv1, int rows1,
                            const bf16_t* qw1, const bf16_t* kw1, int seg1, int pos1, int ld, int q_off, int k_off, int H, int D,
                            float eps, const float* rope, int row_seg_stride, hipStream_t stream, int k_only = 0);
int dk_launch_silu(const bf16_t* x, bf16_t* y, long n, hipStream_t stream);
int dk_launch_add(const bf16_t* a, const bf16_t* b, int b_rows, bf16_t* y, int rows, int cols, hipStream_t stream);
int dk_launch_timestep_embedding(const float* t, int n, int rep, int dim, float max_period, int embed_dtype,
                                 bf16_t* out, hipStream_t stream);
// latent [n_img, Hl, Wl, C] fp32 -> tokens [B, S_i, p*p*C] bf16 (B = n_img * dup)
int dk_launch_latent_to_tokens(const float* x, bf16_t* tok, int n_img, int dup, int Hl, int Wl, int C, int p,
                               int reshape_order, hipStream_t stream);
// The step-loop tail: x0 prediction + CFG + update of x (+ re-patchify for the next step), one launch -- behind two small ones under a guidance
// mode.  All zeros but the operands = the plain Euler step with the CFG combine.  (One struct for both element types: the second inclusion
// finds it at global scope.)
#ifndef DK_STEP_PARAMS
#define DK_STEP_PARAMS
struct StepParams {
  // operands: x f32 [n_img, Hl, Wl, C], the model's output and the tokens of the next step in the element type
  float* x;
  const bf16_t* model_out;
  int ld_out;
  bf16_t* tok;
  int n_img, cfg_on, Hl, Wl, C, p, reshape_order;
  float sigma, sigma_next, cfg_weight;
  // update.  has_row false: x' = x + d (sigma_next - sigma), dk_euler_step_kernel.  True: dk_lms_step_kernel with d = (x - den) / sigma,
  // x' = cx x + cd d + ch hist (hist, fp32 like x, read only under reads_h), hist' = hx x + hd d (written only under writes_h)
  bool has_row;
  float cx, cd, ch, hx, hd;
  float* hist;
  bool reads_h, writes_h;
  // blend (masked; the entry says whether it promises one): x = m x' + (1 - m)(sigma_next noise + (1 - sigma_next) x_orig); x_orig, noise: f32
  // like x, mask: f32 [n_img or 1, Hl, Wl]
  bool masked;
  const float *x_orig, *noise, *mask;
  bool mask_per_image;
  // guidance (include/dk_hip.h; guided: a dk_guided_* call, whose mode and parameters are checked and which needs cfg_on).  Mode 0 is the
  // launch above.  Modes 1 / 2: the per-image moments of the two predictions in front (partial sums per workgroup, then one wave per image folds
  // them in fp64 into the scalars), then the row step with den = g * s (1, rescale) or c + (w - 1)(a D - b c) (2, APG; m: the fp32 momentum
  // buffer, read under reads_m, written under writes_m).  workspace: at least dk_guidance_workspace_size bytes, 8-byte aligned.
  bool guided;
  int mode;
  float phi, eta, r, beta;
  float* m;
  bool reads_m, writes_m;
  void* workspace;
  size_t workspace_bytes;
  // skip-layer guidance (slg: a dk_slg_* call, which needs cfg_on): model_out holds a third row group [2 n_img, 3 n_img), and den takes
  // slg_scale (c - k) with k its x0 prediction; the tokens keep their two copies
  bool slg;
  float slg_scale;
  // stochastic samplers (noisy: a dk_noisy_* call, whose latent must hold a multiple of 4 elements per image): x' takes cn xi behind the update and
  // in front of the blend, xi the standard normals of draw `draw` of seeds[img] (u64 [n_img] on the device; read only where cn != 0), formed in the
  // launch.  cn == 0: the launches above, bit for bit
  bool noisy;
  float cn;
  const unsigned long long* seeds;
  int draw;
};
#endif
size_t dk_guidance_workspace_size(int n_img, int Hl, int Wl, int C);
int dk_launch_step(const StepParams& s, hipStream_t stream);
// FlowEdit (include/dk_hip.h: dk_flowedit_step): z' = z + c (V_tar - V_src) from the rows [src | tar] or [src+ | tar+ | src- | tar-] of model_out
// (n_img each; prime: not read, z stays), then Zs = (1 - sigma_in) x_src + sigma_in xi and Zt = Zs + (z' - x_src) with xi drawn in the launch
// (seeds[img], draw, stream tag 1), written in fp32 (zs_out may be null) and as the tokens of the same rows.  One struct for both element types.
#ifndef DK_FLOWEDIT_PARAMS
#define DK_FLOWEDIT_PARAMS
struct FlowEditParams {
  float* z;
  const float* x_src;
  const bf16_t* model_out;
  int ld_out;
  bf16_t* tok;
  float *zs_out, *zt_out;
  int n_img, cfg_on, Hl, Wl, C, p, reshape_order;
  float w_src, w_tar, c, sigma_in;
  const unsigned long long* seeds;
  int draw, prime;
};
#endif
int dk_launch_flowedit_step(const FlowEditParams& s, hipStream_t stream);
// first-block cache (include/dk_hip.h): d = round(x - d) over M rows of x through the row map, (num, den) = (sum |d - d_ref|, sum |d_ref|) per
// row into row_partials [M][2], then per rows_per_batch rows in a fixed order into probe [M / rows_per_batch][2]; d_ref null: read as zeros
int dk_launch_block_probe(const bf16_t* x, int ldx, int x_seg_len, int x_seg_stride, bf16_t* d, const bf16_t* d_ref, float* row_partials,
                          float* probe, int M, int h, int rows_per_batch, hipStream_t stream);
// reuse false: r = round(x - r); true: x = round(x + r)
int dk_launch_block_residual(bf16_t* x, int ldx, int x_seg_len, int x_seg_stride, bf16_t* r, int M, int h, bool reuse, hipStream_t stream);
