// VAE launchers that exist once per element type (dk_common.h, element-type layer): dk_kernels.h includes this file at global scope (bf16)
// and again inside namespace dk_f16 (fp16) -- same signatures, 16-bit storage either way (bf16_t = the raw halfword).  No include guard.
int dk_launch_conv_halo(const ConvHaloParams& p, hipStream_t stream);      // conv_halo.hip
int dk_launch_attention512(const Attn512Params& p, hipStream_t stream);    // attention512.hip
// ---- vae_ops.hip ----
// the second pass of the GroupNorm statistics alone: per (batch, group) the partials [B][nchunk][G][2] = (sum, M2 about the chunk's own mean)
// of the chunks of HW pixels (statistics pass: ceil(HW / nchunk) pixels each; conv tiles: 256) -> mean / rstd, and
// (gamma given) the per-channel table scale_shift [B][2][C]: scale = rstd * gamma, shift = beta - mean * scale
int dk_launch_groupnorm_finalize(const float* partial, int nchunk, int B, int G, long HW, float eps, float* mean_rstd,
                                 const bf16_t* gamma, const bf16_t* beta, int C, float* scale_shift, hipStream_t stream);
int dk_launch_groupnorm_partials(const bf16_t* x, int B, long HW, int C, int G, float* partial, int nchunk, hipStream_t stream);
int dk_launch_groupnorm_stats(const bf16_t* x, int B, long HW, int C, int G, float* partial, int nchunk,
                              float* mean_rstd, float eps, hipStream_t stream);
int dk_launch_groupnorm_apply(const bf16_t* x, bf16_t* y, int B, long HW, int C, int G, const float* mean_rstd,
                              const bf16_t* gamma, const bf16_t* beta, int do_silu, hipStream_t stream);
int dk_launch_softmax_rows(bf16_t* x, int rows, int cols, int ld, hipStream_t stream);
int dk_launch_transpose(const bf16_t* x, bf16_t* y, int R, int Cc, hipStream_t stream, int ldy = 0);  // ldy > R: zero-padded rows
int dk_launch_pad_channels(const float* x, bf16_t* y, long npix, int C, int Cpad, hipStream_t stream);
int dk_launch_image_post(const bf16_t* x, int ldx, float* img, unsigned char* u8, long npix, hipStream_t stream);
int dk_launch_latent_sample(const bf16_t* mom, int ldm, const float* noise, float* out, long npix, int L, hipStream_t stream);
int dk_launch_bf16_rows_to_f32(const bf16_t* x, int ldx, float* y, long npix, int C, hipStream_t stream);
