// The statements of the coefficient-row step (elementwise.hip: dk_lms_step_kernel and dk_lms_noisy_step_kernel include this file as their body, once
// per element type).  It reads the kernels' arguments by name, the template parameters MASKED, GMODE and SLG, and a constant NOISY; under NOISY
// also the NoiseArgs nz.  Included text, not a function: called through an inlined function, the masked instantiations of dk_lms_step_kernel come out
// of the compiler with two scalar registers swapped, and their instructions are held byte for byte (scripts/device_code_diff.py).
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per_img = (long)Hl * Wl * C;
  if (i >= per_img * n_img) return;
  const StepCell k = step_cell((int)(i / per_img), i % per_img, Hl, Wl, C, p, reshape_order);
  const float xv = x[i];
  const float xb = round_act(xv);  // the value the denoiser saw
  float den = step_den(model_out, ld_out, k.img, k.S_i, k.t, k.f, xb, sigma);
  float slg = 0.0f;
  if constexpr (SLG) {  // (cfg_on != 0: check_step)
    slg = gd.slg_scale * (den - step_den(model_out, ld_out, 2 * n_img + k.img, k.S_i, k.t, k.f, xb, sigma));
  }
  if constexpr (GMODE == DK_GUIDE_CFG) {
    if (cfg_on) {
      const float den_neg = step_den(model_out, ld_out, n_img + k.img, k.S_i, k.t, k.f, xb, sigma);
      den = den_neg + cfg_weight * (den - den_neg);
    }
  } else {  // (cfg_on != 0: check_step)
    const float den_neg = step_den(model_out, ld_out, n_img + k.img, k.S_i, k.t, k.f, xb, sigma);
    if constexpr (GMODE == DK_GUIDE_RESCALE) {
      const float g = den_neg + cfg_weight * (den - den_neg);
      den = g * gd.scal[2 * k.img];
    } else {
      float dl = den - den_neg;
      if (gd.reads_m) dl = dl + gd.beta * gd.m[i];
      if (gd.writes_m) gd.m[i] = dl;
      const float a = gd.scal[2 * k.img], b = gd.scal[2 * k.img + 1];
      den = den + (cfg_weight - 1.0f) * (a * dl - b * den);
    }
  }
  float num = xv - den;
  if constexpr (SLG) {
    num = num - slg;  // x - (den + slg), taken behind the difference: a product that forms den may be contracted into it, and with slg_scale == 0 the
                      // exact zero then leaves the bits of the mode's own step
  }
  const float d = num / sigma;
  float xn;
  if (row.reads_h)
    xn = row.cx * xv + row.cd * d + row.ch * hist[i];
  else if (row.cx == 1.0f)
    xn = xv + d * row.cd;
  else
    xn = row.cx * xv + d * row.cd;
  if (row.writes_h) hist[i] = row.hx * xv + row.hd * d;
  if constexpr (NOISY) {
    const long r = i % per_img;
    xn = xn + nz.cn * philox_normal(nz.seeds[k.img], (unsigned long long)(r >> 2), nz.draw, 0u, (int)(r & 3));
  }
  if constexpr (MASKED) {
    xn = step_blend(xn, i, k.img, k.yy, k.xx, Hl, Wl, sigma_next, x_orig, noise, mask, mask_per_image);
  }
  step_store(x, tok, i, xn, k, n_img, cfg_on);
