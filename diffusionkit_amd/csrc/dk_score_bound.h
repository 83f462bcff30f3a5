// The bound on |scale * q.k| that QK-normed attention operands carry (AttnParams::score_bound), from the norm weights alone.  Host code only, no
// HIP: mmdit_engine.hip uses it at resolve time / per launch, scripts/score_bound_check.cpp runs it under the host sanitizers.
//
// RMSNorm (mmdit.py:754-764) leaves q^ = x * rsqrt(mean(x^2) + eps) * w_q: sum_i (q^_i / w_q,i)^2 = D * ms / (ms + eps) <= D, so
// ||q^||_2 <= max|w_q| * sqrt(D); the same for k^ with w_k.  RoPE rotates pairs of coordinates and changes no norm.  Cauchy-Schwarz:
//   |scale * q^.k^| <= scale * max|w_q| * max|w_k| * D        (= max|w_q| * max|w_k| * sqrt(D) at scale = 1 / sqrt(D)).
// The kernels round q^ and k^ to bf16 element by element, twice where RoPE follows (relative 2^-9 each): below 0.8 % on the product; the
// factor 1.02 covers it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

// max |w| over n bf16 values given as their bit patterns; +inf when a value is not finite (the bound is then useless, and says so)
inline float dk_bf16_absmax(const uint16_t* w, size_t n) {
  float mx = 0.f;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t bits = (uint32_t)(w[i] & 0x7fffu) << 16;
    float f;
    memcpy(&f, &bits, 4);
    if (!(f <= 3.0e38f)) return INFINITY;  // inf or NaN
    mx = f > mx ? f : mx;
  }
  return mx;
}

// q_max / k_max: max|w| of the query / key norm weights of every stream whose rows are in the launch (0: a stream without weights -> 0, unknown)
inline float dk_score_bound(float q_max, float k_max, int D, float scale) {
  if (!(q_max > 0.f) || !(k_max > 0.f) || D <= 0 || !(scale > 0.f)) return 0.f;
  const float b = q_max * k_max * (float)D * scale * 1.02f;
  return b <= 3.0e38f ? b : 0.f;  // (a bound that overflowed is no bound)
}

// per block: the maxima of its D-element norm vectors, laid out one after the other in `host` (n_vec vectors) -> out[v]
inline void dk_norm_weight_maxima(const uint16_t* host, size_t n_vec, int D, float* out) {
  for (size_t v = 0; v < n_vec; ++v) out[v] = dk_bf16_absmax(host + v * (size_t)D, (size_t)D);
}
