// Stand-alone check of diffusionkit_amd/csrc/dk_score_bound.h (the host code behind AttnParams::score_bound), meant to be built with the host
// sanitizers and run directly:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined scripts/score_bound_check.cpp -o score_bound_check && ./score_bound_check
// Covers the per-block maxima over exact-size heap buffers (a read past a vector's D values is an AddressSanitizer report), the formula against
// fp64, the brute-force meaning of the bound (no QK-normed, rotated pair exceeds it), and the cases that must answer "unknown".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../diffusionkit_amd/csrc/dk_score_bound.h"

static int g_bad = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++g_bad; } \
  } while (0)

static uint16_t to_bf16(float f) {  // round to nearest even
  uint32_t u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static float from_bf16(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

int main() {
  std::mt19937 rng(7);
  std::normal_distribution<float> gain(1.0f, 0.02f), unit(0.0f, 1.0f);
  // ---- maxima: n_vec vectors of D values in one exact-size allocation; negative values count by magnitude
  for (int D : {64, 128}) {
    const size_t n_vec = 2 * (19 + 19 + 38);  // FLUX.1-schnell: qn + kn of every stream
    std::vector<uint16_t> host(n_vec * D);
    std::vector<double> want(n_vec, 0.0);
    for (size_t v = 0; v < n_vec; ++v)
      for (int i = 0; i < D; ++i) {
        const float w = (i % 7 == 3 ? -1.f : 1.f) * gain(rng);
        host[v * D + i] = to_bf16(w);
        const double a = std::fabs((double)from_bf16(host[v * D + i]));
        want[v] = a > want[v] ? a : want[v];
      }
    std::vector<float> got(n_vec, -1.f);
    dk_norm_weight_maxima(host.data(), n_vec, D, got.data());
    for (size_t v = 0; v < n_vec; ++v) CHECK((double)got[v] == want[v]);
    CHECK(dk_bf16_absmax(host.data() + (n_vec - 1) * D, (size_t)D) == got[n_vec - 1]);  // the last vector ends where the buffer ends
  }
  CHECK(dk_bf16_absmax(nullptr, 0) == 0.f);
  {
    uint16_t w[4] = {to_bf16(0.5f), 0x7f80 /* +inf */, to_bf16(-2.f), 0};
    CHECK(std::isinf(dk_bf16_absmax(w, 4)));
    w[1] = 0xffc0;  // NaN
    CHECK(std::isinf(dk_bf16_absmax(w, 4)));
    w[1] = 0x8000;  // -0
    CHECK(dk_bf16_absmax(w, 4) == 2.f);
  }
  // ---- the formula: max|w_q| max|w_k| sqrt(D) 1.02 at scale 1 / sqrt(D)
  for (int D : {64, 128}) {
    const float scale = 1.0f / std::sqrt((float)D);
    const float b = dk_score_bound(1.0625f, 1.09375f, D, scale);
    const double want = 1.0625 * 1.09375 * std::sqrt((double)D) * 1.02;
    CHECK(std::fabs((double)b - want) <= 1e-5 * want);
  }
  CHECK(std::fabs(dk_score_bound(1.08f, 1.08f, 128, 1.0f / std::sqrt(128.f)) - 13.46f) < 0.01f);  // the synthetic FLUX weights: B ~ 13
  CHECK(dk_score_bound(0.f, 1.f, 128, 0.1f) == 0.f);
  CHECK(dk_score_bound(1.f, 0.f, 128, 0.1f) == 0.f);
  CHECK(dk_score_bound(1.f, 1.f, 0, 0.1f) == 0.f);
  CHECK(dk_score_bound(1.f, 1.f, 128, 0.f) == 0.f);
  CHECK(dk_score_bound(INFINITY, 1.f, 128, 0.1f) == 0.f);
  CHECK(dk_score_bound(NAN, 1.f, 128, 0.1f) == 0.f);
  CHECK(dk_score_bound(3.0e30f, 3.0e30f, 128, 0.1f) == 0.f);  // overflow: no bound
  // ---- what the bound means: RMSNorm with the weights, bf16 roundings as the kernels place them, a rotation per pair -- no pair of rows exceeds it,
  // not even a query and a key that point the same way with every weight at its maximum
  {
    const int D = 128;
    const float scale = 1.0f / std::sqrt((float)D), eps = 1e-6f;
    std::vector<uint16_t> wq(D), wk(D);
    for (int i = 0; i < D; ++i) wq[i] = to_bf16(gain(rng)), wk[i] = to_bf16(gain(rng));
    const float bound = dk_score_bound(dk_bf16_absmax(wq.data(), D), dk_bf16_absmax(wk.data(), D), D, scale);
    auto normed = [&](const std::vector<float>& x, const std::vector<uint16_t>& w, float angle) {
      double ss = 0;
      for (float v : x) ss += (double)v * v;
      const float r = 1.0f / std::sqrt((float)(ss / D) + eps);
      std::vector<float> y(D);
      for (int i = 0; i < D; ++i) y[i] = from_bf16(to_bf16(x[i] * r * from_bf16(w[i])));
      for (int i = 0; i < D; i += 2) {
        const float c = std::cos(angle * (float)(i + 1)), s = std::sin(angle * (float)(i + 1)), a = y[i], b = y[i + 1];
        y[i] = from_bf16(to_bf16(c * a - s * b));
        y[i + 1] = from_bf16(to_bf16(s * a + c * b));
      }
      return y;
    };
    double worst = 0;
    for (int t = 0; t < 200; ++t) {
      std::vector<float> x(D), z(D);
      for (int i = 0; i < D; ++i) x[i] = unit(rng), z[i] = t % 2 ? x[i] : unit(rng);  // odd t: aligned query and key
      const float angle = t % 4 < 2 ? 0.f : 0.01f * (float)t;
      const std::vector<float> q = normed(x, wq, angle), k = normed(z, wk, angle);
      double dot = 0;
      for (int i = 0; i < D; ++i) dot += (double)q[i] * k[i];
      worst = std::fabs(dot * scale) > worst ? std::fabs(dot * scale) : worst;
    }
    printf("bound %.4f, worst |scale q.k| of 200 pairs %.4f\n", bound, worst);
    CHECK(worst <= bound && worst > 0.8 * bound);
  }
  printf(g_bad ? "%d checks FAILED\n" : "score bound: all checks passed\n", g_bad);
  return g_bad ? 1 : 0;
}
