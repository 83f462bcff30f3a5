// fp4 probe (lab only): pins on hardware what the MX-fp4 GEMM (diffusionkit_amd/csrc/gemm256f4.hip) and its packer
// (diffusionkit_amd/weights.py: pack_mxfp4) assume about v_mfma_scale_f32_16x16x128_f8f6f4 with the FIRST operand fp4 (E2M1, cbsz = 4,
// four live registers per lane) and the second fp8 (e4m3, blgp = 0) -- the companion of scripts/fp8_probe.hip.
//   hipcc --offload-arch=gfx950 -O3 scripts/fp4_probe.hip -o build_lab/fp4_probe && build_lab/fp4_probe
//
// 1. element map: ONE fp4 1.0 at (lane group q, register j, nibble t) of row 0, the fp8 operand's row 0 = a value that names its K
//    (two passes: 1 + k % 16, then 1 + k / 16; fp8 layout as profiles/r02_fp8_probe.log found it) -> D[0][0] names the K that position holds.
// 2. scale map: fp4 ones, the fp8 operand selects one (32-K block, 16-K half), one lane's scale = 2^3 -> which rows / blocks lane L's byte governs.
// 3. hypotheses, random operands and random scales against a host product (the failing ones stay in the log):
//      H0  lane (r, q) holds K [32 q, +32), low nibble first      (the fp8 probe's FIRST hypothesis, carried over)
//      H1  the same, high nibble first
//      H2  registers 0-1 hold K [16 q, +16), registers 2-3 K [64 + 16 q, +16), low nibble first (the fp8 operand's two K = 64 halves, at half the bytes)
//      H3  the same, high nibble first
//    each with the scale byte of lane (r, g) = row r, K [32 g, +32) on BOTH operands, read from byte `opsel` of the scale register
//    (bytes 0 and 2 are tried, garbage in the other bytes).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));

#define CK(x)                                                            \
  do {                                                                   \
    hipError_t e_ = (x);                                                 \
    if (e_ != hipSuccess) {                                              \
      printf("HIP error %s line %d\n", hipGetErrorString(e_), __LINE__); \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

static float e4m3_decode(uint8_t b) {
  const int s = b >> 7, e = (b >> 3) & 15, m = b & 7;
  const float v = e == 0 ? ldexpf((float)m, -9) : ldexpf(1.0f + m / 8.0f, e - 7);
  return s ? -v : v;
}
static float e2m1_decode(int c) {
  static const float mag[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
  return (c & 8) ? -mag[c & 7] : mag[c & 7];
}
static uint8_t e4m3_small_int(int v) {  // 1 .. 16, exact
  for (int c = 0; c < 0x7F; ++c)
    if (e4m3_decode((uint8_t)c) == (float)v) return (uint8_t)c;
  return 0;
}

// one wave: D[i][j] = sum_k A4[i][k] * B8[j][k] with per-lane scale registers.  A4: the RAW register image of the fp4 operand, 16 bytes per
// lane (lane l = bytes [16 l, +16)) -- the host decides what K they mean; B8: fp8 [16][128] row-major, loaded in the fp8 probe's layout.
template <int OPSEL>
__global__ void mfma_once(const uint8_t* A4, const uint8_t* B8, const int* sa, const int* sb, float* D) {
  const int l = threadIdx.x, row = l & 15, q = l >> 4;
  const v4i a4 = *(const v4i*)(A4 + l * 16);
  const v8i a = __builtin_shufflevector(a4, a4, 0, 1, 2, 3, -1, -1, -1, -1);
  v8i b;
  for (int j = 0; j < 8; ++j) b[j] = *(const int*)(B8 + row * 128 + (j < 4 ? q * 16 + 4 * j : 64 + q * 16 + 4 * (j - 4)));
  v4f acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, 4, 0, OPSEL, sa[l], OPSEL, sb[l]);
  for (int r = 0; r < 4; ++r) D[(4 * q + r) * 16 + row] = acc[r];  // D[i][j]: i = A row, j = B row
}

// register image position (byte of the lane's 16, nibble) of K-element k under hypothesis H; *lane_q = the lane group that holds it
static int pos_of(int H, int k, int* lane_q, int* nib) {
  int q, e;  // e: element index 0..31 inside the lane
  if (H < 2) { q = k / 32; e = k % 32; }
  else { q = (k % 64) / 16; e = (k / 64) * 16 + k % 16; }
  *lane_q = q;
  *nib = (H & 1) ? 1 - (e & 1) : (e & 1);  // 0: low nibble
  return e >> 1;
}

int main() {
  srand(1);
  uint8_t *dA, *dB;
  int *dsa, *dsb;
  float* dD;
  CK(hipMalloc(&dA, 1024)); CK(hipMalloc(&dB, 2048)); CK(hipMalloc(&dsa, 256)); CK(hipMalloc(&dsb, 256)); CK(hipMalloc(&dD, 1024));
  std::vector<int> ones(64, 127 | 0x11223300);
  std::vector<float> D(256);
  auto run = [&](const std::vector<uint8_t>& A, const std::vector<uint8_t>& B, const std::vector<int>& sa, const std::vector<int>& sb, int opsel) {
    CK(hipMemcpy(dA, A.data(), 1024, hipMemcpyHostToDevice));
    CK(hipMemcpy(dB, B.data(), 2048, hipMemcpyHostToDevice));
    CK(hipMemcpy(dsa, sa.data(), 256, hipMemcpyHostToDevice));
    CK(hipMemcpy(dsb, sb.data(), 256, hipMemcpyHostToDevice));
    if (opsel == 2) hipLaunchKernelGGL(mfma_once<2>, dim3(1), dim3(64), 0, 0, dA, dB, dsa, dsb, dD);
    else hipLaunchKernelGGL(mfma_once<0>, dim3(1), dim3(64), 0, 0, dA, dB, dsa, dsb, dD);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(D.data(), dD, 1024, hipMemcpyDeviceToHost));
  };

  // ---- 1. element map ----
  printf("element map: (lane group q, register j, nibble t [0 = low]) of row 0 -> K\n");
  {
    std::vector<uint8_t> Blo(2048, 0), Bhi(2048, 0);
    for (int k = 0; k < 128; ++k) { Blo[k] = e4m3_small_int(1 + k % 16); Bhi[k] = e4m3_small_int(1 + k / 16); }
    for (int q = 0; q < 4; ++q)
      for (int j = 0; j < 4; ++j) {
        std::string line;
        for (int t = 0; t < 8; ++t) {
          std::vector<uint8_t> A(1024, 0);
          A[(q * 16 + 0) * 16 + j * 4 + t / 2] = (uint8_t)(0x2 << (4 * (t & 1)));  // E2M1 1.0 = 0b0010; lane = q * 16 + row 0
          run(A, Blo, ones, ones, 0);
          const float lo = D[0];
          run(A, Bhi, ones, ones, 0);
          const float hi = D[0];
          char buf[48];
          snprintf(buf, 48, " b%d.%c=%d", t / 2, (t & 1) ? 'h' : 'l', (lo >= 1 && hi >= 1) ? (int)(hi - 1) * 16 + (int)(lo - 1) : -1);
          line += buf;
        }
        printf("  q%d r%d:%s\n", q, j, line.c_str());
      }
  }
  // ---- 2. scale map: fp4 operand = ones, fp8 operand selects (block qb, half hf); scale of lane L = 2^3 ----
  {
    printf("scale map, fp4 operand (src0): lane L -> [row: (block, half) = D / 16 ...] where D != 16\n");
    const std::vector<uint8_t> A1(1024, 0x22);
    for (int L = 0; L < 64; ++L) {
      std::string line;
      for (int qb = 0; qb < 4; ++qb)
        for (int hf = 0; hf < 2; ++hf) {
          std::vector<uint8_t> B1(2048, 0);
          for (int r = 0; r < 16; ++r)
            for (int k = 0; k < 128; ++k) B1[r * 128 + k] = (k / 32 == qb && (k % 32) / 16 == hf) ? 0x38 : 0x00;  // 0x38 = 1.0 in e4m3
          std::vector<int> sa(64, 127);
          sa[L] = 130;
          run(A1, B1, sa, ones, 0);
          for (int i = 0; i < 16; ++i)
            if (D[i * 16] != 16.f) { char buf[64]; snprintf(buf, 64, " %d:(%d,%d)=%g", i, qb, hf, D[i * 16]); line += buf; }
        }
      printf("  L%2d ->%s\n", L, line.c_str());
    }
  }
  // ---- 3. hypotheses on random operands and scales ----
  {
    std::vector<int> a4(16 * 128);  // E2M1 codes [row][k]
    std::vector<uint8_t> B(2048);
    for (auto& c : a4) c = rand() & 15;
    for (auto& x : B) do x = (uint8_t)(rand() & 0xFF); while ((x & 0x7F) == 0x7F || ((x >> 3) & 15) > 9);  // |value| < 8
    for (int H = 0; H < 4; ++H)
      for (int opsel = 0; opsel <= 2; opsel += 2) {
        std::vector<uint8_t> A(1024, 0);
        for (int r = 0; r < 16; ++r)
          for (int k = 0; k < 128; ++k) {
            int q, nib;
            const int byte = pos_of(H, k, &q, &nib);
            A[(q * 16 + r) * 16 + byte] |= (uint8_t)(a4[r * 128 + k] << (4 * nib));
          }
        std::vector<int> sa(64), sb(64), ea(64), eb(64);
        for (int l = 0; l < 64; ++l) {
          ea[l] = 121 + rand() % 12; eb[l] = 121 + rand() % 12;
          const int junk_a = rand(), junk_b = rand();
          sa[l] = (junk_a & ~(0xFF << (8 * opsel))) | (ea[l] << (8 * opsel));
          sb[l] = (junk_b & ~(0xFF << (8 * opsel))) | (eb[l] << (8 * opsel));
        }
        run(A, B, sa, sb, opsel);
        double worst = 0, ref_max = 0;
        for (int i = 0; i < 16; ++i)
          for (int j = 0; j < 16; ++j) {
            double acc = 0;
            for (int k = 0; k < 128; ++k)
              acc += (double)e2m1_decode(a4[i * 128 + k]) * e4m3_decode(B[j * 128 + k]) * ldexp(1.0, ea[(k / 32) * 16 + i] - 127) *
                     ldexp(1.0, eb[(k / 32) * 16 + j] - 127);
            worst = fmax(worst, fabs(acc - D[i * 16 + j]));
            ref_max = fmax(ref_max, fabs(acc));
          }
        printf("hypothesis H%d, scale byte %d: max |D - ref| = %.3e (|ref| max %.3e)  %s\n", H, opsel, worst, ref_max, worst <= 1e-3 * ref_max ? "PASS" : "FAIL");
      }
  }
  return 0;
}
