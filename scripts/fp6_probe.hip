// fp6 probe (lab only): pins on hardware what the W4A6 GEMM (diffusionkit_amd/csrc/gemm256f4a6.hip), the MX-fp6 row quantiser
// (diffusionkit_amd/csrc/fp6_ops.hip) and the host format (diffusionkit_amd/weights.py: quantize_activation_mxfp6) assume about
// v_mfma_scale_f32_16x16x128_f8f6f4 with the FIRST operand fp4 (E2M1, cbsz = 4) and the SECOND fp6 (E2M3, blgp = 2) -- the companion of
// scripts/fp4_probe.hip, whose result (H0 of profiles/mxfp4_probe.log) is the fp4 side's layout here.
//   hipcc --offload-arch=gfx950 -O3 scripts/fp6_probe.hip -o build_lab/fp6_probe && timeout 120 build_lab/fp6_probe > profiles/mxfp6_probe.log
//
// 1. element map: ONE fp6 1.0 at 6-bit field e (bits [6 e, 6 e + 6) of the lane's register run, little-endian) of lane (row 0, group q); the
//    fp4 operand's row 0 names its K in three base-7 digits (E2M1 has seven non-zero magnitudes) -> D[0][0] names the K that field holds.
//    Fields 32 .. 41 lie in registers 6 and 7: they must read as nothing.
// 2. scale map: both operands ones; the fp4 operand selects one 32-K block; one lane's scale = 2^3, first on the fp6 side, then on the fp4 side
//    (the fp4 side's map must be that of profiles/mxfp4_probe.log).
// 3. hypotheses on random operands and scales against a host product, garbage in registers 6, 7 and in the unused scale bytes:
//      G0  lane (r, q) holds K [32 q, +32), element e in bits [6 e, 6 e + 6) of registers 0 .. 5
//      G1  the same elements, most significant field first (element e in bits [186 - 6 e, +6))
//      G2  the fp8 operand's two K = 64 halves: fields 0 .. 15 = K [16 q, +16), fields 16 .. 31 = K [64 + 16 q, +16)
//      G3  one element per byte of all eight registers (unpacked)
//    each with the fp4 operand as H0 and the scale byte of lane (r, g) = row r, K [32 g, +32) on both sides.
// 4. a dependent chain of the MFMA in the three format pairs (fp8 x fp4, fp6 x fp4, fp4 x fp4), one wave, and four independent chains in one wave.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

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

static const float kE2M1[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
static float e2m1_decode(int c) { return (c & 8) ? -kE2M1[c & 7] : kE2M1[c & 7]; }
static float e2m3_decode(int c) {
  const int s = (c >> 5) & 1, e = (c >> 3) & 3, m = c & 7;
  const float v = e == 0 ? m * 0.125f : ldexpf(1.0f + m / 8.0f, e - 1);
  return s ? -v : v;
}

// one wave: D[i][j] = sum_k A[i][k] * B[j][k]; A and B are RAW register images, 32 bytes per lane -- the host decides what they mean
template <int CBSZ, int BLGP, int OPSEL>
__global__ void mfma_once(const uint8_t* A, const uint8_t* B, const int* sa, const int* sb, float* D) {
  const int l = threadIdx.x, row = l & 15, q = l >> 4;
  const v8i a = *(const v8i*)(A + l * 32);
  const v8i b = *(const v8i*)(B + l * 32);
  v4f acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, CBSZ, BLGP, OPSEL, sa[l], OPSEL, sb[l]);
  for (int r = 0; r < 4; ++r) D[(4 * q + r) * 16 + row] = acc[r];  // D[i][j]: i = A row, j = B row
}

// chains: NCH independent accumulators, each a dependent chain of n MFMAs
template <int CBSZ, int BLGP, int NCH>
__global__ void mfma_chain(const uint8_t* A, const uint8_t* B, int n, float* D) {
  const int l = threadIdx.x;
  const v8i a = *(const v8i*)(A + l * 32);
  const v8i b = *(const v8i*)(B + l * 32);
  v4f acc[NCH];
  for (int c = 0; c < NCH; ++c) acc[c] = v4f{0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < n; ++i) {
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int c = 0; c < NCH; ++c) acc[c] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc[c], CBSZ, BLGP, 0, 127, 0, 127);
  }
  v4f s = acc[0];
  for (int c = 1; c < NCH; ++c) s += acc[c];
  for (int r = 0; r < 4; ++r) D[l * 4 + r] = s[r];
}

static void put_fp4(std::vector<uint8_t>& A, int r, int k, int code) {  // H0 of the fp4 probe
  A[((k / 32) * 16 + r) * 32 + (k % 32) / 2] |= (uint8_t)(code << (4 * (k & 1)));
}
static void put_bits6(std::vector<uint8_t>& B, int lane, int field, int code) {  // little-endian 6-bit field of the lane's 256 bits
  const int bit = 6 * field;
  for (int t = 0; t < 6; ++t)
    if ((code >> t) & 1) B[lane * 32 + ((bit + t) >> 3)] |= (uint8_t)(1 << ((bit + t) & 7));
}
// where K-element k of row r lives under hypothesis G
static void put_fp6(int G, std::vector<uint8_t>& B, int r, int k, int code) {
  if (G == 0) put_bits6(B, (k / 32) * 16 + r, k % 32, code);
  else if (G == 1) put_bits6(B, (k / 32) * 16 + r, 31 - k % 32, code);
  else if (G == 2) put_bits6(B, ((k % 64) / 16) * 16 + r, (k / 64) * 16 + k % 16, code);
  else B[((k / 32) * 16 + r) * 32 + k % 32] |= (uint8_t)code;
}

int main() {
  srand(1);
  uint8_t *dA, *dB;
  int *dsa, *dsb;
  float* dD;
  CK(hipMalloc(&dA, 2048)); CK(hipMalloc(&dB, 2048)); CK(hipMalloc(&dsa, 256)); CK(hipMalloc(&dsb, 256)); CK(hipMalloc(&dD, 1024));
  std::vector<int> ones(64, 127 | 0x11223300);
  std::vector<float> D(256);
  auto run = [&](const std::vector<uint8_t>& A, const std::vector<uint8_t>& B, const std::vector<int>& sa, const std::vector<int>& sb, int opsel) {
    CK(hipMemcpy(dA, A.data(), 2048, hipMemcpyHostToDevice));
    CK(hipMemcpy(dB, B.data(), 2048, hipMemcpyHostToDevice));
    CK(hipMemcpy(dsa, sa.data(), 256, hipMemcpyHostToDevice));
    CK(hipMemcpy(dsb, sb.data(), 256, hipMemcpyHostToDevice));
    if (opsel == 2) hipLaunchKernelGGL((mfma_once<4, 2, 2>), dim3(1), dim3(64), 0, 0, dA, dB, dsa, dsb, dD);
    else hipLaunchKernelGGL((mfma_once<4, 2, 0>), dim3(1), dim3(64), 0, 0, dA, dB, dsa, dsb, dD);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(D.data(), dD, 1024, hipMemcpyDeviceToHost));
  };

  // ---- 1. element map of the fp6 operand ----
  printf("element map, fp6 operand (src1, blgp = 2): (lane group q, 6-bit field e) of row 0 -> K (-1: the field reads as nothing)\n");
  {
    std::vector<uint8_t> Adig[3];
    for (int d = 0, div = 1; d < 3; ++d, div *= 7) {
      Adig[d].assign(2048, 0);
      for (int k = 0; k < 128; ++k) put_fp4(Adig[d], 0, k, 1 + (k / div) % 7);
    }
    for (int q = 0; q < 4; ++q) {
      std::string line;
      for (int e = 0; e < 42; ++e) {
        std::vector<uint8_t> B(2048, 0);
        put_bits6(B, q * 16 + 0, e, 0x08);  // E2M3 1.0 = 0b001000
        int k = 0, ok = 1;
        for (int d = 0, mul = 1; d < 3; ++d, mul *= 7) {
          run(Adig[d], B, ones, ones, 0);
          int digit = -1;
          for (int c = 1; c < 8; ++c)
            if (D[0] == kE2M1[c]) digit = c - 1;
          if (digit < 0) ok = 0;
          k += digit * mul;
        }
        char buf[24];
        snprintf(buf, 24, " %d", ok ? k : -1);
        line += buf;
        if (e == 31) line += " |";
      }
      printf("  q%d:%s\n", q, line.c_str());
    }
    // bit order inside a field: 0b000001 must be the subnormal step 0.125, 0b100000 the sign of zero
    std::vector<uint8_t> A1(2048, 0), B(2048, 0);
    for (int k = 0; k < 128; ++k) put_fp4(A1, 0, k, 2);
    put_bits6(B, 0, 5, 0x01);
    run(A1, B, ones, ones, 0);
    printf("  field code 0b000001 -> %g (E2M3: 0.125)\n", D[0]);
    B.assign(2048, 0);
    put_bits6(B, 0, 5, 0x3F);
    run(A1, B, ones, ones, 0);
    printf("  field code 0b111111 -> %g (E2M3: -7.5)\n", D[0]);
  }
  // ---- 2. scale maps ----
  for (int side = 0; side < 2; ++side) {
    printf("scale map, %s: lane L -> [row: block = D / 32 ...] where D != 32\n", side == 0 ? "fp6 operand (src1)" : "fp4 operand (src0), other side fp6");
    std::vector<uint8_t> B1(2048, 0);
    for (int r = 0; r < 16; ++r)
      for (int k = 0; k < 128; ++k) put_fp6(0, B1, r, k, 0x08);
    for (int L = 0; L < 64; ++L) {
      std::string line;
      for (int qb = 0; qb < 4; ++qb) {
        std::vector<uint8_t> A1(2048, 0);
        for (int r = 0; r < 16; ++r)
          for (int k = 32 * qb; k < 32 * qb + 32; ++k) put_fp4(A1, r, k, 2);
        std::vector<int> sc(64, 127);
        sc[L] = 130;
        if (side == 0) run(A1, B1, ones, sc, 0);
        else run(A1, B1, sc, ones, 0);
        for (int i = 0; i < 16; ++i) {
          const float d = side == 0 ? D[i] : D[i * 16];  // side 0: the fp6 row j = i of A row 0; side 1: A row i
          if (d != 32.f) { char buf[64]; snprintf(buf, 64, " %d:%d=%g", i, qb, d); line += buf; }
        }
      }
      printf("  L%2d ->%s\n", L, line.c_str());
    }
  }
  // ---- 3. hypotheses on random operands and scales ----
  {
    std::vector<int> a4(16 * 128), b6(16 * 128);
    for (auto& c : a4) c = rand() & 15;
    for (auto& c : b6) c = rand() & 63;
    for (int G = 0; G < 4; ++G)
      for (int opsel = 0; opsel <= 2; opsel += 2) {
        std::vector<uint8_t> A(2048, 0), B(2048, 0);
        for (int r = 0; r < 16; ++r)
          for (int k = 0; k < 128; ++k) { put_fp4(A, r, k, a4[r * 128 + k]); put_fp6(G, B, r, k, b6[r * 128 + k]); }
        for (int l = 0; l < 64; ++l) {
          for (int t = 16; t < 32; ++t) A[l * 32 + t] = (uint8_t)rand();               // fp4: registers 4 .. 7 are not read
          if (G != 3) for (int t = 24; t < 32; ++t) B[l * 32 + t] = (uint8_t)rand();   // fp6: registers 6, 7 are not read
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
              acc += (double)e2m1_decode(a4[i * 128 + k]) * e2m3_decode(b6[j * 128 + k]) * ldexp(1.0, ea[(k / 32) * 16 + i] - 127) *
                     ldexp(1.0, eb[(k / 32) * 16 + j] - 127);
            worst = fmax(worst, fabs(acc - D[i * 16 + j]));
            ref_max = fmax(ref_max, fabs(acc));
          }
        printf("hypothesis G%d, scale byte %d: max |D - ref| = %.3e (|ref| max %.3e)  %s\n", G, opsel, worst, ref_max, worst <= 1e-3 * ref_max ? "PASS" : "FAIL");
      }
  }
  // ---- 4. MFMA chains: one wave on the device, hipEvent time over n * 8 * NCH MFMAs ----
  {
    std::vector<uint8_t> A(2048, 0x22), B(2048, 0x22);
    CK(hipMemcpy(dA, A.data(), 2048, hipMemcpyHostToDevice));
    CK(hipMemcpy(dB, B.data(), 2048, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int n = 1 << 17;
    auto time_it = [&](const char* name, int nch, auto launch) {
      float best = 1e30f;
      for (int rep = 0; rep < 4; ++rep) {  // the first repeat warms the clocks
        CK(hipEventRecord(e0, 0));
        launch();
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep > 0) best = fminf(best, ms);
      }
      printf("mfma chain %-28s %d chain(s): %.3f ns per MFMA (best of 3, %d MFMAs)\n", name, nch, best * 1e6 / ((double)n * 8 * nch), n * 8 * nch);
    };
    time_it("fp8 (src1) x fp4 (src0)", 1, [&] { hipLaunchKernelGGL((mfma_chain<4, 0, 1>), dim3(1), dim3(64), 0, 0, dA, dB, n, dD); });
    time_it("fp6 (src1) x fp4 (src0)", 1, [&] { hipLaunchKernelGGL((mfma_chain<4, 2, 1>), dim3(1), dim3(64), 0, 0, dA, dB, n, dD); });
    time_it("fp4 (src1) x fp4 (src0)", 1, [&] { hipLaunchKernelGGL((mfma_chain<4, 4, 1>), dim3(1), dim3(64), 0, 0, dA, dB, n, dD); });
    time_it("fp8 (src1) x fp4 (src0)", 4, [&] { hipLaunchKernelGGL((mfma_chain<4, 0, 4>), dim3(1), dim3(64), 0, 0, dA, dB, n, dD); });
    time_it("fp6 (src1) x fp4 (src0)", 4, [&] { hipLaunchKernelGGL((mfma_chain<4, 2, 4>), dim3(1), dim3(64), 0, 0, dA, dB, n, dD); });
    time_it("fp4 (src1) x fp4 (src0)", 4, [&] { hipLaunchKernelGGL((mfma_chain<4, 4, 4>), dim3(1), dim3(64), 0, 0, dA, dB, n, dD); });
    CK(hipDeviceSynchronize());
  }
  return 0;
}
