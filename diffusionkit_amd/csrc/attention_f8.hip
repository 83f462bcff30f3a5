// Quantised joint attention forward, D = 128: both matrix products on v_mfma_scale_f32_16x16x128_f8f6f4 (OCP MX-fp8: e4m3 elements, one E8M0
// scale per 32 of the contraction).  bf16 in, bf16 out; training-free (SageAttention-style): nothing is calibrated, the operands are quantised
// per launch.  Two kernels.
//
// (a) dk_attn8_kv_kernel, once per launch: one workgroup per (batch row, head, 128-key tile) writes into the caller's workspace
//   K8    [B, H][Sp rows][128 e4m3]   Sp = S rounded up to 128.  Row r of a tile holds key kperm(r) of it (below); one scale per (key, 32 of D).
//   V8T   [B, H][tile][128 d][128 e4m3]   the values transposed, column c of a tile row = key c of the tile; one scale per (d, 32 consecutive keys)
//   SC    [B, H][tile][K: 512 | V: 512] E8M0 bytes: byte 8 * (16 g + (r & 15)) + (r >> 4) is the scale of row r (key row of K8, d row of V8T),
//         block g -- lane (l15, g) of the MFMA's scale operand wants the scales of rows f * 16 + l15, block g: ONE 8-byte load per lane brings a
//         wave a tile's 128 x 4 scales of one operand, 512 contiguous bytes.
//   Keys at positions >= S are written as zero elements under the scale 2^0: a poisoned workspace never reaches a result.
//
// (b) dk_attn8_fwd_kernel: one workgroup per (batch row, head, 128 queries), four waves of 32 queries, 128-key tiles.
//   The MFMA (operand layout pinned in gemm256f8.hip's header): D[i][j] = sum_k A[i][k] B[j][k]; lane (l15, q) supplies row l15 of A and of B,
//   K-elements [16 q, 16 q + 16) in its first four registers and [64 + 16 q, 64 + 16 q + 16) in its last four, and receives D[4 q + e][l15], e = 0..3.
//   Scores  S^T = K8 Q8^T:  A = 16 key rows (8 fragments), B = 16 queries (2 fragments): 16 MFMAs.  Lane (l15, q) then holds, for queries l15 and
//           16 + l15, the scores of tile rows r = 16 kf + 4 q + e: a softmax row lives in the four lanes l15 + 16 {0..3} (two shuffles per maximum).
//   P.V     O^T += V8T P8^T:  A = 16 d rows (8 fragments), B = 16 queries, contraction over the tile's 128 keys: 16 MFMAs.  Lane (l15, q) must supply
//           the probabilities of contraction positions c in [16 q, 16 q + 16) and [64 + 16 q, + 16).
//   Key order: K8 row r = [kf2 | kf1 kf0 | q1 q0 | e1 e0] holds the key at position c = kperm(r) = [kf2 | q1 q0 | kf1 kf0 | e1 e0] (the two 2-bit fields
//   swapped; an involution).  The 32 probabilities a lane holds per query are then exactly its 32 bytes of the P operand, register kf = its four
//   e, in order: P never passes through LDS, and V8T keeps the natural key order, so its block scales run over 32 CONSECUTIVE keys.
//   Q is normed / rotated in fp32, multiplied by scale * log2 e and quantised once (registers, with its four block scales in one scale register).
//   Softmax in fp32 on base-2 scores, running maximum with the deferred rescale (DKG_RESCALE_THR of attention_group.hip), the row sum over the fp32 p.
//   P leaves as e4m3 of p * 2^3: p <= e^4 = 54.6 -> 437 < 448, and p down to 2^-9 stays a normal number; the MFMA's scale byte 127 - 3 undoes it.
//   LDS: K8 / V8T tiles of 16 KiB, two slots each (64 KiB), rows of 128 bytes with gemm256f8.hip's swizzle (16-byte chunk c of row r at c ^ ((r >> 1) & 7));
//   loop = global loads of tile j + 1 into registers | barrier | tile j's arithmetic | LDS stores into the other slot: one barrier per tile.
#include <type_traits>
#include <utility>

#include "dk_kernels.h"

#define DK8_RESCALE_THR 4.0f  // natural-log units (attention_group.hip's DKG_RESCALE_THR)
#define DK8_P_LIFT 3          // P is stored as e4m3 of p * 2^3

struct Attn8Cfg {
  static constexpr int D = 128, NW = 4, KV = 128, QB = 128, NT = 256;
  static constexpr int TILE_BYTES = KV * D;  // 16 KiB, K8 and V8T alike
  static constexpr int SC_TILE = 1024;       // scale bytes per tile: K 512, V 512
  static constexpr int K_OFF = 0, V_OFF = 2 * TILE_BYTES;
  static constexpr int LDS_BYTES = 4 * TILE_BYTES;
  static constexpr int O_PITCH = 272;        // bytes per staged output row (256 + 16: the fragment writes of 16 rows spread over the banks)
  static constexpr int MAX_S = 65536;
};
static_assert(Attn8Cfg::NW * 32 * Attn8Cfg::O_PITCH <= Attn8Cfg::LDS_BYTES, "the output staging fits the tile slots");

typedef __attribute__((address_space(3))) char lds_char8;
typedef int i32x8_a8 __attribute__((ext_vector_type(8)));

// workspace of a launch (dk_attention_fp8_workspace_bytes): K8, V8T, SC per (batch row, head)
__host__ __device__ inline size_t dk_attn8_sp(int S) { return ((size_t)S + 127) / 128 * 128; }
size_t dk_attention_fp8_ws_bytes(int B, int H, int S) {
  if (B <= 0 || H <= 0 || S <= 0) return 0;
  return (size_t)B * H * dk_attn8_sp(S) * (128 + 128 + 8);
}
// position of tile row r in the contraction of P.V (file header)
__host__ __device__ inline int dk_attn8_kperm(int r) { return (r & 0x43) | ((r & 0x30) >> 2) | ((r & 0x0C) << 2); }

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): the MFMA's byte selects are immediates
template <class F, int... I>
__device__ __forceinline__ void dk8_for_impl(F& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void dk8_for(F f) {
  dk8_for_impl(f, std::make_integer_sequence<int, N>{});
}

// E8M0 byte of a block maximum (dk_mx8_quantize8's rule): the smallest power of two s with amax / s <= 448, clamped to [2^-126, 2^127]
__device__ __forceinline__ unsigned dk8_scale_byte(float amax) {
  const unsigned e = (__float_as_uint(amax * (1.0f / 448.0f)) + 0x7FFFFFu) >> 23;
  return e < 1u ? 1u : (e > 254u ? 254u : e);
}

// ---------------------------------------------------------------- (a) the K / V pre-pass ----------------------------------------------------------------
__global__ __launch_bounds__(256) void dk_attn8_kv_kernel(AttnParams p, unsigned char* ws) {
  using C = Attn8Cfg;
  __shared__ unsigned short vt[C::KV][C::D + 2];  // the tile's values, [key][d] (row pitch 65 words)
  const int tid = threadIdx.x;
  const int S = p.S, nt = (S + C::KV - 1) / C::KV;
  const int tile = blockIdx.x % nt, head = (blockIdx.x / nt) % p.H, b = blockIdx.x / (nt * p.H);
  const size_t sp = (size_t)nt * C::KV;
  const size_t bh = (size_t)b * p.H + head;
  unsigned char* const K8 = ws + bh * sp * C::D + (size_t)tile * C::TILE_BYTES;
  unsigned char* const V8 = ws + (size_t)p.B * p.H * sp * C::D + bh * sp * C::D + (size_t)tile * C::TILE_BYTES;
  unsigned char* const SC = ws + 2 * (size_t)p.B * p.H * sp * C::D + (bh * nt + tile) * C::SC_TILE;
  const bf16_t* Kb = p.K + (size_t)b * S * p.ld + head * C::D;
  const bf16_t* Vb = p.V + (size_t)b * S * p.ld + head * C::D;
  const int key0 = tile * C::KV;

  // keys: 16 lanes per key (8 d each: four adjacent lanes share a 32-d block), 16 keys per pass
  const int c8 = tid & 15;
#pragma unroll
  for (int pass = 0; pass < C::KV / 16; ++pass) {
    const int n = pass * 16 + (tid >> 4);  // position in the tile
    const int key = key0 + n;
    const bool real = key < S;
    const size_t row = (size_t)min(key, S - 1) * p.ld + c8 * 8;
    const u32x4 kw = *(const u32x4*)(Kb + row), vw = *(const u32x4*)(Vb + row);
    float v[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) unpack2bf(real ? kw[i] : 0u, v[2 * i], v[2 * i + 1]);
    unsigned e8;
    const uint2 q8 = dk_mx8_quantize8(v, e8);
    const int r = dk_attn8_kperm(n);  // (an involution: the row that holds position n)
    *(uint2*)(K8 + r * C::D + c8 * 8) = q8;
    if ((tid & 3) == 0) SC[8 * (16 * (c8 >> 2) + (r & 15)) + (r >> 4)] = (unsigned char)(real ? e8 : 127u);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned w = real ? vw[i] : 0u;
      vt[n][c8 * 8 + 2 * i] = (unsigned short)(w & 0xFFFFu);
      vt[n][c8 * 8 + 2 * i + 1] = (unsigned short)(w >> 16);
    }
  }
  __syncthreads();
  // values: 16 lanes per d (8 consecutive keys each: four adjacent lanes share a 32-key block), 16 d per pass
#pragma unroll
  for (int pass = 0; pass < C::D / 16; ++pass) {
    const int d = pass * 16 + (tid >> 4);
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = bf2f(vt[c8 * 8 + i][d]);
    unsigned e8;
    const uint2 q8 = dk_mx8_quantize8(v, e8);
    *(uint2*)(V8 + d * C::KV + c8 * 8) = q8;
    const bool real = key0 + (c8 >> 2) * 32 < S;  // (a block without a real key: zero elements, scale 2^0)
    if ((tid & 3) == 0) SC[512 + 8 * (16 * (c8 >> 2) + (d & 15)) + (d >> 4)] = (unsigned char)(real ? e8 : 127u);
  }
}

// ---------------------------------------------------------------- (b) the attention kernel ----------------------------------------------------------------
template <bool QFUSE>
__global__ __launch_bounds__(256) void dk_attn8_fwd_kernel(AttnParams p, const unsigned char* ws) {
  using C = Attn8Cfg;
  constexpr int D = C::D;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_char8* const lds = (lds_char8*)smem;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q4 = lane >> 4;
  const int S = p.S;
  const int nq = (S + C::QB - 1) / C::QB, nt = (S + C::KV - 1) / C::KV;
  int t;
  {  // consecutive tasks (query blocks of one head: the same K8 / V8T) on one XCD, as attention_group.hip
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int xcd = bid & 7, qq = nwg >> 3, r = nwg & 7;
    t = (xcd < r ? xcd * (qq + 1) : r * (qq + 1) + (xcd - r) * qq) + (bid >> 3);
  }
  const int qb = t % nq, head = (t / nq) % p.H, b = t / (nq * p.H);
  const int q0 = qb * C::QB + wave * 32;
  const size_t sp = (size_t)nt * C::KV;
  const size_t bh = (size_t)b * p.H + head;
  const unsigned char* const K8 = ws + bh * sp * D;
  const unsigned char* const V8 = ws + (size_t)p.B * p.H * sp * D + bh * sp * D;
  const unsigned char* const SC = ws + 2 * (size_t)p.B * p.H * sp * D + bh * nt * C::SC_TILE;

  // ---- staging: thread i-th 16-byte chunk of a tile (both operands are 128 rows of 128 bytes, contiguous in the workspace) ----
  unsigned st_off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = tid + C::NT * i, row = id >> 3, ch = id & 7;
    st_off[i] = (unsigned)(row * 128 + ((ch ^ ((row >> 1) & 7)) << 4));
  }
  u32x4 kreg[4], vreg[4];
  u32x2 ksc_n, vsc_n, ksc, vsc;
  auto load_tile = [&](int jt) {
    const unsigned char* kp = K8 + (size_t)jt * C::TILE_BYTES + tid * 16;
    const unsigned char* vp = V8 + (size_t)jt * C::TILE_BYTES + tid * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      kreg[i] = *(const u32x4*)(kp + i * C::NT * 16);
      vreg[i] = *(const u32x4*)(vp + i * C::NT * 16);
    }
    ksc_n = *(const u32x2*)(SC + (size_t)jt * C::SC_TILE + lane * 8);
    vsc_n = *(const u32x2*)(SC + (size_t)jt * C::SC_TILE + 512 + lane * 8);
  };
  auto store_tile = [&](int slot) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *(__attribute__((address_space(3))) u32x4*)(lds + C::K_OFF + slot * C::TILE_BYTES + st_off[i]) = kreg[i];
      *(__attribute__((address_space(3))) u32x4*)(lds + C::V_OFF + slot * C::TILE_BYTES + st_off[i]) = vreg[i];
    }
  };
  // fragment f of a staged operand: rows 16 f + l15, chunks q4 and 4 + q4 (the swizzle term (row >> 1) & 7 = l15 >> 1: 16 f adds nothing below bit 3)
  const unsigned fr_lo = (unsigned)(l15 * 128 + ((q4 ^ (l15 >> 1)) << 4)), fr_hi = (unsigned)(l15 * 128 + (((4 + q4) ^ (l15 >> 1)) << 4));
  auto frag = [&](int base, int f) {
    const u32x4 lo = *(const __attribute__((address_space(3))) u32x4*)(lds + base + f * 2048 + fr_lo);
    const u32x4 hi = *(const __attribute__((address_space(3))) u32x4*)(lds + base + f * 2048 + fr_hi);
    return __builtin_bit_cast(i32x8_a8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
  };

  // ---- Q: lane (l15, q4) holds d in [16 q4, + 16) and [64 + 16 q4, + 16) of queries q0 + 16 qf + l15; norm / RoPE in fp32 (attention4.hip's
  // arithmetic), times scale * log2 e, then MX-fp8: D-block g = [32 g, + 32) is the first halves of lanes q4 = 2 g, 2 g + 1 (g < 2) or their
  // second halves (g >= 2); lane (l15, g) keeps the scale byte of block g of query qf in byte qf of qsc ----
  const float cfold = p.scale * 1.44269504088896340736f;
  i32x8_a8 qf8[2];
  unsigned qsc = 0u;
#pragma unroll
  for (int qf = 0; qf < 2; ++qf) {
    const int qrow = min(q0 + qf * 16 + l15, S - 1);
    const bf16_t* qp = p.Q + ((size_t)b * S + qrow) * p.ld + head * D + q4 * 16;
    float v[2][16];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const u32x4 w = *(const u32x4*)(qp + h * 64 + i * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) unpack2bf(w[e], v[h][i * 8 + 2 * e], v[h][i * 8 + 2 * e + 1]);
      }
    if (QFUSE) {
      if (p.qn_a != nullptr) {
        const bf16_t* wp = (qrow < p.qn_split ? p.qn_a : p.qn_b) + q4 * 16;
        float ss = 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int e = 0; e < 16; ++e) ss += v[h][e] * v[h][e];
        ss += __shfl_xor(ss, 16, 64);
        ss += __shfl_xor(ss, 32, 64);
        const float r = rsqrtf(ss / (float)D + p.qn_eps);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int e = 0; e < 16; ++e) v[h][e] = round_bf16(v[h][e] * r * bf2f(wp[h * 64 + e]));
      }
      if (p.q_rope != nullptr) {
        const float* tab = p.q_rope + ((size_t)qrow * (D / 2) + q4 * 8) * 2;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const float c = tab[h * 64 + 2 * i], sn = tab[h * 64 + 2 * i + 1], xe = v[h][2 * i], xo = v[h][2 * i + 1];
            v[h][2 * i] = c * xe - sn * xo;
            v[h][2 * i + 1] = sn * xe + c * xo;
          }
      }
    }
    float am[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        v[h][e] *= cfold;
        am[h] = fmaxf(am[h], fabsf(v[h][e]));
      }
    // blocks (q4 >> 1) and 2 + (q4 >> 1) are this lane's; the lane 32 away holds the other two
    am[0] = fmaxf(am[0], __shfl_xor(am[0], 16, 64));
    am[1] = fmaxf(am[1], __shfl_xor(am[1], 16, 64));
    const float o0 = __shfl_xor(am[0], 32, 64), o1 = __shfl_xor(am[1], 32, 64);
    const unsigned e_own[2] = {dk8_scale_byte(am[0]), dk8_scale_byte(am[1])};
    // the byte lane (l15, g = q4) supplies: block g = half (g >> 1) of the lane pair (g & 1): g = 0 / 3 the lane's own, g = 1 / 2 the other pair's
    const unsigned e_g = q4 == 0 ? e_own[0] : q4 == 1 ? dk8_scale_byte(o0) : q4 == 2 ? dk8_scale_byte(o1) : e_own[1];
    qsc |= e_g << (8 * qf);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float inv = __uint_as_float((254u - e_own[h]) << 23);  // 2^(127 - e)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(v[h][4 * i] * inv, v[h][4 * i + 1] * inv, w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(v[h][4 * i + 2] * inv, v[h][4 * i + 3] * inv, w, true);
        qf8[qf][h * 4 + i] = w;
      }
    }
  }

  f32x4 o[8][2];  // O^T: [d fragment][query fragment]; lane holds d = 16 df + 4 q4 + e of query 16 qf + l15
#pragma unroll
  for (int df = 0; df < 8; ++df)
#pragma unroll
    for (int qf = 0; qf < 2; ++qf) o[df][qf] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float NEG_INF = -__builtin_inff();
  float m_run[2] = {NEG_INF, NEG_INF}, l_run[2] = {0.f, 0.f};
  const float thr = DK8_RESCALE_THR * 1.44269504088896340736f;  // the scores are base-2 exponents already
  constexpr int P_SCALE = (127 - DK8_P_LIFT) * 0x01010101;
  const float lift = (float)(1 << DK8_P_LIFT);

  load_tile(0);
  store_tile(0);
  ksc = ksc_n, vsc = vsc_n;
  int slot = 0;
  for (int j = 0; j < nt; ++j) {
    if (j + 1 < nt) load_tile(j + 1);
    __syncthreads();  // slot `slot` is complete; every wave is past its reads of slot ^ 1
    // ---- scores: s[kf][qf][e] = tile row 16 kf + 4 q4 + e (key position kperm of it) x query 16 qf + l15 ----
    f32x4 s[8][2];
    dk8_for<8>([&](auto kf_c) {
      constexpr int kf = decltype(kf_c)::value;
      const i32x8_a8 ka = frag(C::K_OFF + slot * C::TILE_BYTES, kf);
      s[kf][0] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(ka, qf8[0], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, kf & 3, (int)ksc[kf >> 2], 0, (int)qsc);
      s[kf][1] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(ka, qf8[1], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, kf & 3, (int)ksc[kf >> 2], 1, (int)qsc);
    });
    if (j == nt - 1 && (S & (C::KV - 1)) != 0) {  // keys beyond S: probability exactly 0 (their quantised score is 0, not -inf)
      const int left = S - j * C::KV;
#pragma unroll
      for (int kf = 0; kf < 8; ++kf)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool dead = 64 * (kf >> 2) + 16 * q4 + 4 * (kf & 3) + e >= left;
          s[kf][0][e] = dead ? NEG_INF : s[kf][0][e];
          s[kf][1][e] = dead ? NEG_INF : s[kf][1][e];
        }
    }
    // ---- online softmax: a row is the four lanes l15 + 16 {0..3}; the rescale is decided per row (attention_group.hip) ----
    i32x8_a8 pf[2];
#pragma unroll
    for (int qf = 0; qf < 2; ++qf) {
      float mx = s[0][qf][0];
#pragma unroll
      for (int kf = 0; kf < 8; ++kf)
#pragma unroll
        for (int e = 0; e < 4; ++e) mx = fmaxf(mx, s[kf][qf][e]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const bool need = mx - m_run[qf] > thr;  // (no maximum yet: the difference is +inf)
      if (__any(need)) {
        const float m_new = need ? fmaxf(m_run[qf], mx) : m_run[qf];
        const float alpha = !need ? 1.f : m_run[qf] == NEG_INF ? 0.f : __builtin_amdgcn_exp2f(m_run[qf] - m_new);
        m_run[qf] = m_new;
        l_run[qf] *= alpha;
#pragma unroll
        for (int df = 0; df < 8; ++df) o[df][qf] *= alpha;
      }
      const float mc = m_run[qf] == NEG_INF ? 0.f : m_run[qf];
      float psum = 0.f;
#pragma unroll
      for (int kf = 0; kf < 8; ++kf) {
        float pe[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          pe[e] = __builtin_amdgcn_exp2f(s[kf][qf][e] - mc);
          psum += pe[e];
        }
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(pe[0] * lift, pe[1] * lift, w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(pe[2] * lift, pe[3] * lift, w, true);
        pf[qf][kf] = w;  // contraction positions 64 (kf >> 2) + 16 q4 + 4 (kf & 3) + e: register kf of the operand
      }
      l_run[qf] += psum;
    }
    // ---- O^T += V8T P8^T ----
    dk8_for<8>([&](auto df_c) {
      constexpr int df = decltype(df_c)::value;
      const i32x8_a8 va = frag(C::V_OFF + slot * C::TILE_BYTES, df);
      o[df][0] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(va, pf[0], o[df][0], 0, 0, df & 3, (int)vsc[df >> 2], 0, P_SCALE);
      o[df][1] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(va, pf[1], o[df][1], 0, 0, df & 3, (int)vsc[df >> 2], 0, P_SCALE);
    });
    if (j + 1 < nt) {
      store_tile(slot ^ 1);
      ksc = ksc_n, vsc = vsc_n;
    }
    slot ^= 1;
  }

  // ---- normalise, stage the wave's 32 rows in LDS (the tile slots are free behind the barrier), store whole rows ----
  __syncthreads();
  lds_char8* const stage = lds + wave * 32 * C::O_PITCH;
#pragma unroll
  for (int qf = 0; qf < 2; ++qf) {
    float l = l_run[qf];
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = l > 0.f ? 1.0f / l : 0.f;
#pragma unroll
    for (int df = 0; df < 8; ++df) {
      const u32x2 w = {pack2bf(o[df][qf][0] * inv, o[df][qf][1] * inv), pack2bf(o[df][qf][2] * inv, o[df][qf][3] * inv)};
      *(__attribute__((address_space(3))) u32x2*)(stage + (qf * 16 + l15) * C::O_PITCH + (df * 16 + q4 * 4) * 2) = w;
    }
  }
  // (wave-private staging: the wave's own LDS writes are complete before its reads -- same wave, in order; no barrier)
#pragma unroll
  for (int pass = 0; pass < 8; ++pass) {
    const int row = pass * 4 + q4, qrow = q0 + row;
    const u32x4 w = *(const __attribute__((address_space(3))) u32x4*)(stage + row * C::O_PITCH + l15 * 16);
    if (qrow < S) *(u32x4*)(p.O + ((size_t)b * S + qrow) * p.ldo + head * D + l15 * 8) = w;
  }
}

template <bool QFUSE>
static int launch_attn8(const AttnParams& p, hipStream_t stream) {
  using C = Attn8Cfg;
  static DkDeviceOnce attr_once;
  if (attr_once.first()) {
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_attn8_fwd_kernel<QFUSE>, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES));
    attr_once.mark();
  }
  const long tasks = (long)((p.S + C::QB - 1) / C::QB) * p.H * p.B;
  hipLaunchKernelGGL((dk_attn8_fwd_kernel<QFUSE>), dim3((unsigned)tasks), dim3(C::NT), C::LDS_BYTES, stream, p, (const unsigned char*)p.f8_ws);
  return 0;
}

// the quantised route (the argument checks that name a rule: dk_attention_route): pre-pass, then the attention kernel
int dk_launch_attention_f8(const AttnParams& p, hipStream_t stream) {
  using C = Attn8Cfg;
  DK_REQUIRE(p.f8_ws != nullptr && p.D == 128 && p.dtype == DK_DTYPE_BF16 && p.bias == nullptr && p.groups == nullptr && p.ident_from == 0,
             "fp8 attention: bf16, head_dim 128, no bias, no groups, no identity attention");
  DK_REQUIRE(p.S <= C::MAX_S && p.f8_ws_bytes >= dk_attention_fp8_ws_bytes(p.B, p.H, p.S) && ((uintptr_t)p.f8_ws & 15) == 0 && p.ldo % 8 == 0 &&
                 ((uintptr_t)p.O & 15) == 0,
             "fp8 attention: S <= 65536, a workspace of dk_attention_fp8_workspace_bytes, 16-byte aligned; 16-byte aligned output rows");
  const long tiles = (long)((p.S + C::KV - 1) / C::KV) * p.H * p.B;
  hipLaunchKernelGGL(dk_attn8_kv_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, p, (unsigned char*)p.f8_ws);
  const bool qfuse = p.qn_a != nullptr || p.q_rope != nullptr;
  return qfuse ? launch_attn8<true>(p, stream) : launch_attn8<false>(p, stream);
}
