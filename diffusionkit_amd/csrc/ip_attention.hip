// Decoupled image-prompt attention (FLUX IP-Adapter, the XLabs form as diffusers' FluxIPAdapterJointAttnProcessor2_0 runs it): the image
// queries of a double block, QK-normed but not rotated, attend to the N <= 16 keys / values the adapter projected from the image prompt.
//   ip[m, head] = softmax_n( scale * q_n[m, head] . K[b, n, head] ) @ V[b, :, head],   q_n = round_bf16( q * rsqrt(mean(q^2) + eps) * w )
// q is the RAW q projection inside the block's QKV buffer (the attention kernel norms and rotates in its own Q load, so the buffer still holds
// it); q_n takes the Q load's expression and rounding (attention5.hip), scores, the exact max-subtracted softmax over the N keys and the
// weighted sum stay in fp32, and the result is rounded once.  No reference counterpart (the reference has no adapter).
//
// Memory-bound: the kernel reads q and writes ip, 2 * h * 2 bytes per row.  A workgroup owns 512 columns (4 heads of D = 128, one 16-byte
// piece per lane) of IP_ROWS consecutive rows of ONE image: the keys and values of its four heads, 2 N pieces per lane, are staged in LDS
// once and re-read per row; a wave issues the loads of four rows back to back before it touches the first.  A head is 16 lanes -- one DPP
// row -- so the sum of squares and the N dot products reduce with four DPP adds each, xor butterflies (every lane of the head ends with the
// same bits).  Loads and stores are buffer instructions whose resource spans one row's head range (h * 2 bytes from a scalar row base):
// lanes past the row end read zeros and their stores are dropped; the k / v columns of QKV, its text rows and a row past the image's last
// (a resource of zero bytes) are never addressed.
#include "dk_kernels.h"

struct IpAttnParams {
  const bf16_t* q;   // the q columns of the first image row of batch row 0
  const bf16_t* qn;  // [128]
  const bf16_t *K, *V;  // [B, N, h] at ldkv elements per row
  bf16_t* out;       // [B * seg_len, h] dense
  int ldq, seg_len, seg_stride, ldkv, h;
  float scale, eps;
};
constexpr int IP_ROWS = 32;  // rows of a workgroup: 8 per wave, two groups of four loads

// sum over the 16 lanes of a DPP row: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror -- each step adds the partner's value to
// the lane's own, a commutative add on both sides, so all 16 lanes hold the same bits
__device__ __forceinline__ float ip_row_sum(float v) {
  int x = __float_as_int(v);
  v += __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false));
  x = __float_as_int(v);
  v += __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x4E, 0xF, 0xF, false));
  x = __float_as_int(v);
  v += __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x141, 0xF, 0xF, false));
  x = __float_as_int(v);
  return v + __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x140, 0xF, 0xF, false));
}
__device__ __forceinline__ void ip_unpack8(const u32x4& r, float* v) {
#pragma unroll
  for (int e = 0; e < 4; ++e) unpack2bf(r[e], v[2 * e], v[2 * e + 1]);
}

template <int N>
__global__ __launch_bounds__(256) void dk_ip_attention_kernel(IpAttnParams p) {
  __shared__ u32x4 kv[2 * N * 64];  // [K | V][n][lane]: the piece lane `lane` of every wave reads
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (uniform: row bases live in SGPRs)
  const int blocks_per_image = (p.seg_len + IP_ROWS - 1) / IP_ROWS;
  const int b = (int)blockIdx.x / blocks_per_image, r0 = ((int)blockIdx.x % blocks_per_image) * IP_ROWS;
  const int off = ((int)blockIdx.y * 64 + lane) * 16;  // byte offset of the lane's piece inside a row of h elements
  const int bytes = p.h * 2;
  for (int j = wave; j < 2 * N; j += 4) {  // row j of the image's [K | V] stack: one 1-KiB piece per wave instruction
    const bf16_t* row = (j < N ? p.K : p.V) + ((size_t)b * N + (j < N ? j : j - N)) * p.ldkv;
    const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void*)row, 0, bytes, 0x00020000);
    kv[j * 64 + lane] = __builtin_amdgcn_raw_buffer_load_b128(rk, off, 0, 0);
  }
  float w[8];
  ip_unpack8(*(const u32x4*)(p.qn + (lane & 15) * 8), w);
  __syncthreads();
#pragma unroll 1
  for (int g = 0; g < IP_ROWS / 16; ++g) {
    u32x4 raw[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + wave + 4 * (4 * g + u);
      const bool live = r < p.seg_len;  // (uniform; a row past the image's last: a resource of zero bytes at the image's first row)
      const bf16_t* row = p.q + ((size_t)b * p.seg_stride + (live ? r : 0)) * p.ldq;
      const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void*)row, 0, live ? bytes : 0, 0x00020000);
      raw[u] = __builtin_amdgcn_raw_buffer_load_b128(rq, off, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + wave + 4 * (4 * g + u);
      if (r >= p.seg_len) break;  // (uniform, and the rows of a wave ascend)
      float v[8];
      ip_unpack8(raw[u], v);
      float ss = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) ss += v[e] * v[e];
      const float rn = rsqrtf(ip_row_sum(ss) / 128.0f + p.eps);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = round_bf16(v[e] * rn * w[e]);
      float s[N], mx = -INFINITY;
#pragma unroll
      for (int n = 0; n < N; ++n) {
        float k[8], d = 0.f;
        ip_unpack8(kv[n * 64 + lane], k);
#pragma unroll
        for (int e = 0; e < 8; ++e) d += v[e] * k[e];
        s[n] = ip_row_sum(d) * p.scale;
        mx = fmaxf(mx, s[n]);
      }
      float l = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int n = 0; n < N; ++n) {
        const float pn = __expf(s[n] - mx);  // (a NaN score: fmaxf passes it by, pn and with it l are NaN -- the whole head's row)
        float vv[8];
        ip_unpack8(kv[(N + n) * 64 + lane], vv);
        l += pn;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += pn * vv[e];
      }
      const float inv = 1.0f / l;
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = pack2bf(acc[2 * e] * inv, acc[2 * e + 1] * inv);
      const __amdgpu_buffer_rsrc_t ro =
          __builtin_amdgcn_make_buffer_rsrc((void*)(p.out + ((size_t)b * p.seg_len + r) * p.h), 0, bytes, 0x00020000);
      __builtin_amdgcn_raw_buffer_store_b128(o, ro, off, 0, 0);  // (past the row end: dropped)
    }
  }
}

// qkv: a joint [B, seg_stride, ldq] buffer whose row holds the q projection in its first h columns; the rows read are first_row ..
// first_row + seg_len - 1 of every batch row, nothing else, and of those the first h columns
int dk_launch_ip_attention(const bf16_t* qkv, int ldq, int seg_len, int seg_stride, int first_row, const bf16_t* qn, const bf16_t* K, const bf16_t* V,
                           int ldkv, int B, int N, int h, int D, float scale, float eps, bf16_t* out, hipStream_t stream) {
  DK_REQUIRE(D == 128, "ip_attention: head_dim must be 128");
  DK_REQUIRE(N >= 1 && N <= 16, "ip_attention: the number of image-prompt tokens must lie in [1, 16]");
  DK_REQUIRE(qkv && qn && K && V && out, "ip_attention: null argument");
  DK_REQUIRE(B > 0 && seg_len > 0 && first_row >= 0 && (B == 1 || first_row + seg_len <= seg_stride), "ip_attention: empty problem, or rows outside their batch row");
  DK_REQUIRE(h > 0 && h % 128 == 0 && h <= (1 << 20), "ip_attention: hidden size must be a whole number of 128-column heads");
  DK_REQUIRE(ldq >= h && ldq % 8 == 0 && ldkv >= h && ldkv % 8 == 0, "ip_attention: row pitches must hold h elements and keep 16-byte alignment");
  DK_REQUIRE((((uintptr_t)qkv | (uintptr_t)qn | (uintptr_t)K | (uintptr_t)V | (uintptr_t)out) & 15) == 0, "ip_attention: pointers must be 16-byte aligned");
  const long blocks = (long)B * ((seg_len + IP_ROWS - 1) / IP_ROWS);
  DK_REQUIRE(blocks < (1L << 31), "ip_attention: too many rows for one launch");
  IpAttnParams p;
  p.q = qkv + (size_t)first_row * ldq; p.qn = qn; p.K = K; p.V = V; p.out = out;
  p.ldq = ldq; p.seg_len = seg_len; p.seg_stride = seg_stride; p.ldkv = ldkv; p.h = h; p.scale = scale; p.eps = eps;
  const dim3 grid((unsigned)blocks, (unsigned)((h + 511) / 512)), block(256);
#define IP_CASE(n)                                                                         \
  case n:                                                                                  \
    hipLaunchKernelGGL(dk_ip_attention_kernel<n>, grid, block, 0, stream, p);              \
    break;
  switch (N) {
    IP_CASE(1) IP_CASE(2) IP_CASE(3) IP_CASE(4) IP_CASE(5) IP_CASE(6) IP_CASE(7) IP_CASE(8)
    IP_CASE(9) IP_CASE(10) IP_CASE(11) IP_CASE(12) IP_CASE(13) IP_CASE(14) IP_CASE(15) IP_CASE(16)
  }
#undef IP_CASE
  DK_CHECK_HIP(hipGetLastError());
  return 0;
}
