// Joint text/image attention forward, VALU-lean variant (dk_attn2_fwd_kernel).
//
// Same algorithm, layouts and MFMA operand mapping as dk_attn_fwd_kernel (attention.hip; reference
// call sites python/src/diffusionkit/mlx/mmdit.py:562,643,687,736) -- transposed scores S^T = K Q^T,
// lane-local online softmax, O^T += V^T P^T with V read through ds_read_b64_tr_b16 -- but the per-tile
// instruction stream is cut down, because rocprofv3 counters showed the first kernel VALU-bound
// (13 VALU per MFMA, VALU busy 59 %, MFMA busy 33 %; profiles/archive/r01_attention_pmc.md):
//   * K/V tile loads use ONE 32-bit lane offset per 16-byte chunk against a wave-uniform base that
//     advances per tile (global_load saddr form): no per-tile address arithmetic, the key clamp is
//     evaluated only in the tail tile;
//   * every LDS offset (swizzled K fragments, V transpose-read base, staging stores) is computed
//     once per kernel; the tile body only adds compile-time immediates (the loop is unrolled over
//     the two LDS buffers for that);
//   * the running-max rescale of O (64 multiplies) runs only when some query of the wave raised its
//     maximum by more than DK_RESCALE_THR (wave-uniform vote); probabilities are then bounded by
//     e^THR instead of 1, which fp32 accumulation and bf16 P tolerate (guide T13; the safe order is
//     kept: the decision precedes the exponentials of the tile it covers, nothing else is pending);
//   * the two 32-key score chains of a tile are interleaved (two independent accumulators).
//
// IDENT (identity attention, AttnParams::ident_from = F; D = 64; perturbed-attention guidance): a query s >= F sees the keys [0, F) and its
// own key only.  A template case of the same kernel: with IDENT false every addition below folds away.  A query block that lies wholly in the
// image range walks the ceil(F / 64) text tiles and then the (at most two) tiles of its own 128 rows (dk_ident_walk); a block with a text
// query walks every tile, so its text rows take the plain kernel's tiles in the plain kernel's order.  The element mask
// `query < F || key < F || key == query` is a select to -1e30 in front of the running maximum, in the tiles that hold a key >= F, for the
// waves that hold an image query; tiles wholly below F and waves wholly of text take the unmasked body.  The hazards:
//   * a fully masked tile.  A wave whose 32 queries see no key of a tile (wave-uniform: no text query, no text key, not the wave's own rows)
//     skips the tile's arithmetic, so (m, l, O) are untouched.  Inside a wave that does run, a lane may still find all its keys masked; its
//     scores are the finite -1e30, never -inf.  Every walk starts at tile 0, which holds key 0 < F, so every query's maximum is finite
//     before it meets a masked tile: mloc - m_run is then about -1e30, the lane never votes for the rescale, and its probabilities are
//     exp2(-1e30 c - m c) = 0 exactly -- l and O gain exact zeros.  No exp(-inf - (-inf)) can form;
//   * barriers.  The tile list, the loads, the LDS stores and the barriers depend on the query block alone (scalars): workgroup-uniform.
//     Only the arithmetic between them is skipped per wave;
//   * the ragged last key tile.  load_tile clamps the rows of whatever tile it is given exactly as before, and the tail mask `key >= S`
//     still follows the identity mask (a lane whose query lies beyond S must not unmask the key of the same index);
//   * the fused Q load (QFUSE) is in front of the tile loop and unchanged: it composes with IDENT as a second template flag.
//   * the launch's critical path.  A block with a text query is as long as a plain one: those blocks take the first workgroup ids.
// In the one wave that straddles F the text lanes share the deferred-rescale vote with image lanes whose maxima differ from the plain
// kernel's, so those (at most 31) text rows may rescale at other tiles than the plain launch does: equal to rounding, not bit for bit.
// Text rows of waves wholly below F are the plain kernel's bits.
#include "dk_kernels.h"

#define DK_RESCALE_THR 4.0f  // natural-log units of the scaled scores

template <int D, int NW>
struct Attn2Cfg {
  static constexpr int KV = 64;
  static constexpr int ROWB = D * 2;
  static constexpr int TILE_BYTES = KV * D * 2;
  static constexpr int NT = NW * 64;
  static constexpr int NCHUNK = KV * D / 8;                 // 16-byte chunks per K (or V) tile
  static constexpr int NCH = (NCHUNK + NT - 1) / NT;        // per thread (the last one may be partial: NW = 7)
  static constexpr bool RAGGED = (NCHUNK % NT) != 0;
  static constexpr int CPR = D / 8;
  static constexpr int QB = NW * 32;
  static constexpr int LDS_BYTES = 4 * TILE_BYTES;  // K[2] V[2]
};

template <int D>
__device__ __forceinline__ int k2_swz(int r) { return D == 128 ? (r & 15) : ((r >> 1) & 7); }

typedef __attribute__((address_space(3))) char lds_char;

template <int D, int NW, bool HAS_BIAS = false, bool QFUSE = false, bool IDENT = false>
__global__ __launch_bounds__(NW * 64, 2) void dk_attn2_fwd_kernel(AttnParams p) {
  using C = Attn2Cfg<D, NW>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // The dynamic LDS region starts at LDS address 0 (this kernel has no static __shared__ objects), so
  // LDS accesses are formed from small integer addresses: hipcc then knows the address bits and
  // folds every compile-time offset into the ds instruction's immediate field instead of emitting a
  // v_add per access (it cannot prove base + offset stays non-negative for a symbol address).
  if ((unsigned)(size_t)(lds_char*)smem != 0u) __builtin_trap();
  lds_char* const lds = (lds_char*)0;
  constexpr int K_OFF = 0, V_OFF = 2 * C::TILE_BYTES;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  const int S = p.S;

  const int nq = (S + C::QB - 1) / C::QB;
  int t;
  {
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  int qb = t % nq, head = (t / nq) % p.H, b = t / (nq * p.H);
  if (IDENT) {
    // The query blocks that hold a text query walk every tile, the others five or so: the long ones are the launch's critical path, so they take
    // the first workgroup ids (dispatched first, in plain blockIdx order: round-robin over the XCDs) and the short ones fill in behind them
    const int n_long = min((p.ident_from + C::QB - 1) / C::QB, nq), bid = blockIdx.x, first = n_long * p.H * p.B;
    int bh;
    if (bid < first) qb = bid % n_long, bh = bid / n_long;
    else qb = n_long + (bid - first) % (nq - n_long), bh = (bid - first) / (nq - n_long);
    head = bh % p.H, b = bh / p.H;
  }
  const int q0 = qb * C::QB + wave * 32;

  const bf16_t* Qb = p.Q + (size_t)b * S * p.ld + head * D;
  const char* Kb = (const char*)(p.K + (size_t)b * S * p.ld + head * D);  // wave-uniform bases
  const char* Vb = (const char*)(p.V + (size_t)b * S * p.ld + head * D);
  const unsigned row_bytes = (unsigned)p.ld * 2u;

  // Q fragments (B operand of S^T = K Q^T): lane holds Q[q0 + l31][kk*16 + hi*8 .. +7]
  ex8 qf[D / 16];
  {
    const int qrow = min(q0 + l31, S - 1);
    const bf16_t* qp = Qb + (size_t)qrow * p.ld + hi * 8;
#pragma unroll
    for (int kk = 0; kk < D / 16; ++kk) qf[kk] = *(const ex8*)(qp + kk * 16);
    if (QFUSE) {
      // QKNorm + RoPE of this lane's query row on the fly (same fp32 arithmetic and bf16 rounding points as
      // dk_qk_norm_rope_kernel): the lane and its partner (lane ^ 32) hold the two halves of every 16-element group
      float v[D / 16][8];
#pragma unroll
      for (int kk = 0; kk < D / 16; ++kk)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[kk][e] = (float)qf[kk][e];
      if (p.qn_a != nullptr) {
        float ss = 0.f;
#pragma unroll
        for (int kk = 0; kk < D / 16; ++kk)
#pragma unroll
          for (int e = 0; e < 8; ++e) ss += v[kk][e] * v[kk][e];
        ss += __shfl_xor(ss, 32, 64);
        const float r = rsqrtf(ss / (float)D + p.qn_eps);
        const bf16_t* w = (qrow < p.qn_split ? p.qn_a : p.qn_b) + hi * 8;
#pragma unroll
        for (int kk = 0; kk < D / 16; ++kk) {
          const ex8 wv = *(const ex8*)(w + kk * 16);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[kk][e] = round_act(v[kk][e] * r * (float)wv[e]);
        }
      }
      if (p.q_rope != nullptr) {
        const float* tab = p.q_rope + ((size_t)qrow * (D / 2) + hi * 4) * 2;
#pragma unroll
        for (int kk = 0; kk < D / 16; ++kk) {
          const f32x4 t0 = *(const f32x4*)(tab + kk * 16), t1 = *(const f32x4*)(tab + kk * 16 + 4);
          const float cs[8] = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float c = cs[2 * i], sn = cs[2 * i + 1], xe = v[kk][2 * i], xo = v[kk][2 * i + 1];
            v[kk][2 * i] = c * xe - sn * xo;
            v[kk][2 * i + 1] = sn * xe + c * xo;
          }
        }
      }
#pragma unroll
      for (int kk = 0; kk < D / 16; ++kk)
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[kk][e] = (elem_s)v[kk][e];
    }
  }

  // ---- per-thread constants: staging chunk coordinates, global lane offsets, LDS offsets ----
  bool st_on[C::NCH];       // chunk exists (NT does not divide the chunk count for 7-wave workgroups)
  unsigned g_off[C::NCH];   // byte offset of chunk i inside a 64-key tile (key-local row, 16-byte column)
  unsigned ks_off[C::NCH];  // LDS store offset inside a K tile
  unsigned vs_off[C::NCH];  // LDS store offset inside a V tile
  int st_kl[C::NCH];
#pragma unroll
  for (int i = 0; i < C::NCH; ++i) {
    const int id0 = tid + C::NT * i;
    st_on[i] = !C::RAGGED || id0 < C::NCHUNK;
    const int id = st_on[i] ? id0 : 0;
    const int kl = id / C::CPR, c8 = id % C::CPR;
    st_kl[i] = kl;
    g_off[i] = (unsigned)kl * row_bytes + (unsigned)c8 * 16u;
    ks_off[i] = (unsigned)(kl * C::ROWB + ((c8 ^ k2_swz<D>(kl)) << 4));
    // V image: [d/16][key][16]; d-block b stores key row kl at row kl ^ f(b), f(b) = ((b & 1) << 2) | (b & 3): bit 2 puts the
    // two blocks a tr-read touches on different bank halves, bits 0-1 spread the four blocks one staging store writes
    // (same key, 2 KiB apart = the same banks) over the four 32-byte rows of a 128-byte bank period (it was a 4-way conflict)
    vs_off[i] = (unsigned)((c8 >> 1) * 2048 + (kl ^ ((((c8 >> 1) & 1) << 2) | ((c8 >> 1) & 3))) * 32 + (c8 & 1) * 16);
  }
  unsigned kr_off[D / 16];  // K fragment read: row l31 (+32 per sub-tile as an immediate), swizzled chunk
#pragma unroll
  for (int kk = 0; kk < D / 16; ++kk) kr_off[kk] = (unsigned)(l31 * C::ROWB + (((kk * 2 + hi) ^ k2_swz<D>(l31)) << 4));
  const int x16 = (lane >> 4) & 1, p16 = lane & 15;
  unsigned vr_off[2];  // by parity of the 32-wide d-tile dt: the lane reads block b = 2*dt + x16, f(b) & 3 = 2*(dt & 1) + x16
#pragma unroll
  for (int par = 0; par < 2; ++par)
    vr_off[par] = (unsigned)(x16 * 2048 + ((4 * (hi ^ x16) + (p16 >> 2)) ^ (2 * par + x16)) * 32 + (p16 & 3) * 8);

  u32x4 kreg[C::NCH], vreg[C::NCH];
  const int ntiles = (S + 63) / 64;
  // IDENT: the tiles this workgroup walks (dk_ident_walk, dk_kernels.h), chosen per query block from scalars alone; step i of nsteps is tile
  // tile_of(i).  Otherwise step i is tile i of ntiles
  const int F = IDENT ? p.ident_from : 0;
  const IdentWalk walk = IDENT ? dk_ident_walk(qb * C::QB, S, F) : IdentWalk{ntiles, ntiles, 0};
  const int nsteps = IDENT ? walk.n_lo + walk.n_hi : ntiles;
  const int n_lo = walk.n_lo, hi_d = walk.hi0 - walk.n_lo;
  auto tile_of = [&](int i) { return IDENT && i >= n_lo ? i + hi_d : i; };
  // (IDENT) per wave, in tiles: the wave computes the tiles below n_act (all of them when it holds a text query, else those with a text key)
  // and tile j_own, which holds its 32 rows; it masks from tile f_mask on (never, when it holds no image query).  Per lane: the query,
  // unclamped (a lane beyond S owns no key), and the first key index it does not see unless it is its own (a text query sees all)
  const int n_act = q0 < F ? 0x7fffffff : (F + 63) / 64, j_own = q0 >> 6;
  const int f_mask = q0 + 32 > F ? F / 64 : 0x7fffffff;
  const int qself = q0 + l31, qlim = qself < F ? 0x7fffffff : F;
  auto load_tile = [&](int j) {
    const char* kb = Kb + (size_t)j * 64 * row_bytes;
    const char* vb = Vb + (size_t)j * 64 * row_bytes;
    if (j * 64 + 64 <= S) {
#pragma unroll
      for (int i = 0; i < C::NCH; ++i) {
        if (C::RAGGED && !st_on[i]) continue;
        kreg[i] = *(const u32x4*)(kb + g_off[i]);
        vreg[i] = *(const u32x4*)(vb + g_off[i]);
      }
    } else {  // tail tile: rows beyond S - 1 re-read the last key (their scores are masked below)
#pragma unroll
      for (int i = 0; i < C::NCH; ++i) {
        if (C::RAGGED && !st_on[i]) continue;
        const int kl = min(st_kl[i], S - 1 - j * 64);
        const unsigned off = (unsigned)kl * row_bytes + (g_off[i] - (unsigned)st_kl[i] * row_bytes);
        kreg[i] = *(const u32x4*)(kb + off);
        vreg[i] = *(const u32x4*)(vb + off);
      }
    }
  };
#define DK2_STORE_TILE(BUF)                                                            \
  _Pragma("unroll") for (int i = 0; i < C::NCH; ++i) {                                 \
    if (C::RAGGED && !st_on[i]) continue;                                              \
    *(__attribute__((address_space(3))) u32x4*)(lds + K_OFF + (BUF) * C::TILE_BYTES + ks_off[i]) = kreg[i]; \
    *(__attribute__((address_space(3))) u32x4*)(lds + V_OFF + (BUF) * C::TILE_BYTES + vs_off[i]) = vreg[i]; \
  }

  f32x16 o[D / 32];
#pragma unroll
  for (int i = 0; i < D / 32; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[i][e] = 0.f;
  float m_run = -1e30f, l_run = 0.f;
  const float c = p.scale * 1.44269504088896340736f;  // p = 2^(s*c - m*c)
  const float thr = DK_RESCALE_THR / p.scale;          // threshold on the raw scores
  const float inv_scale = 1.0f / p.scale;
  const bf16_t* bias_row = HAS_BIAS ? p.bias + (size_t)head * p.bias_head_stride + (size_t)min(q0 + l31, S - 1) * p.ldb : nullptr;

  load_tile(0);  // (IDENT: tile 0 holds key 0 < F, so it is the first tile of every walk)
  DK2_STORE_TILE(0)
  __syncthreads();

#define DK2_TILE(BUF, I)                                                                                   \
  do {                                                                                                     \
    const int i_ = (I), j_ = tile_of(i_);                                                                  \
    if (i_ + 1 < nsteps) load_tile(tile_of(i_ + 1));                                                       \
    /* IDENT: a wave none of whose 32 queries sees a key of this tile -- no text query, no text key, not its own rows -- skips the tile's */ \
    /* arithmetic: (m, l, O) stay as they are.  It still takes the loads, the stores and the barrier, which are the workgroup's */ \
    if (!IDENT || j_ < n_act || j_ == j_own) {                                                             \
    f32x16 s0, s1;                                                                                         \
    _Pragma("unroll") for (int e = 0; e < 16; ++e) { s0[e] = 0.f; s1[e] = 0.f; }                           \
    __builtin_amdgcn_s_setprio(1);                                                                         \
    _Pragma("unroll") for (int kk = 0; kk < D / 16; ++kk) {                                                \
      const ex8 k0 = *(const __attribute__((address_space(3))) ex8*)(lds + K_OFF + (BUF) * C::TILE_BYTES + kr_off[kk]); \
      const ex8 k1 = *(const __attribute__((address_space(3))) ex8*)(lds + K_OFF + (BUF) * C::TILE_BYTES + 32 * C::ROWB + kr_off[kk]); \
      s0 = mfma_32x32x16(k0, qf[kk], s0);                               \
      s1 = mfma_32x32x16(k1, qf[kk], s1);                               \
    }                                                                                                      \
    __builtin_amdgcn_s_setprio(0);                                                                         \
    if (IDENT && j_ >= f_mask) { /* a tile with keys >= F, a wave with image queries */                    \
      asm volatile("; identity mask" ::: "memory");                                                        \
      _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                     \
        const int key = j_ * 64 + (e & 3) + 8 * (e >> 2) + 4 * hi;                                         \
        if (!(key < qlim || key == qself)) s0[e] = -1e30f;                                                 \
        if (!(key + 32 < qlim || key + 32 == qself)) s1[e] = -1e30f;                                       \
        /* (every compare leaves a lane mask in a scalar pair: keep the scheduler from gathering all 64 in front of the selects) */ \
        if ((e & 3) == 3) __builtin_amdgcn_sched_barrier(0);                                               \
      }                                                                                                    \
    }                                                                                                      \
    if (!HAS_BIAS && j_ * 64 + 64 > S) {                                                                   \
      asm volatile("; tail tile" ::: "memory"); /* keeps hipcc from if-converting the mask into every tile */ \
      _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                     \
        const int key = j_ * 64 + (e & 3) + 8 * (e >> 2) + 4 * hi;                                         \
        if (key >= S) s0[e] = -1e30f;                                                                      \
        if (key + 32 >= S) s1[e] = -1e30f;                                                                 \
      }                                                                                                    \
    }                                                                                                      \
    if (HAS_BIAS) { /* scores += bias / scale (the exponent below multiplies by scale * log2 e) */            \
      _Pragma("unroll") for (int g4 = 0; g4 < 4; ++g4) {                                                   \
        const uint2 b0 = *(const uint2*)(bias_row + j_ * 64 + 8 * g4 + 4 * hi);                             \
        const uint2 b1 = *(const uint2*)(bias_row + j_ * 64 + 32 + 8 * g4 + 4 * hi);                        \
        float f0[4], f1[4];                                                                                \
        unpack2(b0.x, f0[0], f0[1]); unpack2(b0.y, f0[2], f0[3]);                                      \
        unpack2(b1.x, f1[0], f1[1]); unpack2(b1.y, f1[2], f1[3]);                                      \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                    \
          s0[4 * g4 + e] += f0[e] * inv_scale;                                                             \
          s1[4 * g4 + e] += f1[e] * inv_scale;                                                             \
        }                                                                                                  \
      }                                                                                                    \
    }                                                                                                      \
    if (HAS_BIAS) { /* the mask comes AFTER the bias, as a select: whatever the pad columns S..ldb of a bias row hold never reaches a score */\
      _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                     \
        const int key = j_ * 64 + (e & 3) + 8 * (e >> 2) + 4 * hi;                                         \
        s0[e] = key >= S ? -1e30f : s0[e];                                                                 \
        s1[e] = key + 32 >= S ? -1e30f : s1[e];                                                            \
      }                                                                                                    \
    }                                                                                                      \
    float mloc = fmaxf(s0[0], s1[0]);                                                                      \
    _Pragma("unroll") for (int e = 1; e < 16; ++e) mloc = fmaxf(mloc, fmaxf(s0[e], s1[e]));                \
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));                                                          \
    if (!__all(mloc - m_run <= thr)) {                                                                     \
      const float m_new = fmaxf(m_run, mloc);                                                              \
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);                                     \
      m_run = m_new;                                                                                       \
      l_run *= alpha;                                                                                      \
      _Pragma("unroll") for (int i = 0; i < D / 32; ++i) _Pragma("unroll") for (int e = 0; e < 16; ++e) o[i][e] *= alpha; \
    }                                                                                                      \
    const float mc = m_run * c;                                                                            \
    float psum = 0.f;                                                                                      \
    _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                       \
      s0[e] = __builtin_amdgcn_exp2f(s0[e] * c - mc);                                                      \
      s1[e] = __builtin_amdgcn_exp2f(s1[e] * c - mc);                                                      \
      psum += s0[e] + s1[e];                                                                               \
    }                                                                                                      \
    l_run += psum;                                                                                         \
    __builtin_amdgcn_s_setprio(1);                                                                         \
    _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                                        \
      _Pragma("unroll") for (int tt = 0; tt < 2; ++tt) {                                                   \
        ex8 pf;                                                                                         \
        _Pragma("unroll") for (int e = 0; e < 8; ++e) pf[e] = (elem_s)(u == 0 ? s0[8 * tt + e] : s1[8 * tt + e]); \
        _Pragma("unroll") for (int dt = 0; dt < D / 32; ++dt) {                                            \
          const int imm = V_OFF + (BUF) * C::TILE_BYTES + dt * 4096 + (32 * u + 16 * tt) * 32;             \
          const s16x4 vh0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lds + imm + vr_off[dt & 1])); \
          const s16x4 vh1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lds + imm + 256 + vr_off[dt & 1])); \
          const ex8 vf = __builtin_bit_cast(ex8, __builtin_shufflevector(vh0, vh1, 0, 1, 2, 3, 4, 5, 6, 7)); \
          o[dt] = mfma_32x32x16(vf, pf, o[dt]);                         \
        }                                                                                                  \
      }                                                                                                    \
    }                                                                                                      \
    __builtin_amdgcn_s_setprio(0);                                                                         \
    }                                                                                                      \
    if (i_ + 1 < nsteps) { DK2_STORE_TILE((BUF) ^ 1) }                                                     \
    __syncthreads();                                                                                       \
  } while (0)

  int j = 0;
  for (; j + 1 < nsteps; j += 2) {
    DK2_TILE(0, j);
    DK2_TILE(1, j + 1);
  }
  if (j < nsteps) DK2_TILE(0, j);
#undef DK2_TILE
#undef DK2_STORE_TILE

  // ---- normalise and store: lane owns query q0+l31, d = dt*32 + 8g + 4hi + {0..3} ----
  const float lsum = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = 1.0f / lsum;
  const int q = q0 + l31;
  if (q < S) {
    bf16_t* op = p.O + ((size_t)b * S + q) * p.ldo + head * D;
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        uint2 w;
        w.x = pack2(o[dt][4 * g4 + 0] * inv, o[dt][4 * g4 + 1] * inv);
        w.y = pack2(o[dt][4 * g4 + 2] * inv, o[dt][4 * g4 + 3] * inv);
        *(uint2*)(op + dt * 32 + 8 * g4 + 4 * hi) = w;
      }
  }
}

template <int D, int NW, bool HAS_BIAS = false, bool QFUSE = false, bool IDENT = false>
static int launch_attn2(const AttnParams& p, hipStream_t stream) {
  using C = Attn2Cfg<D, NW>;
  static DkDeviceOnce attr_once;
  if (attr_once.first()) {
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_attn2_fwd_kernel<D, NW, HAS_BIAS, QFUSE, IDENT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     C::LDS_BYTES));
    attr_once.mark();
  }
  const int nq = (p.S + C::QB - 1) / C::QB;
  hipLaunchKernelGGL((dk_attn2_fwd_kernel<D, NW, HAS_BIAS, QFUSE, IDENT>), dim3(nq * p.H * p.B), dim3(C::NT), C::LDS_BYTES, stream, p);
  return 0;
}

#ifdef DK_ATTN2_DEFAULT_SCHED_TU
// attention2p.hip: this file compiled a second time, under LLVM's default machine scheduler, for the D = 128 instantiations -- the
// iterative-ilp strategy the D = 64 kernels are built under (Makefile) drives them into spills (5 registers with the fused query norm).
// (Round 4 lab, profiles/lab_kernels/attention2_pipelined.patch: a D = 64 form with the next tile's score MFMAs and this tile's P.V
// MFMAs interleaved with the exponentials by a sched_group_barrier pipeline -- parity-green, 200 registers = 2 waves per SIMD,
// 6 % SLOWER than the lean form on the SD3 shapes, profiles/r04_attention_d64_pipelined.log; not built.)
int dk_launch_attention2_d128(const AttnParams& p, hipStream_t stream) {  // (arguments checked by dk_attention_route)
  if (p.bias != nullptr) return launch_attn2<128, 4, true>(p, stream);
  if (p.qn_a != nullptr || p.q_rope != nullptr) return launch_attn2<128, 4, false, true>(p, stream);
  return launch_attn2<128, 4>(p, stream);
}
#elif defined(DK_ELEM_F16)
// attention2_f16.hip: this file compiled inside namespace dk_f16 -- the D = 64 forms on IEEE-half operands (scores, running maximum and sum in
// fp32 as before; P rounded to fp16 for the P.V MFMA: P <= e^DK_RESCALE_THR under the deferred rescale, far inside fp16's range)
int dk_launch_attention2(const AttnParams& p, int waves, hipStream_t stream) {  // (arguments checked by dk_attention_route)
  DK_REQUIRE(p.D == 64 && p.bias == nullptr && p.O8 == nullptr && waves == 4, "attention2 (fp16): head_dim 64, no score bias, no MX-fp8 copy");
  if (p.ident_from != 0)
    return p.qn_a != nullptr || p.q_rope != nullptr ? launch_attn2<64, 4, false, true, true>(p, stream) : launch_attn2<64, 4, false, false, true>(p, stream);
  if (p.qn_a != nullptr || p.q_rope != nullptr) return launch_attn2<64, 4, false, true>(p, stream);
  return launch_attn2<64, 4>(p, stream);
}
#else
int dk_launch_attention2_d128(const AttnParams& p, hipStream_t stream);  // attention2p.hip
int dk_launch_attention2(const AttnParams& p, int waves, hipStream_t stream) {  // (arguments checked by dk_attention_route)
  if (p.dtype == DK_DTYPE_F16) return dk_f16::dk_launch_attention2(p, waves, stream);
  DK_REQUIRE(waves == 4, "attention2: 4 waves per workgroup (the 8- and 7-wave forms were pruned in round 3)");
  if (p.ident_from != 0) {  // identity attention: D = 64, no score bias (dk_attention_route)
    DK_REQUIRE(p.D == 64 && p.bias == nullptr, "attention2 (identity): head_dim 64, no score bias");
    return p.qn_a != nullptr || p.q_rope != nullptr ? launch_attn2<64, 4, false, true, true>(p, stream) : launch_attn2<64, 4, false, false, true>(p, stream);
  }
  if (p.bias != nullptr)  // text encoders: D = 64, short sequences
    return p.D == 128 ? dk_launch_attention2_d128(p, stream) : launch_attn2<64, 4, true>(p, stream);
  if (p.qn_a != nullptr || p.q_rope != nullptr)  // query-side QKNorm / RoPE fused into the Q load (MMDiT call sites)
    return p.D == 128 ? dk_launch_attention2_d128(p, stream) : launch_attn2<64, 4, false, true>(p, stream);
  return p.D == 128 ? dk_launch_attention2_d128(p, stream) : launch_attn2<64, 4>(p, stream);
}
#endif
