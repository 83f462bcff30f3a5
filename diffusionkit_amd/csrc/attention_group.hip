// Group-masked joint attention forward (dk_attng_fwd_kernel), D = 128, bf16: regional prompts for the FLUX geometry.
//
// The mask is one 32-bit word per token of the joint [text | image] sequence (AttnParams::groups, [B, S], every word non-zero): query i sees key j iff
// their words share a bit.  No [S, S] table exists anywhere: a (query, key) pair costs one AND of two registers, and only where a tile needs it.
//
// Work split.  One workgroup per (batch row, head, block of 128 queries), four waves of 32 queries; 64-key tiles.  The MFMA operand mapping is
// attention4.hip's (transposed scores S^T = K Q^T on v_mfma_f32_32x32x16_bf16, so a lane owns ONE query and its softmax is lane-local; O^T += V^T P^T
// with V through ds_read_b64_tr_b16; the same swizzled K / V tile layouts in LDS), but none of its phase scheme: the loop here is
//   global loads of the NEXT VISITED tile into registers | barrier | this tile's arithmetic from LDS slot s | LDS stores into slot s ^ 1
// one barrier per tile, K[2] V[2] + the tiles' 64 group words [2] in LDS.  The walk is irregular (tiles are skipped), which is what the hand-scheduled
// bodies cannot take; this one is left to the compiler's scheduler.
//
// Tile classes.  The per-tile OR / AND of the key words are reduced BY THE KERNEL ITSELF in its prologue (each wave reads a quarter of the batch row's
// words, coalesced, and folds 64 of them with six butterfly steps; S * 4 bytes per workgroup out of L2: 22 KB at FLUX's 1024^2 shape with three prompts,
// about a tile's worth of time against 88 tiles).  A pre-pass kernel would save that but needs a workspace the stand-alone operator and the engine's
// carve do not have, a second launch per attention, and an ordering promise between the two; the words are read once per launch either way.
//   * block level: a tile none of the block's 128 queries shares a bit with (or_block & or_tile == 0) is not visited: no load, no barrier, no MFMA;
//   * wave level, per visited tile: or_wave & or_tile == 0: the wave skips the arithmetic (it still stores its share of the next tile and meets the
//     barrier); and_wave & and_tile != 0: every pair is allowed, the unmasked body; otherwise mixed.
//   * mixed: a disallowed score becomes -inf by a select in front of the running maximum (a NaN score of a key the query may not see is discarded, not
//     multiplied), so its probability is exp2(-inf) = 0 exactly.  A zero probability is not enough for P.V: the matrix product would still form
//     0 * V, and V of a key this query may not see must not reach it (0 * NaN).  So the P.V of a mixed tile runs once per DISTINCT query word of the
//     wave: the V fragments with the keys that word may not see cleared to zero bits, the probabilities of the other words' lanes cleared, into a
//     fresh accumulator that only that word's lanes add.  A wave inside one region (the common case) has one word and accumulates directly.
//     A wave across a box edge has two or three.  The cost grows with the number of distinct words in 32 consecutive tokens; recorded, not bounded.
//
// The running maximum starts at -inf and may stay there while a row's first visited tiles hold no allowed key for it (they are visited for other rows
// of the block).  No finite stand-in that a real score could undercut: the two places where -inf - (-inf) could form are guarded by selects --
// the rescale factor of a row without a maximum is 0 (its l and O are exact zeros), and the offset of such a row is 0, so exp2(-inf - 0) = 0.
//
// Ragged S: keys beyond S carry the word 0 (never allowed: the last tile is mixed, its rows re-read the last key like attention4.hip's), queries beyond S
// carry 0 too (nothing allowed, never stored).  Launch: skipped tiles make the blocks uneven (a text block of one region walks its own tiles and its box,
// an image block everything it shares a bit with); the grid is not balanced and the keys are not split.
#include "dk_kernels.h"

#define DKG_RESCALE_THR 4.0f  // natural-log units of the scaled scores (the deferred rescale of the other kernels)

struct AttnGCfg {
  static constexpr int D = 128, NW = 4;
  static constexpr int KV = 64;
  static constexpr int ROWB = D * 2;
  static constexpr int TILE_BYTES = KV * D * 2;
  static constexpr int NT = NW * 64;
  static constexpr int NCH = KV * D / 8 / NT;  // 16-byte chunks of a K (or V) tile per thread
  static constexpr int CPR = D / 8;
  static constexpr int QB = NW * 32;
  static constexpr int MAX_TILES = 1024;  // S <= 65536
  static constexpr int K_OFF = 0, V_OFF = 2 * TILE_BYTES, GK_OFF = 4 * TILE_BYTES, OR_OFF = GK_OFF + 2 * KV * 4, AND_OFF = OR_OFF + MAX_TILES * 4,
                       BLK_OFF = AND_OFF + MAX_TILES * 4;
  static constexpr int LDS_BYTES = BLK_OFF + NW * 4;
};

typedef __attribute__((address_space(3))) char lds_charg;

__device__ __forceinline__ unsigned dkg_wave_or(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned dkg_wave_and(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v &= (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}

template <bool QFUSE>
__global__ __launch_bounds__(256) void dk_attng_fwd_kernel(AttnParams p) {
  using C = AttnGCfg;
  constexpr int D = C::D;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  lds_charg* const lds = (lds_charg*)smem;
  __attribute__((address_space(3))) unsigned* const t_or = (__attribute__((address_space(3))) unsigned*)(lds + C::OR_OFF);
  __attribute__((address_space(3))) unsigned* const t_and = (__attribute__((address_space(3))) unsigned*)(lds + C::AND_OFF);
  __attribute__((address_space(3))) unsigned* const blk = (__attribute__((address_space(3))) unsigned*)(lds + C::BLK_OFF);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, l31 = lane & 31;
  const int S = p.S;
  const int nq = (S + C::QB - 1) / C::QB, nt = (S + C::KV - 1) / C::KV;
  int t;
  {  // consecutive tasks (query blocks of one head: the same K / V) on one XCD, as attention4.hip
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  }
  const int qb = t % nq, head = (t / nq) % p.H, b = t / (nq * p.H);
  const int q0 = qb * C::QB + wave * 32;
  const unsigned row_bytes = (unsigned)p.ld * 2u;
  const uint32_t* const G = p.groups + (size_t)b * S;

  // ---- the tiles' OR / AND words, the wave's and the block's ----
  for (int j = wave; j < nt; j += C::NW) {
    const int key = j * C::KV + lane;
    const unsigned w = key < S ? G[key] : 0u;
    const unsigned o = dkg_wave_or(w), a = dkg_wave_and(w);  // (a ragged tile's AND is 0: mixed)
    if (lane == 0) t_or[j] = o, t_and[j] = a;
  }
  const unsigned gq = q0 + l31 < S ? G[q0 + l31] : 0u;  // this lane's query word (both halves of the wave hold the same 32 queries)
  const unsigned wq_or = (unsigned)__builtin_amdgcn_readfirstlane((int)dkg_wave_or(gq));
  const unsigned wq_and = (unsigned)__builtin_amdgcn_readfirstlane((int)dkg_wave_and(q0 + l31 < S ? gq : ~0u));
  if (lane == 0) blk[wave] = wq_or;

  // ---- per-thread staging coordinates and LDS offsets (attention4.hip's tile layouts) ----
  unsigned g_row[C::NCH], g_col[C::NCH], ks_off[C::NCH], vs_off[C::NCH];
#pragma unroll
  for (int i = 0; i < C::NCH; ++i) {
    const int id = tid + C::NT * i;
    const int kl = id / C::CPR, c8 = id % C::CPR;
    g_row[i] = (unsigned)kl;
    g_col[i] = (unsigned)c8 * 16u;
    ks_off[i] = (unsigned)(kl * C::ROWB + ((c8 ^ (kl & 15)) << 4));
    vs_off[i] = (unsigned)((c8 >> 1) * 2048 + (kl ^ ((((c8 >> 1) & 1) << 2) | ((c8 >> 1) & 3))) * 32 + (c8 & 1) * 16);
  }
  const unsigned kr_base = (unsigned)(l31 * C::ROWB + ((hi ^ (l31 & 15)) << 4));
  const int x16 = (lane >> 4) & 1, p16 = lane & 15;
  unsigned vr_off[2];
#pragma unroll
  for (int par = 0; par < 2; ++par)
    vr_off[par] = (unsigned)(x16 * 2048 + ((4 * (hi ^ x16) + (p16 >> 2)) ^ (2 * par + x16)) * 32 + (p16 & 3) * 8);

  const bf16_t* Qb = p.Q + (size_t)b * S * p.ld + head * D;
  const char* Kb = (const char*)(p.K + (size_t)b * S * p.ld + head * D);
  const char* Vb = (const char*)(p.V + (size_t)b * S * p.ld + head * D);

  u32x4 kreg[C::NCH], vreg[C::NCH];
  unsigned gkreg = 0u;
  // tile jt -> registers; rows beyond S - 1 re-read the last key (their word is 0: never allowed)
  auto load_tile = [&](int jt) {
    const int last = S - 1 - jt * C::KV;
    const size_t base = (size_t)jt * C::KV * row_bytes;
#pragma unroll
    for (int i = 0; i < C::NCH; ++i) {
      const size_t off = base + (size_t)(unsigned)min((int)g_row[i], last) * row_bytes + g_col[i];
      kreg[i] = *(const u32x4*)(Kb + off);
      vreg[i] = *(const u32x4*)(Vb + off);
    }
    if (tid < C::KV) gkreg = jt * C::KV + tid < S ? G[jt * C::KV + tid] : 0u;
  };
  auto store_tile = [&](int slot) {
#pragma unroll
    for (int i = 0; i < C::NCH; ++i) {
      *(__attribute__((address_space(3))) u32x4*)(lds + C::K_OFF + slot * C::TILE_BYTES + ks_off[i]) = kreg[i];
      *(__attribute__((address_space(3))) u32x4*)(lds + C::V_OFF + slot * C::TILE_BYTES + vs_off[i]) = vreg[i];
    }
    if (tid < C::KV) *(__attribute__((address_space(3))) unsigned*)(lds + C::GK_OFF + slot * C::KV * 4 + tid * 4) = gkreg;
  };

  // ---- Q fragments (B operand of S^T = K Q^T): lane holds Q[q0 + l31][kk*16 + hi*8 .. +7]; the fused load is attention4.hip's arithmetic ----
  bf16x8 qf[D / 16];
  {
    const int qrow = min(q0 + l31, S - 1);
    const bf16_t* qp = Qb + (size_t)qrow * p.ld + hi * 8;
#pragma unroll
    for (int kk = 0; kk < D / 16; ++kk) qf[kk] = *(const bf16x8*)(qp + kk * 16);
    if (QFUSE) {
      bf16x8 wv[D / 16];
      f32x4 t0[D / 16], t1[D / 16];
      if (p.qn_a != nullptr) {
        const bf16_t* w = (qrow < p.qn_split ? p.qn_a : p.qn_b) + hi * 8;
#pragma unroll
        for (int kk = 0; kk < D / 16; ++kk) wv[kk] = *(const bf16x8*)(w + kk * 16);
      }
      if (p.q_rope != nullptr) {
        const float* tab = p.q_rope + ((size_t)qrow * (D / 2) + hi * 4) * 2;
#pragma unroll
        for (int kk = 0; kk < D / 16; ++kk) t0[kk] = *(const f32x4*)(tab + kk * 16), t1[kk] = *(const f32x4*)(tab + kk * 16 + 4);
      }
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
#pragma unroll
        for (int kk = 0; kk < D / 16; ++kk)
#pragma unroll
          for (int e = 0; e < 8; ++e) v[kk][e] = round_bf16(v[kk][e] * r * (float)wv[kk][e]);
      }
      if (p.q_rope != nullptr) {
#pragma unroll
        for (int kk = 0; kk < D / 16; ++kk) {
          const float cs[8] = {t0[kk][0], t0[kk][1], t0[kk][2], t0[kk][3], t1[kk][0], t1[kk][1], t1[kk][2], t1[kk][3]};
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
        for (int e = 0; e < 8; ++e) qf[kk][e] = (__bf16)v[kk][e];
    }
  }

  __syncthreads();  // t_or / t_and / blk are written
  const unsigned or_blk = blk[0] | blk[1] | blk[2] | blk[3];
  // the next tile at or behind j that the block visits (nt: none); the same for every thread
  auto next_tile = [&](int j) {
    while (j < nt && (t_or[j] & or_blk) == 0u) ++j;
    return __builtin_amdgcn_readfirstlane(j);
  };

  f32x16 o[D / 32];
#pragma unroll
  for (int i = 0; i < D / 32; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[i][e] = 0.f;
  const float NEG_INF = -__builtin_inff();
  float m_run = NEG_INF, l_run = 0.f;
  const float c = p.scale * 1.44269504088896340736f;  // p = 2^(s*c - m*c)
  const float thr = DKG_RESCALE_THR / p.scale;         // threshold on the raw scores

  // 16 MFMAs of O^T += V^T P^T against LDS slot `slot`; kmask != ~0: the V fragments keep only the keys whose bit is set.  Element j of a fragment
  // of 16-key step n in lane half hi is key 16 n + (j & 3) + 8 (j >> 2) + 4 hi: the order of the score accumulators, which P inherits
  auto pv = [&](f32x16* acc, const bf16x8* pw, int slot, bool clear, unsigned long long kmask) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      u32x4 km = {~0u, ~0u, ~0u, ~0u};
      if (clear) {
        const unsigned kb = (unsigned)(kmask >> (16 * n + 4 * hi));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int b0 = (r & 1) * 2 + (r >> 1) * 8;
          km[r] = ((0u - ((kb >> b0) & 1u)) & 0xFFFFu) | ((0u - ((kb >> (b0 + 1)) & 1u)) & 0xFFFF0000u);
        }
      }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const unsigned a = (unsigned)(C::V_OFF + slot * C::TILE_BYTES + dt * 4096 + 16 * n * 32) + vr_off[dt & 1];
        const s16x4 vh0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lds + a));
        const s16x4 vh1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lds + a + 256));
        u32x4 fr = __builtin_bit_cast(u32x4, __builtin_shufflevector(vh0, vh1, 0, 1, 2, 3, 4, 5, 6, 7));
        if (clear) fr &= km;
        acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fr), pw[n], acc[dt], 0, 0, 0);
      }
    }
  };

  int j = next_tile(0);
  int slot = 0;
  if (j < nt) {
    load_tile(j);
    store_tile(0);
  }
  while (j < nt) {
    const int jn = next_tile(j + 1);
    if (jn < nt) load_tile(jn);
    __syncthreads();  // slot `slot` is complete; every wave is past its reads of slot ^ 1
    const unsigned k_or = (unsigned)__builtin_amdgcn_readfirstlane((int)t_or[j]), k_and = (unsigned)__builtin_amdgcn_readfirstlane((int)t_and[j]);
    if ((wq_or & k_or) != 0u) {
      const bool full = (wq_and & k_and) != 0u;
      // ---- scores: s0 = keys 0..31 of the tile, s1 = keys 32..63; element e of a lane is key (e & 3) + 8 (e >> 2) + 4 hi ----
      f32x16 s0, s1;
#pragma unroll
      for (int e = 0; e < 16; ++e) s0[e] = 0.f, s1[e] = 0.f;
#pragma unroll
      for (int kk = 0; kk < D / 16; ++kk) {
        const unsigned a = (unsigned)(C::K_OFF + slot * C::TILE_BYTES) + (kr_base ^ (unsigned)(kk << 5));
        const bf16x8 f0 = *(const __attribute__((address_space(3))) bf16x8*)(lds + a);
        const bf16x8 f1 = *(const __attribute__((address_space(3))) bf16x8*)(lds + a + 32 * C::ROWB);
        s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f0, qf[kk], s0, 0, 0, 0);
        s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f1, qf[kk], s1, 0, 0, 0);
      }
      if (!full) {  // mixed: disallowed scores leave by a select (a NaN among them is dropped here)
        const lds_charg* gk = lds + C::GK_OFF + slot * C::KV * 4;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const u32x4 w0 = *(const __attribute__((address_space(3))) u32x4*)(gk + (8 * g + 4 * hi) * 4);
          const u32x4 w1 = *(const __attribute__((address_space(3))) u32x4*)(gk + (32 + 8 * g + 4 * hi) * 4);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            s0[4 * g + i] = (gq & w0[i]) != 0u ? s0[4 * g + i] : NEG_INF;
            s1[4 * g + i] = (gq & w1[i]) != 0u ? s1[4 * g + i] : NEG_INF;
          }
        }
      }
      // ---- online softmax, lane-local; the lane 32 away holds the other half of the row's keys ----
      float mx = fmaxf(s0[0], s1[0]);
#pragma unroll
      for (int e = 1; e < 16; ++e) mx = fmaxf(fmaxf(mx, s0[e]), s1[e]);
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      // (a row without a maximum so far: -inf - (-inf) is NaN, `> thr` false; with its first allowed key the difference is +inf)
      // The deferred rescale is decided PER ROW, not by a vote of the wave: a row's bits then depend on its own scores alone (the other lanes multiply
      // by exactly 1), which is what lets a NaN in a key that only a neighbour row may see leave this row bit for bit.
      const bool need = mx - m_run > thr;
      if (__any(need)) {
        const float m_new = need ? fmaxf(m_run, mx) : m_run;
        const float alpha = !need ? 1.f : m_run == NEG_INF ? 0.f : __builtin_amdgcn_exp2f((m_run - m_new) * c);
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int i = 0; i < D / 32; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) o[i][e] *= alpha;
      }
      const float mc = m_run == NEG_INF ? 0.f : m_run * c;
      float psum = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        s0[e] = __builtin_amdgcn_exp2f(s0[e] * c - mc);
        s1[e] = __builtin_amdgcn_exp2f(s1[e] * c - mc);
        psum += s0[e] + s1[e];
      }
      l_run += psum;
      bf16x8 pf[4];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        pf[0][e] = (__bf16)s0[e]; pf[1][e] = (__bf16)s0[8 + e]; pf[2][e] = (__bf16)s1[e]; pf[3][e] = (__bf16)s1[8 + e];
      }
      if (full) {
        pv(o, pf, slot, false, ~0ull);
      } else {
        // P.V once per distinct query word of the wave (file header)
        const unsigned gkl = *(const __attribute__((address_space(3))) unsigned*)(lds + C::GK_OFF + slot * C::KV * 4 + lane * 4);
        const unsigned long long todo0 = __ballot(gq != 0u);
        unsigned long long todo = todo0;
        while (todo != 0ull) {
          const int leader = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(todo));
          const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)gq, leader);
          const bool mine = gq == w;
          const unsigned long long mm = __ballot(mine);
          const unsigned long long kmask = __ballot((gkl & w) != 0u);
          if (mm == todo0) {
            pv(o, pf, slot, true, kmask);
          } else {
            bf16x8 pw[4];
            const bf16x8 zero8 = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
#pragma unroll
            for (int n = 0; n < 4; ++n) pw[n] = mine ? pf[n] : zero8;
            f32x16 tmp[D / 32];
#pragma unroll
            for (int i = 0; i < D / 32; ++i)
#pragma unroll
              for (int e = 0; e < 16; ++e) tmp[i][e] = 0.f;
            pv(tmp, pw, slot, true, kmask);
#pragma unroll
            for (int i = 0; i < D / 32; ++i)
#pragma unroll
              for (int e = 0; e < 16; ++e) o[i][e] = mine ? o[i][e] + tmp[i][e] : o[i][e];
          }
          todo &= ~mm;
        }
      }
    }
    if (jn < nt) store_tile(slot ^ 1);
    slot ^= 1;
    j = jn;
  }

  // ---- normalise and store: lane owns query q0 + l31, d = dt*32 + 8g + 4hi + {0..3} ----
  const float l = l_run + __shfl_xor(l_run, 32, 64);
  const float inv = l > 0.f ? 1.0f / l : 0.f;  // (l = 0: a row beyond S)
  const int q = q0 + l31;
  if (q < S) {
    bf16_t* op = p.O + ((size_t)b * S + q) * p.ldo + head * D;
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        uint2 w;
        w.x = pack2bf(o[dt][4 * g4 + 0] * inv, o[dt][4 * g4 + 1] * inv);
        w.y = pack2bf(o[dt][4 * g4 + 2] * inv, o[dt][4 * g4 + 3] * inv);
        *(uint2*)(op + dt * 32 + 8 * g4 + 4 * hi) = w;
      }
  }
}

template <bool QFUSE>
static int launch_attng(const AttnParams& p, hipStream_t stream) {
  using C = AttnGCfg;
  static DkDeviceOnce attr_once;
  if (attr_once.first()) {
    DK_CHECK_HIP(hipFuncSetAttribute((const void*)dk_attng_fwd_kernel<QFUSE>, hipFuncAttributeMaxDynamicSharedMemorySize, C::LDS_BYTES));
    attr_once.mark();
  }
  const long tasks = (long)((p.S + C::QB - 1) / C::QB) * p.H * p.B;
  hipLaunchKernelGGL((dk_attng_fwd_kernel<QFUSE>), dim3((unsigned)tasks), dim3(C::NT), C::LDS_BYTES, stream, p);
  return 0;
}

// the group-masked kernel (the argument checks that name a rule: dk_attention_route)
int dk_launch_attention_group(const AttnParams& p, hipStream_t stream) {
  DK_REQUIRE(p.groups != nullptr && p.D == 128 && p.dtype == DK_DTYPE_BF16 && p.bias == nullptr && p.O8 == nullptr, "group-masked attention: bf16, head_dim 128, no bias, no MX-fp8 copy");
  DK_REQUIRE(p.S <= AttnGCfg::MAX_TILES * AttnGCfg::KV, "group-masked attention: S <= 65536");
  const bool qfuse = p.qn_a != nullptr || p.q_rope != nullptr;
  return qfuse ? launch_attng<true>(p, stream) : launch_attng<false>(p, stream);
}
