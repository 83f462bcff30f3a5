// The tail the three 256 x 256 GEMM kernels share (gemm256v3.hip, gemm256v4.hip, gemm256f8.hip): round(alpha * acc + bias) is staged as a
// 16-bit image in wave-private 16 KiB LDS regions and read back 8 columns per lane, 16 rows per step, through the output, residual and gate
// row maps, with the epilogue folded at compile time -- one 16-byte store per lane and row (a lane takes 8 consecutive columns of one row, 4 lanes
// a 32-column row of the image: 8-byte stores are issue-bound, this is half as many instructions).  One text for all three, so that "gemm256v4
// equals gemm256v3 bit for bit" and "the fp8 kernel's tail equals the bf16 kernels'" hold by construction.
//
// No include guard and no includes of its own: like dk_elem_launchers.h this file is compiled at global scope, where round_act / pack2 /
// unpack2 are the bf16 helpers (gemm256v4.hip, gemm256f8.hip, gemm256v3.hip), and again inside namespace dk_f16 (gemm256v3_f16.hip includes
// gemm256v3.hip there), where they mean IEEE half.  The includer has dk_kernels.h.
//
// A kernel brings what is its own as compile-time parameters and small inlined functors, never as a run-time branch on the caller: where a
// pass's image lies (`pass_of`), where a key / query row's sum of squares comes from (`ss_of`), and how a finished row leaves (`store`,
// `store_raw`).

typedef __attribute__((address_space(3))) char dk_tail_lds;

// ---- staged image: 64-byte rows (32 columns), the 16-byte chunk c of a row at position c ^ ((row >> 2) & 3) -- conflict-free for the 8-byte
// staging writes (16 rows x one chunk per 16 lanes) and for the 16-byte read-back (4 rows x 4 chunks per 16 lanes)
// write: lane (l15, q) of the MFMA C layout owns row mf*16 + l15, columns nf*16 + 4*q + {0..3} of the 32-column half (nf = 0, 1)
__device__ __forceinline__ unsigned dk_tail_stage_off(int row, int nf, int q) {
  return (unsigned)(row * 64 + (((nf * 2 + (q >> 1)) ^ ((row >> 2) & 3)) << 4) + (q & 1) * 8);
}
// read: lane takes the 8 columns of chunk `chunk` (= lane & 3) of row `row`
__device__ __forceinline__ unsigned dk_tail_read_off(int row, int chunk) {
  return row * 64 + (((unsigned)chunk ^ ((unsigned)(row >> 2) & 3u)) << 4);
}
__device__ __forceinline__ u32x4 dk_tail_read(unsigned reg0, int row, int chunk) {
  return *(const __attribute__((address_space(3))) u32x4*)((dk_tail_lds*)0 + reg0 + dk_tail_read_off(row, chunk));
}

__device__ __forceinline__ void dk_tail_unpack8(const uint4 v, float* f) {
  unpack2(v.x, f[0], f[1]);
  unpack2(v.y, f[2], f[3]);
  unpack2(v.z, f[4], f[5]);
  unpack2(v.w, f[6], f[7]);
}
__device__ __forceinline__ uint4 dk_tail_pack8(const float* vv) {
  uint4 o4;
  o4.x = pack2(vv[0], vv[1]);
  o4.y = pack2(vv[2], vv[3]);
  o4.z = pack2(vv[4], vv[5]);
  o4.w = pack2(vv[6], vv[7]);
  return o4;
}

// ---- tile set-up: what the read-back of one output tile needs, evaluated once (scalar unit)
struct DkTailTile {
  bf16_t* Cb;  // the output this tile goes to (second output of a column split: C2), its leading dimension and epilogue
  int ldcb, epi;
  int n0, ncol0;  // first column of the tile in the GEMM (bias, gate, residual) / inside its output
  int m0, mrow0;  // first GEMM row of the tile / of this wave's block of rows
  int M, c_seg_len, ldr;
  bool has_res;
  // fast: the tile lies inside one row segment of every map and inside M: the maps are evaluated once; otherwise each lane walks its rows
  // through the maps.  cut (gemm256v4.hip only): inside one segment of every map, but M ends inside the tile
  bool fast, cut;
  size_t physC0, physR0;    // fast / cut: physical row of the wave's first row in C and in the residual  (dk_tail_first_rows)
  const bf16_t* gate_row;   // fast / cut: the tile's gate row                                          (dk_tail_first_rows)
  bool kfuse;               // key or query tile with the fused QKNorm + RoPE ...
  const bf16_t* nw;         // ... and its norm weight
};

// BM: rows of the tile; brow: first row of this wave's block inside it.  M, ldc, c_seg_len, ldr are passed beside `p`: gemm256f8.hip keeps them
// as named scalars (a select between its two parameter blocks once became a scratch copy, tests/test_codegen_guards.py)
template <bool WITH_CUT, class P>
__device__ __forceinline__ DkTailTile dk_tail_tile(const P& p, int m0, int n0, int BM, int brow, int M, int ldc, int c_seg_len, int ldr) {
  DkTailTile t;
  const bool out2 = p.n_split > 0 && n0 >= p.n_split;  // tile-uniform: second output of a column-split GEMM
  t.Cb = (bf16_t*)(out2 ? p.C2 : p.C);
  t.ldcb = out2 ? p.ldc2 : ldc;
  t.epi = out2 ? p.epi2 : p.epi;
  t.n0 = n0;
  t.ncol0 = out2 ? n0 - p.n_split : n0;
  t.m0 = m0, t.mrow0 = m0 + brow;
  t.M = M, t.c_seg_len = c_seg_len, t.ldr = ldr;
  t.has_res = t.epi == DK_EPI_GATE_RES || t.epi == DK_EPI_RES;
  auto inside = [&](int len) { return m0 / len == (m0 + BM - 1) / len; };
  t.fast = m0 + BM <= M && inside(c_seg_len) && (!t.has_res || inside(p.r_seg_len)) && (t.epi != DK_EPI_GATE_RES || inside(p.gate_seg_len));
  t.cut = false;
  if (WITH_CUT) {  // the last row tile of a single-segment problem: tile-uniform maps, M ends inside it
    auto inside_cut = [&](int len) { return m0 / len == (M - 1) / len; };
    t.cut = !t.fast && m0 + BM > M && inside_cut(c_seg_len) && (!t.has_res || inside_cut(p.r_seg_len)) &&
            (t.epi != DK_EPI_GATE_RES || inside_cut(p.gate_seg_len));
  }
  t.physC0 = t.physR0 = 0, t.gate_row = nullptr;  // (dk_tail_first_rows)
  const bool qtile = p.qn_w != nullptr && n0 >= p.qn_col0 && n0 < p.qn_col1;  // query tile: same treatment as a key tile, own weight
  t.kfuse = p.kn_w != nullptr && ((n0 >= p.kn_col0 && n0 < p.kn_col1) || qtile);
  t.nw = qtile ? p.qn_w : p.kn_w;
  return t;
}

// the physical first rows and the gate row of a tile-uniform tile.  EK: the epilogue where the caller knows it at compile time (gemm256v4.hip calls
// this behind its dispatch: a bias-only tile then computes neither residual row nor gate row), or -1: t.epi
template <int EK, class P>
__device__ __forceinline__ void dk_tail_first_rows(const P& p, DkTailTile& t) {
  const bool hres = EK >= 0 ? (EK == DK_EPI_GATE_RES || EK == DK_EPI_RES) : t.has_res;
  const bool gate = EK >= 0 ? EK == DK_EPI_GATE_RES : t.epi == DK_EPI_GATE_RES;
  const int m0 = t.m0, brow = t.mrow0 - t.m0;
  t.physC0 = (size_t)((m0 / t.c_seg_len) * p.c_seg_stride + (m0 % t.c_seg_len)) + brow;
  t.physR0 = hres ? (size_t)((m0 / p.r_seg_len) * p.r_seg_stride + (m0 % p.r_seg_len)) + brow : 0;
  t.gate_row = gate ? p.gate + (size_t)(m0 / p.gate_seg_len) * p.gate_stride : nullptr;
}

// ---- row walk of the slow path: (segment, row inside it) of this lane's current row in the C, residual and gate maps; 16 rows per step
struct DkTailWalk {
  int c_seg = 0, c_rem = 0, r_seg = 0, r_rem = 0, g_seg = 0, g_rem = 0;
  template <class P>
  __device__ __forceinline__ void start(const P& p, int c_seg_len, int ms, bool hres, bool gate) {
    c_seg = ms / c_seg_len, c_rem = ms % c_seg_len;
    if (hres) r_seg = ms / p.r_seg_len, r_rem = ms % p.r_seg_len;
    if (gate) g_seg = ms / p.gate_seg_len, g_rem = ms % p.gate_seg_len;
  }
  template <class P>
  __device__ __forceinline__ size_t crow(const P& p) const { return (size_t)c_seg * p.c_seg_stride + c_rem; }
  template <class P>
  __device__ __forceinline__ size_t rrow(const P& p) const { return (size_t)r_seg * p.r_seg_stride + r_rem; }
  template <class P>
  __device__ __forceinline__ const bf16_t* gate(const P& p) const { return p.gate + (size_t)g_seg * p.gate_stride; }
  template <class P>
  __device__ __forceinline__ void step(const P& p, int c_seg_len, bool hres, bool gate) {
    for (c_rem += 16; c_rem >= c_seg_len; c_rem -= c_seg_len) ++c_seg;
    if (hres)
      for (r_rem += 16; r_rem >= p.r_seg_len; r_rem -= p.r_seg_len) ++r_seg;
    if (gate)
      for (g_rem += 16; g_rem >= p.gate_seg_len; g_rem -= p.gate_seg_len) ++g_seg;
  }
};

// ---- per-row finish: from the staged values of a lane's 8 columns to what is stored.  Same arithmetic and rounding points as
// dk_qk_norm_rope_kernel and the stand-alone epilogue kernels.
// fused QKNorm: round(v * rsqrt(ss / D + eps) * w), ss = the row's sum of squares over its head
__device__ __forceinline__ void dk_tail_norm8(float* vv, float ss, int D, float eps, const float* kw8) {
  const float r = rsqrtf(ss / (float)D + eps);
#pragma unroll
  for (int e = 0; e < 8; ++e) vv[e] = round_act(vv[e] * r * kw8[e]);
}
// RoPE: four (even, odd) pairs by the (cos, sin) pairs t0 = {c0, s0, c1, s1}, t1 = {c2, s2, c3, s3}
__device__ __forceinline__ void dk_tail_rotate8(float* vv, f32x4 t0, f32x4 t1) {
  const float cs[8] = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float c = cs[2 * i], sn = cs[2 * i + 1], xe = vv[2 * i], xo = vv[2 * i + 1];
    vv[2 * i] = c * xe - sn * xo;
    vv[2 * i + 1] = sn * xe + c * xo;
  }
}
template <class P>
__device__ __forceinline__ const float* dk_tail_rope_entry(const P& p, int kpos, int kcol) {
  return p.kn_rope + ((size_t)(p.kn_pos_off + kpos) * (size_t)(p.kn_D / 2) + (size_t)(kcol >> 1)) * 2;
}
// epilogue `ep` on values that hold round(alpha * acc + bias); res(): the residual's 8 columns (called only where the epilogue reads them),
// gate8: the gate's
template <class Res>
__device__ __forceinline__ void dk_tail_epilogue8(float* vv, int ep, bool hres, Res res, const float* gate8) {
  if (ep == DK_EPI_BIAS_GELU) {
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
      const f32x2 g2 = gelu_erf_f2(f32x2{vv[e], vv[e + 1]});
      vv[e] = g2[0], vv[e + 1] = g2[1];
    }
  } else if (ep == DK_EPI_BIAS_SILU) {
#pragma unroll
    for (int e = 0; e < 8; ++e) vv[e] = silu_f(vv[e]);
  } else if (hres) {
    float r8[8];
    dk_tail_unpack8(res(), r8);
    if (ep == DK_EPI_GATE_RES) {
#pragma unroll
      for (int e = 0; e < 8; ++e) vv[e] = r8[e] + round_act(gate8[e] * vv[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) vv[e] += r8[e];
    }
  }
}

// ---- sum of squares of key / query rows for the 8-wave kernels (gemm256v3.hip, gemm256f8.hip): this wave's 64 columns from the accumulators
// (the same rounded values that get staged; scale(nf, e): alpha, or the weight scale of the column), left in LDS behind the staging images;
// a 128-column head adds the partner wave's half when it reads.  (gemm256v4.hip sums the staged image instead, in another order.)
constexpr unsigned DK_TAIL_XCH_OFF = 8u * 16384u;
template <int MF, class Scale>
__device__ __forceinline__ void dk_tail_sumsq_exchange(const f32x4 (&acc)[4][MF], const u32x2 (&bias_q)[4], Scale scale, int wave, int l15, int q) {
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    float ss = 0.f;
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) {
      float b4[4];
      unpack2(bias_q[nf][0], b4[0], b4[1]);
      unpack2(bias_q[nf][1], b4[2], b4[3]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = round_act(acc[nf][mf][e] * scale(nf, e) + b4[e]);
        ss += v * v;
      }
    }
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    if (q == 0) *(__attribute__((address_space(3))) float*)((dk_tail_lds*)0 + DK_TAIL_XCH_OFF + (wave * 128 + mf * 16 + l15) * 4) = ss;
  }
  __syncthreads();
}
__device__ __forceinline__ float dk_tail_sumsq_read(int wave, int row, int D) {
  float ss = *(const __attribute__((address_space(3))) float*)((dk_tail_lds*)0 + DK_TAIL_XCH_OFF + (wave * 128 + row) * 4);
  if (D == 128) ss += *(const __attribute__((address_space(3))) float*)((dk_tail_lds*)0 + DK_TAIL_XCH_OFF + ((wave ^ 1) * 128 + row) * 4);
  return ss;
}

// ---- row loop: NPASS 32-column passes of one wave, MF steps of 16 rows each.
// FAST: tile-uniform row maps (t.fast, or t.cut with CUT); EK: the epilogue folded at compile time (-1: t.epi at run time); KF: key / query
// tile with the fused QKNorm + RoPE (bias-only epilogue).
// CUT (with FAST): the tile lies inside one segment of every map but M ends inside it (the last row tile: 4352 rows in 224-row tiles) -- the
// tile-uniform addressing of FAST with a row limit: rows past it are neither stored nor (residual) loaded from their own address.
// RAW_OK: `store_raw` takes the staged words as they are, so a bias-only epilogue stores them unchanged (PLAIN).
//   pass_of(pass) -> DkTailPass: the pass's image and its first column inside the tile
//   ss_of(pass, itr, row) -> the sum of squares of row `row` (= itr * 16 + lane / 4 of the wave's block) over this lane's head (KF only)
//   store(itr, crow, ocol, ok, vv) / store_raw(crow, ocol, ok, sv): physical output row, column inside the output, `ok`: the row exists
// FAST tiles fetch everything the rows read from memory before the first store, for all passes at once: the residual is updated in place
// (C == res), so the compiler may not move a row's load above the previous row's store, and as written row by row every row of every pass was
// its own dependent memory round trip (with the fused norm two more loads per row for the cos / sin entries).
struct DkTailPass {
  unsigned reg0;  // LDS byte offset of the pass's 8 KiB image
  int coff;       // first of its 32 columns inside the tile
};
template <bool FAST, int EK, bool KF, int MF, bool CUT, int NPASS, bool RAW_OK, class P, class PassOf, class SsOf, class Store, class StoreRaw>
__device__ __forceinline__ void dk_tail_rows(const P& p, const DkTailTile& t, int lane, PassOf pass_of, SsOf ss_of, Store store, StoreRaw store_raw) {
  static_assert(FAST || !CUT, "CUT is a form of FAST");
  static_assert(!CUT || EK >= 0, "CUT: the residual rows are fetched up front, with the row limit");
  constexpr int HROWS = 16 * MF;  // rows of a wave's block (the LDS image keeps 128-row regions; a 224-row tile uses 112 of each)
  constexpr bool PLAIN = RAW_OK && EK == DK_EPI_BIAS && !KF;  // the staged values ARE the output
  const int rrow = lane >> 2, rc2 = (lane & 3) * 2;
  const int row_lim = CUT ? t.M - 1 - t.mrow0 : HROWS;  // last valid row of this wave's block
  if (CUT && row_lim < 0) return;                       // (the whole block lies past M)
  const int ep = EK >= 0 ? EK : t.epi;
  const bool hres = EK >= 0 ? (EK == DK_EPI_GATE_RES || EK == DK_EPI_RES) : t.has_res;
  constexpr bool PRE_RES = FAST && (EK == DK_EPI_GATE_RES || EK == DK_EPI_RES);
  constexpr bool PRE_GATE = FAST && EK == DK_EPI_GATE_RES;
  constexpr bool PRE_ROPE = FAST && KF;
  uint4 res_pre[PRE_RES ? NPASS : 1][PRE_RES ? MF : 1];
  f32x4 rope_pre[PRE_ROPE ? NPASS : 1][PRE_ROPE ? 2 * MF : 1];
  float gate_pre[PRE_GATE ? NPASS : 1][8];
#pragma unroll
  for (int pass = 0; pass < NPASS; ++pass) {
    const int col = t.n0 + pass_of(pass).coff + rc2 * 4;
    if (PRE_RES) {
#pragma unroll
      for (int itr = 0; itr < MF; ++itr)
        res_pre[pass][itr] = *(const uint4*)(p.res + (t.physR0 + (CUT ? min(itr * 16 + rrow, row_lim) : itr * 16 + rrow)) * (size_t)t.ldr + col);
    }
    if (PRE_GATE) dk_tail_unpack8(*(const uint4*)(t.gate_row + col), gate_pre[pass]);
    if (PRE_ROPE) {
      if (p.kn_rope != nullptr) {
        const int kcol = col % p.kn_D;
#pragma unroll
        for (int itr = 0; itr < MF; ++itr) {
          const float* tab = dk_tail_rope_entry(p, (t.mrow0 + itr * 16 + rrow) % p.kn_seg_len, kcol);
          rope_pre[pass][2 * itr] = *(const f32x4*)tab, rope_pre[pass][2 * itr + 1] = *(const f32x4*)(tab + 4);
        }
      }
    }
  }
#pragma unroll
  for (int pass = 0; pass < NPASS; ++pass) {
    const DkTailPass ps = pass_of(pass);
    const int col = t.n0 + ps.coff + rc2 * 4;      // first of this lane's 8 columns of the GEMM (gate, residual)
    const int ocol = t.ncol0 + ps.coff + rc2 * 4;  // the same inside the output it goes to
    float gate8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float kw8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int kcol = KF ? col % p.kn_D : 0;  // first of this lane's 8 columns inside its head (the ranges start at multiples of 256)
    if (KF) dk_tail_unpack8(*(const uint4*)(t.nw + kcol), kw8);
    if (PRE_GATE) {
#pragma unroll
      for (int e = 0; e < 8; ++e) gate8[e] = gate_pre[pass][e];
    } else if (FAST && ep == DK_EPI_GATE_RES) {
      dk_tail_unpack8(*(const uint4*)(t.gate_row + col), gate8);
    }
    DkTailWalk w;
    if (!FAST) w.start(p, t.c_seg_len, t.mrow0 + rrow, hres, ep == DK_EPI_GATE_RES);
#pragma unroll
    for (int itr = 0; itr < MF; ++itr) {
      const int row = itr * 16 + rrow;  // row inside the wave's block of HROWS rows
      size_t crow = t.physC0 + row, rrow_phys = t.physR0 + row;
      bool valid = !CUT || row <= row_lim;
      const int kpos = KF ? (t.mrow0 + row) % p.kn_seg_len : 0;  // the row's position inside its sequence
      if (!FAST) {
        valid = t.mrow0 + row < t.M;
        crow = w.crow(p);
        rrow_phys = w.rrow(p);
        if (ep == DK_EPI_GATE_RES && valid) dk_tail_unpack8(*(const uint4*)(w.gate(p) + col), gate8);
        w.step(p, t.c_seg_len, hres, ep == DK_EPI_GATE_RES);
      }
      const bool ok = (FAST && !CUT) || valid;
      const u32x4 sv = dk_tail_read(ps.reg0, row, rc2 >> 1);
      if (PLAIN) {
        store_raw(crow, ocol, ok, sv);
        continue;
      }
      float vv[8];
      dk_tail_unpack8(make_uint4(sv[0], sv[1], sv[2], sv[3]), vv);
      if (KF) {
        dk_tail_norm8(vv, ss_of(pass, itr, row), p.kn_D, p.kn_eps, kw8);
        if (p.kn_rope != nullptr) {
          const float* tab = dk_tail_rope_entry(p, kpos, kcol);
          f32x4 t0 = {1.f, 0.f, 1.f, 0.f}, t1 = {1.f, 0.f, 1.f, 0.f};
          if (PRE_ROPE) t0 = rope_pre[pass][2 * itr], t1 = rope_pre[pass][2 * itr + 1];
          else if (valid) t0 = *(const f32x4*)tab, t1 = *(const f32x4*)(tab + 4);
          dk_tail_rotate8(vv, t0, t1);
        }
      }
      auto res = [&] {
        uint4 rr = make_uint4(0u, 0u, 0u, 0u);
        if (PRE_RES) rr = res_pre[pass][itr];
        else if (FAST || valid) rr = *(const uint4*)(p.res + rrow_phys * (size_t)t.ldr + col);
        return rr;
      };
      dk_tail_epilogue8(vv, ep, hres, res, gate8);
      store(itr, crow, ocol, ok, vv);
    }
  }
}
