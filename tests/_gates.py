"""Per-element and per-row gates of the operator parity tests, their fp32 restatements, case lists and mutants (tests/test_gate_power_cpu.py proves
the gates on the host, tests/test_gpu_ops.py and tests/test_gpu_f16_ops.py apply them to the HIP kernels).  Plain torch, no GPU.

A whole-tensor rel-L2 at 3e-3 sits over a bf16 rounding floor of 1.7e-3 and cannot see a fault confined to a row, a fragment or a tile edge.  The gates here
are local:

  GEMM / conv, per element:   |got - ref| <= sp(ref) + (epilogue terms) + C_GEMM unit,   unit = sum_k |a_k| |w_k| + |bias|
  attention / norms, per row: ||got_row - ref_row||_2 <= c_row ||ref_row||_2 + sqrt(L) sp(0)

``ref`` is fp64, ``sp`` the spacing of the element type (tests/_numeric_range.py).  Every constant is MEASURED on an fp32 restatement of the operation (never
on a kernel) on the inputs of the tests, and doubled; the measured values stand beside the constants and in DESIGN.md section 4.  The mutants return the
restatement's result with one fault a kernel of this design could have; each names the code it imitates."""
import math

import torch
import torch.nn.functional as F

from tests import _numeric_range as NR
from tests._numeric_range import BF, F16, gelu64, rnd, silu64, spacing, worst
from tests._util import randn

LOG2E = 1.4426950408889634
TILE = 256          # row tile of the 256 x 256 GEMM kernels (gemm256v3.hip, gemm256v4.hip)
SUBSET_ABOVE = 1178 * 1536 * 1536  # fp64 references of larger problems are formed for a row subset only
DERIV = 1.13        # |gelu'| <= 1.129, |silu'| <= 1.0999


def inputs(dt, *shape, seed, scale=1.0):
    """the tests' own constructors: tests/_util.randn (bf16-representable), rounded once more for float16 (test_gpu_f16_ops.rnd)"""
    x = randn(*shape, seed=seed, scale=scale)
    return rnd(x, F16) if dt == F16 else x


def row_subset(M, N, K, seed=0):
    """None (every row) up to 1178 x 1536 x 1536 (products) and 1178 x 1536 outputs; above: every row of the first and of the last row tile, 64 seeded
    random rows and row (M + 1) / 2"""
    if (M * N * K <= SUBSET_ABOVE and M * N <= 1178 * 1536) or M <= 2 * TILE + 64:
        return None
    last0 = (M - 1) // TILE * TILE
    mid = torch.randperm(last0 - TILE, generator=torch.Generator().manual_seed(900 + seed + M))[:64] + TILE
    seg2 = torch.tensor([(M + 1) // 2])  # (the first row of a second row segment, where the gate row changes)
    return torch.cat([torch.arange(TILE), torch.cat([mid, seg2]).unique(), torch.arange(last0, M)])


def col_subset(M, N, K, seed=0):
    """with a row subset, N > 576: the first and the last column tile and 64 seeded random columns of the tiles between (every mutant sits in the first or
    the last column tile); else None"""
    if row_subset(M, N, K) is None or N <= 2 * TILE + 64:
        return None
    last0 = (N - 1) // TILE * TILE
    mid = torch.randperm(last0 - TILE, generator=torch.Generator().manual_seed(901 + seed + N))[:64] + TILE
    return torch.cat([torch.arange(TILE), mid.sort().values, torch.arange(last0, N)])


def pixel_subset(B, Ho, Wo, work):
    """conv outputs above the same size: the first and the last 16 pixel rows of every image and 4 seeded rows between -> mask [B, Ho, Wo] or None"""
    if work <= SUBSET_ABOVE or Ho <= 36:
        return None
    m = torch.zeros(B, Ho, Wo, dtype=torch.bool)
    m[:, :16], m[:, Ho - 16:] = True, True
    m[:, torch.randperm(Ho - 32, generator=torch.Generator().manual_seed(902 + Ho))[:4] + 16] = True
    return m


# ---- GEMM and conv: per element ----------------------------------------------------------------------------------------------------------------
# C_GEMM: twice the worst |fp32 restatement - ref64| / unit over GEMM_CASES and CONV_CASES, both summation orders (torch's own, K walked in 32-wide
# steps as the MFMA loops do), before any rounding.  Measured (test_gate_power_cpu.py::test_gemm_gate / test_conv_gate print them): GEMM 1.81e-7
# (1178 x 512 x 384, seeds 50-52, torch's order; 32-wide steps: 9.27e-8 at 256 x 256 x 64), conv 1.91e-7 ((2, 16, 24, 128) nearest-x2 -> 256 channels,
# torch's order; tap by tap in 32-channel steps: 6.53e-8)
C_GEMM = 3.9e-7


def gemm_f32(x, w, b, order="torch"):
    """fp32 accumulation of x w^T (+ b): torch's own order, or K walked in 32-wide steps"""
    if order == "torch":
        acc = x @ w.t()
    else:
        acc = torch.zeros(x.shape[0], w.shape[0])
        for k0 in range(0, x.shape[1], 32):
            acc += x[:, k0:k0 + 32] @ w[:, k0:k0 + 32].t()
    return acc if b is None else acc + b


def epilogue_f32(acc, dt, epi, res=None, gate=None):
    """the tails' rounding points (dk_gemm_tail.h): round(acc + bias), the function on the rounded value, gate x rounded, + residual, final rounding"""
    pre = rnd(acc, dt)
    if epi == "bias":
        return pre
    if epi == "gelu":
        return rnd(0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0))), dt)
    if epi == "silu":
        return rnd(pre * torch.sigmoid(pre), dt)
    if epi == "res":
        return rnd(res + pre, dt)
    return rnd(res + rnd(gate * pre, dt), dt)


def epilogue_bound(pre, unit, dt, epi, res=None, gate=None):
    """(ref64, bound) from the fp64 pre-activation and its unit: the error of the pre-activation, sp(pre) + C unit, goes through the epilogue by its
    derivative bound (GELU / SiLU 1.13, gate x by |gate|); every further rounding point adds its spacing, taken at |value| + the error that has reached
    it (a value pushed over a power of two is rounded on the coarser grid)"""
    e = spacing(pre.abs() + C_GEMM * unit, dt) + C_GEMM * unit
    if epi == "bias":
        return pre, e
    if epi in ("gelu", "silu"):
        ref = gelu64(pre) if epi == "gelu" else silu64(pre)
        return ref, spacing(ref.abs() + DERIV * e, dt) + DERIV * e
    if epi == "res":
        ref = res.double() + pre
        return ref, spacing(ref.abs() + e, dt) + e
    gp = gate.double() * pre
    ge = gate.double().abs() * e
    e_gp = spacing(gp.abs() + ge, dt) + ge
    ref = res.double() + gp
    return ref, spacing(ref.abs() + e_gp, dt) + e_gp


def gemm_ref64(x, w, b):
    """(fp64 x w^T + b, unit); the unit is a magnitude under a constant of 4e-7 and is summed in fp32"""
    pre = x.double() @ w.double().t()
    unit = (x.abs() @ w.abs().t()).double()
    if b is not None:
        pre, unit = pre + b.double(), unit + b.double().abs()
    return pre, unit


def gemm_gate(got, x, w, b, dt, epi="bias", res=None, gate=None, rows=None):
    """worst |got - ref| / bound of a GEMM output [M, N], or of several (a list: one reference serves them all); ``gate`` already expanded to rows
    [M, N] or broadcastable [1, N]; ``rows``: the subset"""
    gots = got if isinstance(got, (list, tuple)) else [got]
    if rows is not None:
        gots, x = [t[rows] for t in gots], x[rows]
        res = res[rows] if res is not None else None
        gate = gate[rows] if gate is not None and gate.shape[0] > 1 else gate
        cols = col_subset(got[0].shape[0] if isinstance(got, (list, tuple)) else got.shape[0], w.shape[0], w.shape[1])
        if cols is not None:
            gots, w, b = [t[:, cols] for t in gots], w[cols], (b[cols] if b is not None else None)
            res = res[:, cols] if res is not None else None
            gate = gate[:, cols] if gate is not None else None
    pre, unit = gemm_ref64(x, w, b)
    ref, bound = epilogue_bound(pre, unit, dt, epi, res, gate)
    return max(worst((t.detach().double().cpu() - ref).abs(), bound) for t in gots)


def _gemm_case(name, M, N, K, seeds, wscale, bscale, epi="bias", dt=BF, gate_rows=1, ksplit=False):
    return dict(name=name, M=M, N=N, K=K, seeds=seeds, wscale=wscale, bscale=bscale, epi=epi, dt=dt, gate_rows=gate_rows, ksplit=ksplit)


# (the GPU tests' shapes and seeds; where a test runs one shape with several epilogues the large shapes carry one of them here.  No case has
# K % 64 == 32: every GEMM route requires K % 64 == 0, gemm.hip "K must be a multiple of 64")
GEMM_CASES = (
    [_gemm_case(f"bias {M}x{N}x{K}", M, N, K, (1, 2, 3, None, None), 0.05, 1.0)
     for M, N, K in ((128, 128, 64), (256, 384, 128), (100, 200, 192), (1178, 1536, 1536), (4352, 3072, 3072), (7, 64, 256), (333, 3, 1152), (2, 344 * 128, 128))]
    + [_gemm_case(f"epilogues {e}", 320, 384, 256, (4, 5, 6, 7, 8), 0.05, 0.1, e, gate_rows=2) for e in ("gelu", "silu", "gate_res", "res")]
    + [_gemm_case(f"variants {e}", 1024, 768, 640, (14, 15, 16, 17, 18), 0.05, 0.1, e, gate_rows=2) for e in ("bias", "gelu", "gate_res")]
    + [_gemm_case(f"half tile {e}", 1100, 384, 640, (21, 22, 23, 24, 25), 0.03, 0.1, e, gate_rows=2) for e in ("bias", "gelu", "gate_res")]
    + [_gemm_case("half tile 2356 gate_res", 2356, 2432, 2432, (21, 22, 23, 24, 25), 0.03, 0.1, "gate_res", gate_rows=2)]
    + [_gemm_case(f"v4=v3 {M}x{N}x{K} {e}", M, N, K, (70, 71, 72, 73, 74), 0.05, 0.1, e)
       for (M, N, K), e in (((256, 256, 64), "bias"), ((300, 512, 128), "gelu"), ((1024, 768, 192), "gate_res"), ((777, 256, 256), "gelu"),
                            ((2048, 1024, 448), "gate_res"), ((4352, 3072, 3072), "gelu"), ((224, 256, 128), "bias"), ((4480, 512, 2048), "gate_res"))]
    + [_gemm_case(f"split {M}x{N}x{K} {e}", M, N, K, (50, 51, 52, 53, 54), 0.05, 0.1, e, ksplit=True)
       for M, N, K, e in ((1024, 768, 640, "gate_res"), (1178, 512, 384, "bias"), (3328, 2560, 256, "gelu"), (4352, 3072, 512, "gate_res"))]
    + [_gemm_case(f"auto split {M}x{N}x{K} {e}", M, N, K, (60, 61, 62, 63, 64), 0.02, 0.1, e, ksplit=True)
       for M, N, K, e in ((1280, 3072, 15360, "gate_res"), (2560, 3072, 12288, "bias"))]
    + [_gemm_case(f"f16 128 {M}x{N}x{K} {e}", M, N, K, (10, 11, 12, 13, 14), 0.08, 0.1, e, dt=F16)
       for M, N, K in ((154, 384, 256), (77, 256, 448)) for e in ("bias", "gelu", "silu", "gate_res")]
    + [_gemm_case("f16 k split", 1024, 512, 6144, (50, 51, 52, None, None), 0.02, 0.1, "bias", dt=F16, ksplit=True)])


def gemm_operands(c):
    """(x, w, b, res, gate [M, N] rows or None, rows) of a case, as the GPU test draws them"""
    dt, (sx, sw, sb, sr, sg) = c["dt"], c["seeds"]
    M, N, K = c["M"], c["N"], c["K"]
    x, w, b = inputs(dt, M, K, seed=sx), inputs(dt, N, K, seed=sw, scale=c["wscale"]), inputs(dt, N, seed=sb, scale=c["bscale"])
    res = gate = None
    if c["epi"] in ("res", "gate_res"):
        res = inputs(dt, M, N, seed=sr)
    if c["epi"] == "gate_res":
        gr = c["gate_rows"]
        gate = inputs(dt, gr, N, seed=sg).repeat_interleave((M + gr - 1) // gr, 0)[:M]
    return x, w, b, res, gate, row_subset(M, N, K)


class GemmRestatement:
    """the fp32 accumulator of a case on its row subset and everything the mutants need"""

    def __init__(self, c, order="steps"):
        self.c, self.dt, self.epi = c, c["dt"], c["epi"]
        x, w, b, res, gate, rows = gemm_operands(c)
        self.M, self.N, self.K = c["M"], c["N"], c["K"]
        self.idx = torch.arange(self.M) if rows is None else rows          # global row of every subset row
        cols = col_subset(self.M, self.N, self.K)
        cols = torch.arange(self.N) if cols is None else cols
        self.Ns = cols.numel()                                              # columns of the subset: the first and the last column tile at its ends
        self.x, self.w, self.b = x[self.idx], w[cols], b[cols]
        self.res = res[self.idx][:, cols] if res is not None else None
        self.gate = gate[self.idx][:, cols] if gate is not None else None
        self.acc = gemm_f32(self.x, self.w, self.b, order)
        self.pre64, self.unit = gemm_ref64(self.x, self.w, self.b)
        self.ref, self.bound = epilogue_bound(self.pre64, self.unit, self.dt, self.epi, self.res, self.gate)

    def out(self, acc=None):
        return epilogue_f32(self.acc if acc is None else acc, self.dt, self.epi, self.res, self.gate)

    def ratio(self, got):
        return worst((got.double() - self.ref).abs(), self.bound)

    def unit_error(self):
        return float(((self.acc.double() - self.pre64).abs() / self.unit).max())

    # -- mutants (positions are subset rows; the last subset rows are the last row tile) --
    def last_tile_row(self):
        """a row of the ragged last row tile (the last row; with M % 256 == 0 the last tile is whole and the row is its last)"""
        return self.idx.numel() - 1

    def m_k_step_dropped(self):
        """gemm256v3.hip / gemm256v4.hip K loop: the last 32-wide MFMA step missing for one row of the last row tile x the first column tile"""
        r, nc = self.last_tile_row(), min(TILE, self.Ns)
        acc = self.acc.clone()
        acc[r, :nc] -= self.x[r, self.K - 32:] @ self.w[:nc, self.K - 32:].t()
        return self.out(acc)

    def m_bias_missing(self):
        """dk_gemm_tail.h bias load: the ragged N % 4 columns (else the last 4) of the last 3 rows get no bias"""
        n = self.N % 4 or 4
        acc = self.acc.clone()
        acc[-3:, self.Ns - n:] -= self.b[self.Ns - n:]
        return self.out(acc)

    def m_one_zero(self, q=0.5):
        """a store skipped by a wrong row / column limit in the tail: one element of the last row left zero (the one at quantile ``q`` of the row's
        magnitudes; the median: a typical element)"""
        out = self.out()
        out[-1, int(self.ref[-1].abs().argsort()[int(self.Ns * q)])] = 0.0
        return out

    def m_fragment_swapped(self):
        """the staged-tile read-back (dk_gemm_tail.h): one 16 x 16 MFMA fragment taken from the neighbouring 16-column block"""
        acc = self.acc.clone()
        r0 = max(0, self.idx.numel() - 16)
        acc[r0:r0 + 16, 0:16] = (self.acc[r0:r0 + 16, 16:32] - self.b[16:32]) + self.b[0:16]
        return self.out(acc)

    def m_gate_row(self):
        """gate_res tails: the first row of segment 2 gated with segment 1's gate row (the per-lane row walk of a tile that straddles segments)"""
        seg = (self.M + 1) // 2
        r = int((self.idx == seg).nonzero()[0])
        gate = self.gate.clone()
        gate[r] = self.gate[0]
        return epilogue_f32(self.acc, self.dt, self.epi, self.res, gate)

    def m_gelu_before_bias(self):
        """BIAS_GELU tails: the function applied to the accumulator and the bias added behind it, on one row"""
        out = self.out()
        a = rnd(self.acc[-1] - self.b, self.dt)
        out[-1] = rnd(0.5 * a * (1.0 + torch.erf(a / math.sqrt(2.0))) + self.b, self.dt)
        return out

    def m_slab_omitted(self):
        """dk_ksplit.h finisher: one producer slab (here the last quarter of K, in 64-wide K tiles) never added for the first 256 x 256 tile"""
        k0 = self.K - max(64, self.K // 4 // 64 * 64)
        nr, nc = min(TILE, self.idx.numel()), min(TILE, self.Ns)
        acc = self.acc.clone()
        acc[:nr, :nc] -= self.x[:nr, k0:] @ self.w[:nc, k0:].t()
        return self.out(acc)

    def mutants(self):
        m = {"k step dropped": self.m_k_step_dropped, "bias missing": self.m_bias_missing, "one element zero": self.m_one_zero}
        if self.N >= 32:
            m["fragment swapped"] = self.m_fragment_swapped
        if self.epi == "gate_res" and self.c["gate_rows"] == 2:
            m["gate row of segment 1"] = self.m_gate_row
        if self.epi == "gelu":
            m["gelu before bias"] = self.m_gelu_before_bias
        if self.c["ksplit"]:
            m["slab omitted"] = self.m_slab_omitted
        return m


# conv 3 x 3 as a GEMM over 9 taps x C channels
def conv_taps(x, mode):
    """the nine shifted [B, Ho, Wo, C] views of a 3 x 3 conv: "plain" (pad 1), "ups" (nearest x 2, then pad 1), "s2" (pad bottom / right, stride 2)"""
    if mode == "ups":
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    B, H, W, C = x.shape
    if mode == "s2":
        xp, Ho, Wo, st = F.pad(x, (0, 0, 0, 1, 0, 1)), H // 2, W // 2, 2
    else:
        xp, Ho, Wo, st = F.pad(x, (0, 0, 1, 1, 1, 1)), H, W, 1
    return [[xp[:, ky:ky + Ho * st:st, kx:kx + Wo * st:st] for kx in range(3)] for ky in range(3)]


def conv_ref64(x, w, b, mode, mask=None):
    """(pre, unit) [B, Ho, Wo, O], or [pixels, O] over the pixels of ``mask``"""
    taps = conv_taps(x, mode)
    pre = unit = 0.0
    for ky in range(3):
        for kx in range(3):
            t, wk = (taps[ky][kx] if mask is None else taps[ky][kx][mask]), w[:, ky, kx]
            pre, unit = pre + t.double() @ wk.double().t(), unit + (t.abs() @ wk.abs().t()).double()
    return pre + b.double(), unit + b.double().abs()


def conv_f32(x, w, b, mode, order="torch", drop=None):
    """fp32 conv: torch's own order, or tap by tap in 32-channel steps.  ``drop`` = (tile-row mask [B, Ho, Wo], c0): channels from c0 on missing there"""
    taps = conv_taps(x, mode)
    if order == "torch":
        xin = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) if mode == "ups" else x
        xin = F.pad(xin.permute(0, 3, 1, 2), (0, 1, 0, 1)) if mode == "s2" else xin.permute(0, 3, 1, 2)
        return F.conv2d(xin, w.permute(0, 3, 1, 2), b, stride=2 if mode == "s2" else 1, padding=0 if mode == "s2" else 1).permute(0, 2, 3, 1).contiguous()
    acc = torch.zeros(*taps[0][0].shape[:3], w.shape[0])
    for ky in range(3):
        for kx in range(3):
            for c0 in range(0, x.shape[-1], 32):
                acc += taps[ky][kx][..., c0:c0 + 32] @ w[:, ky, kx, c0:c0 + 32].t()
    return acc + b


def conv_gate(got, x, w, b, dt, mode="plain", res=None):
    gots = got if isinstance(got, (list, tuple)) else [got]
    B, Ho, Wo, O = gots[0].shape
    mask = pixel_subset(B, Ho, Wo, B * Ho * Wo * 9 * x.shape[-1] * O)
    if mask is not None:
        gots, res = [t[mask] for t in gots], (res[mask] if res is not None else None)
    pre, unit = conv_ref64(x, w, b, mode, mask)
    ref, bound = epilogue_bound(pre, unit, dt, "res" if res is not None else "bias", res)
    return max(worst((t.detach().double().cpu() - ref).abs(), bound) for t in gots)


# (B, H, W, C, O, mode, residual, seeds x / w / b / res): test_conv3x3, test_conv3x3_on_256_tile_kernel (the 224 x 224 launches on the GPU only),
# test_conv3x3_stride2_downsample, test_conv3x3_halo_upsample
CONV_CASES = [(1, 16, 16, 64, 128, "plain", False, (20, 21, 22, 23)), (2, 8, 24, 128, 64, "plain", True, (20, 21, 22, 23)),
              (1, 16, 8, 64, 64, "ups", False, (20, 21, 22, 23)), (1, 32, 32, 128, 3, "plain", False, (20, 21, 22, 23)),
              (1, 40, 24, 64, 256, "plain", False, (20, 21, 22, 23)), (2, 16, 24, 128, 256, "plain", True, (20, 21, 22, 23)),
              (1, 12, 16, 64, 512, "ups", False, (20, 21, 22, 23)),
              (1, 16, 16, 64, 128, "s2", False, (24, 25, 26, None)), (2, 8, 24, 128, 64, "s2", False, (24, 25, 26, None)),
              (1, 64, 32, 64, 64, "s2", False, (24, 25, 26, None)), (2, 16, 24, 128, 256, "ups", False, (96, 97, 98, None))]


class ConvRestatement:
    def __init__(self, case, dt=BF, order="steps"):
        B, H, W, C, O, mode, has_res, (sx, sw, sb, sr) = case
        self.dt, self.mode, self.O, self.C = dt, mode, O, C
        self.x, self.w, self.b = inputs(dt, B, H, W, C, seed=sx), inputs(dt, O, 3, 3, C, seed=sw, scale=0.05), inputs(dt, O, seed=sb, scale=0.1)
        self.acc = conv_f32(self.x, self.w, self.b, mode, order)
        self.res = inputs(dt, *self.acc.shape, seed=sr) if has_res else None
        self.pre64, self.unit = conv_ref64(self.x, self.w, self.b, mode)
        self.epi = "res" if has_res else "bias"
        self.ref, self.bound = epilogue_bound(self.pre64, self.unit, dt, self.epi, self.res)

    def out(self, acc=None, res="same"):
        res = self.res if isinstance(res, str) else res
        return epilogue_f32(self.acc if acc is None else acc, self.dt, "res" if res is not None else "bias", res)

    def ratio(self, got):
        return worst((got.double() - self.ref).abs(), self.bound)

    def unit_error(self):
        return float(((self.acc.double() - self.pre64).abs() / self.unit).max())

    def m_border_wraps(self):
        """the halo / im2col gather (conv_halo.hip, gemm256v3 CONV = true): pixel (1, 0) reads its flat-index neighbour, the last pixel of the row above,
        where the tap at x - 1 is padding, for the first output-channel block"""
        acc, oc = self.acc.clone(), min(64, self.O)
        xs = self.x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) if self.mode == "ups" else self.x
        for ky in range(3):
            acc[0, 1, 0, :oc] += xs[0, 1 + ky - 1 - 1, -1] @ self.w[:oc, ky, 0].t() if 1 + ky - 2 >= 0 else 0.0
        return self.out(acc)

    def m_upsample_row(self):
        """the nearest-x2 view folded into the gather: output pixel (2, 2) reads source row y / 2 + 1 in every tap = the output of pixel (4, 2)"""
        acc = self.acc.clone()
        acc[0, 2, 2] = self.acc[0, 4, 2]
        return self.out(acc)

    def m_residual_missing(self):
        """the residual add of the tail skipped for the last pixel (a row limit one short)"""
        out = self.out()
        out[-1, -1, -1] = rnd(self.acc[-1, -1, -1], self.dt)
        return out

    def m_chunk_dropped(self):
        """the chunk loop (conv_halo.hip: 64-channel chunks; here the last 32 channels) ends one step early for the last row of 16 pixels"""
        acc, c0 = self.acc.clone(), self.C - 32
        taps = conv_taps(self.x, self.mode)
        n = min(16, acc.shape[2])
        for ky in range(3):
            for kx in range(3):
                acc[0, -1, :n] -= taps[ky][kx][0, -1, :n, c0:] @ self.w[:, ky, kx, c0:].t()
        return self.out(acc)

    def mutants(self):
        m = {"chunk dropped": self.m_chunk_dropped}
        if self.mode != "s2":
            m["border wraps"] = self.m_border_wraps
        if self.mode == "ups":
            m["upsample row + 1"] = self.m_upsample_row
        if self.res is not None:
            m["residual missing"] = self.m_residual_missing
        return m


# ---- per-row gates ---------------------------------------------------------------------------------------------------------------------------------
def row_ratio(got, ref, c_row, dt):
    """worst ||got_row - ref_row|| / (c_row ||ref_row|| + sqrt(L) sp(0)) over the rows (last dimension)"""
    got, ref = got.detach().double().cpu(), ref.double()
    floor = math.sqrt(ref.shape[-1]) * float(spacing(torch.zeros(1, dtype=torch.float64), dt))
    return worst(torch.linalg.norm(got - ref, dim=-1), c_row * torch.linalg.norm(ref, dim=-1) + floor)


def row_rel(got, ref):
    return float((torch.linalg.norm(got.double() - ref.double(), dim=-1) / torch.linalg.norm(ref.double(), dim=-1).clamp(min=1e-300)).max())


# c_row: twice the worst row of the fp32 restatement (output rounded) over the family's cases.  Measured worst rows:
#   attention bf16 D 64 / 128: 3.88e-3 ((2, 4, 4685, 64), last image; spiked keys <= 3.55e-3; 32- and 128-key tiles 3.75e-3 / 3.45e-3 where 64-key
#     tiles give 3.48e-3)             key split, partials rounded once more: 4.19e-3 (three ranges)
#   attention bf16 D 512: 3.15e-3 (T = 100)             attention float16: 4.39e-4 ((2, 3, 333, 64))
#   LN-modulate 1.88e-3 (bf16, h = 256) / 2.19e-4 (float16, h = 1536)
#   QKNorm + RoPE 2.91e-3 (bf16, D = 128: two roundings) / 4.14e-4 (float16)
#   GroupNorm (+ SiLU) per (image, group) 3.53e-3 (64 channels, 8 x 8: 128 values per group, rounded in front of SiLU and behind it); per
#     (image, channel) 4.45e-3 (512 channels, 8 x 8: 64 values per row)
C_ROW = {("attn", BF): 7.8e-3, ("attn_split", BF): 8.4e-3, ("attn512", BF): 6.3e-3, ("attn", F16): 8.8e-4, ("ln", BF): 3.8e-3, ("ln", F16): 4.4e-4,
         ("qk", BF): 5.9e-3, ("qk", F16): 8.3e-4, ("gn", BF): 7.1e-3, ("gn_channel", BF): 8.9e-3}


# attention
def attn_ref64(q, k, v, scale):
    """fp64 softmax(q k^T scale) v; q [G, Sq, D], k / v [G, Sk, D]"""
    out = torch.empty(q.shape, dtype=torch.float64)
    for i in range(q.shape[0]):
        out[i] = torch.softmax(q[i].double() @ k[i].double().t() * scale, dim=-1) @ v[i].double()
    return out


def flash_f32(q, k, v, scale, dt, tile=64, thr=4.0, no_rescale=None):
    """The kernels' tile loop in fp32 (attention2.hip DK2_TILE, attention4.hip, scripts/gen_attn5.py, attention512.hip; all four agree on the
    rounding points): scores in fp32, p = exp2(s c - m c) against a running maximum that moves only when a tile exceeds it by ``thr`` (deferred
    rescale), the row sum over the fp32 p, P rounded to the element type in front of P.V, fp32 accumulator.  Returns (o, l, m c) unnormalised.
    ``no_rescale`` = (group, row): that row's accumulator is not multiplied by the rescale factor (its row sum is)."""
    c = torch.tensor(scale * LOG2E, dtype=torch.float32)
    G, Sq, D = q.shape
    m = torch.full((G, Sq), -1e30)
    l, o = torch.zeros(G, Sq), torch.zeros(G, Sq, D)
    for j0 in range(0, k.shape[1], tile):
        s = q @ k[:, j0:j0 + tile].transpose(1, 2)
        mloc = s.amax(-1)
        m_new = torch.where(mloc - m > thr / scale, torch.maximum(m, mloc), m)
        alpha = torch.exp2((m - m_new) * c)
        l = l * alpha
        if no_rescale is not None and j0 > 0:
            alpha = alpha.clone()
            alpha[no_rescale] = 1.0
        o, m = o * alpha[..., None], m_new
        p = torch.exp2(s * c - (m * c)[..., None])
        l = l + p.sum(-1)
        o = o + rnd(p, dt) @ v[:, j0:j0 + tile]
    return o, l, m * c


def attn_f32(q, k, v, scale, dt, tile=64, ranges=1, unit_weight=None, no_rescale=None):
    """the restated kernel's output, rounded.  ``ranges`` > 1: attention5.hip's key-split jobs -- every key range (whole tiles) leaves its normalised
    partial rounded to the element type with (m c, l); dk_attn5_merge_kernel weights them with l 2^(mc_i - max mc).  ``unit_weight`` = (range,
    group, rows): that range merged with l alone there"""
    if ranges == 1:
        o, l, _ = flash_f32(q, k, v, scale, dt, tile, no_rescale=no_rescale)
        return rnd(o / l[..., None], dt)
    nt = (k.shape[1] + tile - 1) // tile
    cuts = [(nt * i // ranges) * tile for i in range(ranges)] + [k.shape[1]]
    parts = [flash_f32(q, k[:, a:b], v[:, a:b], scale, dt, tile) for a, b in zip(cuts[:-1], cuts[1:])]
    mx = torch.stack([p[2] for p in parts]).amax(0)
    acc, wsum = 0.0, 0.0
    for i, (o, l, mc) in enumerate(parts):
        e = torch.exp2(mc - mx)
        if unit_weight is not None and unit_weight[0] == i:
            e = e.clone()
            e[unit_weight[1], unit_weight[2]] = 1.0
        wgt = l * e
        acc, wsum = acc + wgt[..., None] * rnd(o / l[..., None], dt), wsum + wgt
    return rnd(acc / wsum[..., None], dt)


def split_qkv(qkv, H, D, heads=None):
    """[B, S, 3 H D] -> q, k, v [B H', S, D] (``heads``: the first ones only)"""
    B, S, _ = qkv.shape
    h, hs = H * D, heads or H
    return tuple(qkv[..., i * h:i * h + hs * D].reshape(B, S, hs, D).permute(0, 2, 1, 3).reshape(B * hs, S, D) for i in range(3))


def attn_gate(got, qkv, H, D, dt, heads=None, images=None, family="attn"):
    """worst row ratio of an attention output [B, S, H D], or of several (a list: one reference; ``family`` then a list too), against fp64, over
    ``images`` (default all) and the first ``heads`` heads"""
    B, S, _ = qkv.shape
    images = list(range(B)) if images is None else images
    hs = heads or H
    q, k, v = split_qkv(qkv[images], H, D, hs)
    ref = attn_ref64(q, k, v, 1.0 / math.sqrt(D))
    gots, fams = (got, family) if isinstance(got, (list, tuple)) else ([got], [family])
    fams = [fams] * len(gots) if isinstance(fams, str) else fams
    ys = [t.detach().float().cpu()[images][..., :hs * D].reshape(len(images), S, hs, D).permute(0, 2, 1, 3).reshape(-1, S, D) for t in gots]
    return max(row_ratio(y, ref, C_ROW[(f, dt)], dt) for y, f in zip(ys, fams))


def attn_gate_images(B, S):
    """at S >= 4000 the fp64 reference is formed for the last image only"""
    return [B - 1] if S >= 4000 else None


def attn_gate_heads(H, S):
    """... and for the first two heads (four below)"""
    return min(H, 2 if S >= 4000 else 4)


def _attn_case(name, B, H, S, D, seed, scale=1.0, dt=BF, spikes=(), ranges=1, heads=None):
    return dict(name=name, B=B, H=H, S=S, D=D, seed=seed, scale=scale, dt=dt, spikes=spikes, ranges=ranges, heads=heads)


# spikes: (key, query, head, factor): key row = factor x query row of that head (the tests' own lines)
ATTN_CASES = (
    [_attn_case(f"attention {B}x{H}x{S}x{D}", B, H, S, D, 30, heads=attn_gate_heads(H, S))
     for B, H, S, D in ((1, 2, 128, 128), (1, 3, 200, 128), (2, 4, 333, 64), (1, 24, 1088, 128), (2, 24, 653, 64), (2, 4, 4685, 64), (2, 3, 2065, 128),
                        (1, 2, 2304, 128), (1, 2, 397, 64), (1, 2, 2321, 128))]
    + [_attn_case(f"variants {B}x{H}x{S}x{D}", B, H, S, D, 32)
       for B, H, S, D in ((1, 2, 333, 128), (2, 3, 700, 64), (1, 2, 64, 128), (1, 2, 100, 64), (1, 2, 128, 128), (1, 2, 129, 128), (1, 2, 192, 128), (1, 2, 250, 128),
                          (1, 3, 1088, 128), (2, 2, 653, 64), (1, 2, 64, 64), (1, 2, 128, 64), (1, 2, 129, 64), (1, 2, 192, 64), (1, 3, 1119, 64),
                          (1, 2, 397, 64), (1, 2, 2321, 128))]
    + [_attn_case(f"attention5 {B}x{H}x{S}", B, H, S, 128, 33, heads=min(3, attn_gate_heads(H, S))) for B, H, S in ((1, 2, 768), (2, 3, 1024), (1, 2, 2304), (1, 24, 4352))]
    + [_attn_case(f"key split {n}", 1, 2, 3072, 128, 34, 0.7, spikes=((3000, 77, 0, 5.0),), ranges=n) for n in (2, 3, 4)]
    + [_attn_case("attention5 spiked", 1, 1, 1024, 128, 31, 0.5, spikes=((700, 7, 0, 6.0), (1023, 300, 0, 6.0))),
       _attn_case("spiked D128", 1, 1, 320, 128, 31, 0.5, spikes=((250, 7, 0, 6.0),)),
       _attn_case("spiked D64", 1, 2, 400, 64, 33, 0.5, spikes=((330, 9, 0, 8.0),)),
       _attn_case("f16 ragged", 2, 3, 333, 64, 80, dt=F16),
       _attn_case("f16 spiked", 1, 2, 400, 64, 33, 0.5, dt=F16, spikes=((330, 9, 0, 8.0),))])


def attn_qkv(c):
    B, H, S, D, dt = c["B"], c["H"], c["S"], c["D"], c["dt"]
    h = H * D
    qkv = inputs(dt, B, S, 3 * h, seed=c["seed"], scale=c["scale"])
    for key, qr, hd, f in c["spikes"]:
        qkv[0, key, h + hd * D:h + (hd + 1) * D] = rnd(qkv[0, qr, hd * D:(hd + 1) * D] * f, dt)
    return qkv


class AttnRestatement:
    """groups = (image, head) pairs: the last image at S >= 4000, the first ``heads`` heads"""

    def __init__(self, c, tile=64, qkv3=None):
        self.c, self.dt, self.tile = c, c["dt"], tile
        B, H, S, D = c["B"], c["H"], c["S"], c["D"]
        if qkv3 is None:
            qkv = attn_qkv(c)
            imgs = attn_gate_images(B, S) or list(range(B))
            self.q, self.k, self.v = split_qkv(qkv[imgs], H, D, c["heads"])
        else:
            self.q, self.k, self.v = qkv3
        self.S, self.D, self.scale = S, D, 1.0 / math.sqrt(D)
        self.ref = attn_ref64(self.q, self.k, self.v, self.scale)
        self.base = self.f32()

    def f32(self, g=slice(None), rows=slice(None), keys=slice(None), **kw):
        return attn_f32(self.q[g, rows], self.k[g, keys], self.v[g, keys], self.scale, self.dt, self.tile, self.c["ranges"], **kw)

    def ratio(self, got):
        family = "attn_split" if self.c["ranges"] > 1 else "attn512" if self.D == 512 else "attn"
        return row_ratio(got, self.ref, C_ROW[(family, self.dt)], self.dt)

    def last_block(self):
        return slice((self.S - 1) // 64 * 64, self.S)

    def m_last_key_dropped(self):
        """the key mask of the last tile (DK4_MASK, attention2.hip's ``key >= S`` select) one key short, for the last query block of the last head"""
        out, g, r = self.base.clone(), slice(self.q.shape[0] - 1, self.q.shape[0]), self.last_block()
        out[g, r] = self.f32(g, r, slice(0, self.S - 1))
        return out

    def m_ragged_tile_dropped(self):
        """nsteps = S / 64 instead of ceil: the ragged last key tile never visited by one wave's 32 queries of the first head"""
        out, g, r = self.base.clone(), slice(0, 1), slice(0, 32)
        out[g, r] = self.f32(g, r, slice(0, self.S // 64 * 64))
        return out

    def m_row_from_neighbour(self):
        """the output store (lane owns query q0 + l31): one row written with its neighbour's values"""
        out, r = self.base.clone(), min(self.S - 2, 37)
        out[0, r] = self.base[0, r + 1]
        return out

    def m_rows_scaled(self):
        """the row sum of one 64-query block off by one part in 64 (a psum lane left out of the __shfl_xor fold)"""
        r0 = max(0, min(64, self.S - 64))  # (the second 64-query block where there is one)
        out, r = self.base.clone(), slice(r0, r0 + 64)
        out[0, r] = rnd(self.base[0, r] * (1.0 + 1.0 / 64.0), self.dt)
        return out

    def m_no_rescale(self):
        """guide rule 26: the accumulator of the spiked query not multiplied by the rescale factor when the maximum moves (its row sum is)"""
        _, qr, hd, _ = self.c["spikes"][0]
        out = self.base.clone()
        out[hd, qr:qr + 1] = attn_f32(self.q[hd:hd + 1, qr:qr + 1], self.k[hd:hd + 1], self.v[hd:hd + 1], self.scale, self.dt, self.tile,
                                      no_rescale=(0, 0))[0]
        return out

    def m_merge_unit_weight(self):
        """dk_attn5_merge_kernel: the first key range of the first head's first 256-query block merged with l alone instead of l 2^(mc_i - max mc)"""
        out = self.base.clone()
        out[0:1, :256] = self.f32(slice(0, 1), slice(0, 256), unit_weight=(0, 0, slice(None)))
        return out

    def mutants(self):
        m = {"last key dropped": self.m_last_key_dropped, "row from neighbour": self.m_row_from_neighbour}
        if self.c["ranges"] == 1:  # (under the key split's wider bound, 8.4e-3 for its second rounding, 1 / 64 is 1.9 x to 2.0 x: not claimed there)
            m["64 rows x (1 + 1/64)"] = self.m_rows_scaled
        if self.S % 64:
            m["ragged key tile dropped"] = self.m_ragged_tile_dropped
        if self.c["spikes"] and self.c["ranges"] == 1:
            m["spiked row not rescaled"] = self.m_no_rescale
        if self.c["ranges"] > 1:
            m["merge weight 1"] = self.m_merge_unit_weight
        return m


# D = 512 (attention512.hip): single head, separate q / k / v, seeds 34 / 35 / 36; the spiked case of test_attention_d512_spiked_key
D512_CASES = [(1, 64), (2, 96), (1, 100), (1, 1000), (1, 1001), (2, 4096), "spiked"]


def d512_operands(case):
    if case == "spiked":
        q, k, v = (randn(1, 320, 512, seed=s, scale=0.5) for s in (37, 38, 39))
        k[0, 250] = rnd(q[0, 7] * 6.0, BF)
        return q, k, v, dict(_attn_case("d512 spiked", 1, 1, 320, 512, 37, spikes=((250, 7, 0, 6.0),)))
    B, T = case
    q, k, v = (randn(B, T, 512, seed=s) for s in (34, 35, 36))
    return q, k, v, dict(_attn_case(f"d512 {B}x{T}", B, 1, T, 512, 34))


def d512_gate(got, q, k, v, images=None):
    """(at T >= 4000 the fp64 reference is formed for the last image only)"""
    images = (attn_gate_images(q.shape[0], q.shape[1]) or list(range(q.shape[0]))) if images is None else images
    ref = attn_ref64(q[images], k[images], v[images], 1.0 / math.sqrt(512))
    return row_ratio(got.detach().float().cpu()[images], ref, C_ROW[("attn512", BF)], BF)


# LN-modulate
# (dt, B, S, h, seeds[, (sigma, mean)]): x = 3 N(0, 1) + 0.5 as in test_ln_modulate / test_ln_modulate_f16; the last two: rows at mean / sigma 16
# (test_ln_modulate_large_mean*), where a channel left out of the mean shows -- on the tests' own rows it moves the result by less than the rounding
LN_CASES = [(BF, 1, 100, 256, (40, 41, 42)), (BF, 2, 77, 1536, (40, 41, 42)), (BF, 1, 300, 3072, (40, 41, 42)), (BF, 1, 5, 2432, (40, 41, 42)),
            (F16, 2, 77, 1536, (90, 91, 92)), (F16, 2, 77, 2432, (90, 91, 92)),
            (BF, 1, 5, 2432, (43, 44, 45), (0.5, 8.0)), (F16, 1, 5, 2432, (93, 94, 95), (0.5, 8.0))]


def ln_operands(case):
    dt, B, S, h, (sx, ss, sc) = case[:5]
    sigma, mean = case[5] if len(case) > 5 else (3.0, 0.5)
    x = rnd(inputs(dt, B, S, h, seed=sx, scale=sigma) + mean, dt)
    return x, inputs(dt, B, h, seed=ss), inputs(dt, B, h, seed=sc, scale=0.5)


def ln_weight(scale, dt):
    return rnd(torch.tensor(1.0, dtype=torch.float32) + scale, dt)


def ln_ref64(x, shift, scale, dt):
    """fp64 LayerNorm x round(1 + scale) + shift (the weight's rounding is the one the kernel and the reference share)"""
    xd = x.double()
    mu = xd.mean(-1, keepdim=True)
    y = (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(-1, keepdim=True) + 1e-6)
    return y * ln_weight(scale, dt).double()[:, None] + shift.double()[:, None]


def ln_f32(x, shift, scale, dt, mean_over=None):
    """fp32 two-pass LayerNorm, one output rounding.  ``mean_over`` = (image, row, n): that row's mean over its first n channels only"""
    mu = x.mean(-1, keepdim=True)
    if mean_over is not None:
        b, r, n = mean_over
        mu = mu.clone()
        mu[b, r] = x[b, r, :n].sum() / x.shape[-1]
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return rnd((x - mu) * torch.rsqrt(var + 1e-6) * ln_weight(scale, dt)[:, None] + shift[:, None], dt)


def ln_gate(got, x, shift, scale, dt):
    return row_ratio(got, ln_ref64(x, shift, scale, dt), C_ROW[("ln", dt)], dt)


def ln_mutants(case):
    dt, B, S, h = case[:4]
    x, shift, scale = ln_operands(case)
    m = {}
    if B > 1:
        def other_shift():
            """elementwise.hip ln_modulate: the image index of one row (the last of image 0) off by one -- it takes image 1's shift"""
            out = ln_f32(x, shift, scale, dt)
            out[0, -1] = ln_f32(x[0:1, -1:], shift[1:2], scale[0:1], dt)[0, 0]
            return out
        m["other image's shift"] = other_shift
    if h == 2432 and len(case) > 5:
        def mean_tail():
            """h = 2432 = 38 x 64: the last 8 channels (the partial vector of the last 64-lane chunk) left out of one row's mean"""
            return ln_f32(x, shift, scale, dt, mean_over=(0, 1, h - 8))
        m["last 8 channels not in the mean"] = mean_tail
    return m


# QKNorm + RoPE: (dt, D, norm, rope, axes) on qkv [2, 5 + 4 x 6, 3 x 3 D], seeds as test_qk_norm_rope / test_qk_norm_rope_f16
QK_CASES = [(BF, 128, True, True, (16, 56, 56), (50, 51, 52)), (BF, 64, True, False, None, (50, 51, 52)), (BF, 128, False, True, (16, 56, 56), (50, 51, 52)),
            (F16, 64, True, True, (16, 24, 24), (93, 94, 95))]
QK_B, QK_H, QK_ST, QK_GH, QK_GW = 2, 3, 5, 4, 6


def rope_table64(S_t, gh, gw, axes, theta=10000.0):
    """cos / sin [S, D / 2, 2] in fp64: text positions zero, image tokens (0, row, col)"""
    S = S_t + gh * gw
    pos = torch.zeros(S, 3, dtype=torch.float64)
    pos[S_t:, 1] = torch.arange(gh, dtype=torch.float64)[:, None].expand(gh, gw).reshape(-1)
    pos[S_t:, 2] = torch.arange(gw, dtype=torch.float64)[None, :].expand(gh, gw).reshape(-1)
    outs = []
    for i, dim in enumerate(axes):
        ang = pos[:, i:i + 1] * (1.0 / theta ** (torch.arange(0, dim, 2, dtype=torch.float64) / dim))[None]
        outs.append(torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1))
    return torch.cat(outs, dim=1)


def qk_operands(case):
    dt, D, norm, rope, axes, (s0, s1, s2) = case
    S, h = QK_ST + QK_GH * QK_GW, QK_H * D
    qkv = inputs(dt, QK_B, S, 3 * h, seed=s0)
    qw, kw = rnd(1 + randn(D, seed=s1, scale=0.1), dt), rnd(1 + randn(D, seed=s2, scale=0.1), dt)
    tab = rope_table64(QK_ST, QK_GH, QK_GW, axes) if rope else None
    return qkv, (qw if norm else None), (kw if norm else None), tab


def qk_apply(t, w, tab, dt, f64, pairs="adjacent", mid_round=True):
    """RMSNorm (x w, rounded to the element type: the kernel's and the reference's shared rounding point) then RoPE on t [B, S, H, D]; fp64 or fp32"""
    t = t.double() if f64 else t
    if w is not None:
        ms = (t * t).mean(-1, keepdim=True)
        t = t * (1.0 / torch.sqrt(ms + 1e-6) if f64 else torch.rsqrt(ms + 1e-6)) * (w.double() if f64 else w)
        if mid_round and not f64:
            t = rnd(t, dt)
    if tab is not None:
        tb = tab if f64 else tab.to(torch.float32)
        c, s = tb[None, :, None, :, 0], tb[None, :, None, :, 1]
        if pairs == "adjacent":
            xe, xo = t[..., 0::2], t[..., 1::2]
            t = torch.stack([c * xe - s * xo, s * xe + c * xo], dim=-1).flatten(-2)
        else:
            half = t.shape[-1] // 2
            xe, xo = t[..., :half], t[..., half:]
            t = torch.cat([c * xe - s * xo, s * xe + c * xo], dim=-1)
    return t


def qk_ref64(qkv, qw, kw, tab, D):
    """fp64 q | k columns [B, S, 2 H, D] (rows = (image, token, head))"""
    B, S, _ = qkv.shape
    H = qkv.shape[-1] // (3 * D)
    h = H * D
    return torch.cat([qk_apply(qkv[..., i * h:(i + 1) * h].reshape(B, S, H, D), w, tab, None, True) for i, w in ((0, qw), (1, kw))], dim=2)


def qk_f32(qkv, qw, kw, tab, D, dt, table_shift=None, q_head_weight=None, half_pairs=None):
    """the fp32 restatement, rounded [B, S, 2 H, D].  Faults: ``table_shift`` = token whose table row is position + 1; ``q_head_weight`` = query head
    normalised with the key weight; ``half_pairs`` = head rotated over pairs (i, i + D / 2)"""
    B, S, _ = qkv.shape
    H = qkv.shape[-1] // (3 * D)
    h = H * D
    outs = []
    for i, w in ((0, qw), (1, kw)):
        t = qkv[..., i * h:(i + 1) * h].reshape(B, S, H, D)
        tb = tab
        if table_shift is not None:
            tb = tab.clone()
            tb[table_shift] = tab[table_shift + 1]
        o = rnd(qk_apply(t, w, tb, dt, False), dt)
        if i == 0 and q_head_weight is not None:
            o[:, :, q_head_weight] = rnd(qk_apply(t[:, :, q_head_weight:q_head_weight + 1], kw, tb, dt, False), dt)[:, :, 0]
        if half_pairs is not None:
            o[:, :, half_pairs] = rnd(qk_apply(t[:, :, half_pairs:half_pairs + 1], w, tb, dt, False, pairs="halves"), dt)[:, :, 0]
        outs.append(o)
    return torch.cat(outs, dim=2)


def qk_gate(got_qk, qkv, qw, kw, tab, D, dt):
    """got_qk: the q | k columns [B, S, 2 H D] the kernel left"""
    B, S, _ = qkv.shape
    ref = qk_ref64(qkv, qw, kw, tab.double().cpu() if tab is not None else None, D)
    return row_ratio(got_qk.detach().float().cpu().reshape(ref.shape), ref, C_ROW[("qk", dt)], dt)


def qk_mutants(case):
    dt, D, norm, rope, _, _ = case
    qkv, qw, kw, tab = qk_operands(case)
    m = {}
    if rope:
        m["table row of position + 1"] = lambda: qk_f32(qkv, qw, kw, tab, D, dt, table_shift=QK_ST + QK_GW - 1)  # elementwise.hip: the table row index
        m["pairs (i, i + D/2)"] = lambda: qk_f32(qkv, qw, kw, tab, D, dt, half_pairs=1)  # the rotate-half convention instead of adjacent pairs
    if norm:
        m["key weight on a query head"] = lambda: qk_f32(qkv, qw, kw, tab, D, dt, q_head_weight=2)  # the q / k select of the weight pointer
    return m


# GroupNorm (+ SiLU), rows = (image, group): (C, G, (H, W), silu), B = 2, seeds 60 / 61 / 62
GN_CASES = [(64, 32, (8, 8), True), (128, 32, (16, 16), False), (512, 32, (8, 8), True), (256, 32, (32, 32), True)]


def gn_operands(case):
    C, G, HW, silu = case
    x = rnd(randn(2, HW[0], HW[1], C, seed=60, scale=2.0) + 0.7, BF)
    return x, rnd(1 + randn(C, seed=61, scale=0.1), BF), randn(C, seed=62, scale=0.1)


def gn_rows(y, G):
    """[B, H, W, C] -> [B, G, H W C / G]"""
    B, H, W, C = y.shape
    return y.reshape(B, H * W, G, C // G).permute(0, 2, 1, 3).reshape(B, G, -1)


def gn_apply(x, gamma, beta, G, silu, dt, f64, no_beta_from=None, no_silu=None):
    """two-pass GroupNorm (fp64, or fp32 with the output rounded to the element type in front of SiLU and behind it).  Faults: ``no_beta_from`` =
    first channel of a tail without beta; ``no_silu`` = group left without SiLU"""
    B, H, W, C = x.shape
    xs = gn_rows(x.double() if f64 else x, G)                                   # [B, G, L]
    cpg = C // G
    mean = xs.mean(-1, keepdim=True)
    var = ((xs - mean) ** 2).mean(-1, keepdim=True)
    g_, b_ = (gamma.double(), beta.double()) if f64 else (gamma, beta.clone())
    if no_beta_from is not None:
        b_ = b_.clone()
        b_[no_beta_from:] = 0.0
    ga = g_.reshape(G, 1, cpg).expand(G, H * W, cpg).reshape(1, G, -1)
    be = b_.reshape(G, 1, cpg).expand(G, H * W, cpg).reshape(1, G, -1)
    y = (xs - mean) / torch.sqrt(var + 1e-5) * ga + be
    if not f64:
        y = rnd(y, dt)
    if silu:
        z = y * torch.sigmoid(y)
        z = z if f64 else rnd(z, dt)
        if no_silu is not None:
            z[:, no_silu] = y[:, no_silu]
        y = z
    return y


def gn_ratio(got_rows, ref_rows, cpg, dt=BF):
    """worst of the (image, group) rows and the (image, channel) rows; both [B, G, pixels x cpg] in"""
    B, G, L = ref_rows.shape
    ch = lambda t: t.reshape(B, G, L // cpg, cpg).permute(0, 1, 3, 2).reshape(B, G * cpg, L // cpg)  # noqa: E731
    return max(row_ratio(got_rows, ref_rows, C_ROW[("gn", dt)], dt), row_ratio(ch(got_rows), ch(ref_rows), C_ROW[("gn_channel", dt)], dt))


def gn_gate(got, x, gamma, beta, G, silu, dt=BF):
    return gn_ratio(gn_rows(got.detach().float().cpu(), G), gn_apply(x, gamma, beta, G, silu, dt, True), x.shape[-1] // G, dt)


def gn_stats_ratio(tab, x, gamma, beta, G):
    """A statistic that misses one pixel of 64 ... 1024 moves the normalised output by less than its rounding: no gate on the output sees it.  The
    statistics are gated where they are stored, in the (scale | shift) table [B, 2, C], with the relative rstd bound of tests/_numeric_range.py
    (2 E32 + 1e-6, E32 measured there on a literal fp32 two-pass).  Returns the worst of rstd error / bound and shift error / bound"""
    mean, var = NR.gn_stats64(x, G)
    _, e_scale, e_shift = NR.gn_table_check(tab, mean, var, gamma, beta, G)
    return max(e_scale / NR.GN_RSTD_BOUND, e_shift)


def gn_table_mutant(x, gamma, beta, G, group=3):
    """the statistics pass's chunk loop one pixel short for one group (a ragged last chunk dropped): the table built from those statistics"""
    mean, var = NR.gn_stats64(x, G)
    cpg = x.shape[-1] // G
    v = x[..., group * cpg:(group + 1) * cpg].reshape(x.shape[0], -1, cpg)[:, :-1].reshape(x.shape[0], -1).double()
    mean[:, group], var[:, group] = v.mean(1), ((v - v.mean(1, keepdim=True)) ** 2).mean(1)
    return NR.gn_table64(mean, var, gamma, beta, G).to(torch.float32)


def gn_mutants(case):
    C, G, HW, silu = case
    x, gamma, beta = gn_operands(case)
    # elementwise.hip's GroupNorm apply reads gamma / beta as 16-byte vectors: the last vector (8 channels) without beta.  (The last channel alone: its
    # beta is 0.1 N(0, 1) from seed 62 and at two of the four shapes so small that the row stays inside the rounding of a correct result -- 1.5 and
    # 0.95 of the bound; a fault of that size cannot be told from a correct kernel on this input, by any gate.)
    m = {"beta missing on the last 8 channels": lambda: gn_apply(x, gamma, beta, G, silu, BF, False, no_beta_from=C - 8)}
    if silu:
        m["SiLU skipped on one group"] = lambda: gn_apply(x, gamma, beta, G, silu, BF, False, no_silu=G - 1)  # the apply pass's silu flag per group
    return m
