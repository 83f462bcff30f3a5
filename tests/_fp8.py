"""Test-side restatement of the MX scale side-array layout (diffusionkit_amd/csrc/dk_common.h: dk_mx_scale_index), so that the
parity tests can build / read the arrays the fp8 GEMM consumes without going through the library that is under test."""
import torch


def n_blk128(rows: int) -> int:
    return (rows + 127) // 128 + 1


def scale_index(r: torch.Tensor, kb: torch.Tensor, nblk: int) -> torch.Tensor:
    """byte position of the scale of (physical row r, 32-column block kb): [kb / 4][r / 128][kb % 4][r % 16][(r / 16) % 8]"""
    return ((((kb >> 2) * nblk + (r >> 7)) * 64 + (kb & 3) * 16 + (r & 15)) << 3) + ((r >> 4) & 7)


def scales_to_array(e: torch.Tensor, rows: int = None) -> torch.Tensor:
    """E8M0 bytes [M, K / 32] -> the side array (uint8, dk_mx_scale_bytes(rows, K) bytes) of a buffer with ``rows`` rows."""
    M, KB = e.shape
    rows = M if rows is None else rows
    nblk = n_blk128(rows)
    arr = torch.zeros(((KB * 32 + 127) // 128) * nblk * 512, dtype=torch.uint8)
    r = torch.arange(M)[:, None].expand(M, KB)
    kb = torch.arange(KB)[None, :].expand(M, KB)
    arr[scale_index(r, kb, nblk).reshape(-1)] = e.reshape(-1).cpu()
    return arr


def array_to_scales(arr: torch.Tensor, M: int, K: int, rows: int = None, row0: int = 0, col0: int = 0) -> torch.Tensor:
    """the scales of rows [row0, row0 + M), columns [col0, col0 + K) of a buffer whose side array is ``arr``"""
    rows = M if rows is None else rows
    nblk = n_blk128(rows)
    KB = K // 32
    r = (row0 + torch.arange(M))[:, None].expand(M, KB)
    kb = (col0 // 32 + torch.arange(KB))[None, :].expand(M, KB)
    return arr.cpu()[scale_index(r, kb, nblk).reshape(-1)].reshape(M, KB)


def fp8_activation(M, K, seed):
    """the activation of the fp8 / fp4 GEMM tests: bf16 N(0, 1), the first half of K scaled by 4 (block scales that differ along a row)"""
    from tests._util import bf16r, randn
    a = bf16r(randn(M, K, seed=seed, scale=1.0))
    a[:, :K // 2] *= 4.0
    return a


def fp8_problem(M, N, K, seed, w_pitch=None):
    """(a, e4m3 bytes of a, its E8M0 scales, e4m3 weight bytes [N, w_pitch or K], wscale, dequantised a, dequantised w): activations through
    oracle/fp8.py mx8_encode, weights at 0.02 through the product quantiser (diffusionkit_amd/weights.py: the format's definition)"""
    from diffusionkit_amd.weights import dequantize_weight_e4m3, quantize_weight_e4m3
    from oracle import fp8 as o8
    from tests._util import BF, randn
    a = fp8_activation(M, K, seed)
    w = (randn(N, K, seed=seed + 1, scale=0.02)).to(BF)
    qa, ea = o8.mx8_encode(a)
    qw, ws = quantize_weight_e4m3(w)
    a_dq = mx8_decode(qa, ea)
    w_dq = dequantize_weight_e4m3(qw, ws)
    if w_pitch:
        wp = torch.zeros(N, w_pitch, dtype=torch.uint8)
        wp[:, :K] = qw
        qw = wp
    return a, qa, ea, qw, ws, a_dq, w_dq


def mx8_decode(q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """e4m3 bytes [M, K] + E8M0 bytes [M, K / 32] -> fp32 values"""
    M, K = q.shape
    v = q.cpu().view(torch.float8_e4m3fn).to(torch.float32).reshape(M, K // 32, 32)
    return (v * torch.ldexp(torch.ones(M, K // 32, 1), e.cpu().to(torch.int32)[..., None] - 127)).reshape(M, K)


class GemmProblem:
    """One problem of the block-scaled GEMMs on the device (``kind`` "fp8": ops.gemm_fp8, "fp4": ops.gemm_fp4), seed M + N + K, bias seed 5; launched
    bias-only (``run``) or with one gate row (seed 6) and a residual (seed 7) in the tail (``run_res``), each with its per-element gate of
    tests/_gates.py on the dequantised operands.  ``w``: a bf16 weight instead of the seeded one (fp4)."""

    def __init__(self, kind, dev, M, N, K, w_pitch=None, w=None):
        from tests._util import BF, randn
        self.kind, self.dev, self.M, self.N, self.K = kind, dev, M, N, K
        if kind == "fp4":
            from tests import _mxfp4 as f4
            qa, ea, w4, sw, ws, self.w_dq, self.a_dq = f4.fp4_problem(M, N, K, seed=M + N + K, w_pitch=w_pitch, w=w)
            weight = (w4.to(dev), sw.to(dev), ws.to(dev))
        else:
            _, qa, ea, qw, ws, self.a_dq, self.w_dq = fp8_problem(M, N, K, seed=M + N + K, w_pitch=w_pitch)
            weight = (qw.to(dev), ws.to(dev))
        self.bias, self.gate, self.res = randn(N, seed=5, scale=0.5), randn(1, N, seed=6), randn(M, N, seed=7)
        rows = (M + 127) // 128 * 128
        a8 = torch.zeros(rows, K, dtype=torch.uint8)
        a8[:M] = qa
        self.args = (a8.to(dev), scales_to_array(ea, rows).to(dev)) + weight
        self.ref = (self.a_dq.double() @ self.w_dq.double().t() + self.bias.double()).float()
        self.dev_tail = dict(bias=self.bias.to(dev, BF), gate=self.gate.to(dev, BF), res=self.res.to(dev, BF))

    def _launch(self, **kw):
        from diffusionkit_amd import ops
        return (ops.gemm_fp4 if self.kind == "fp4" else ops.gemm_fp8)(*self.args, M=self.M, k=self.K, **kw).float().cpu()

    def run(self, **extra):
        return self._launch(bias=self.dev_tail["bias"], **extra)

    def run_res(self, **extra):
        from diffusionkit_amd._lib import DK_EPI_GATE_RES
        return self._launch(epilogue=DK_EPI_GATE_RES, gate_seg_len=self.M, **self.dev_tail, **extra)

    def gate_bias(self, what, y, missed):
        from tests import _gates as G
        G.assert_gate(f"{self.kind} bias {self.M}x{self.N}x{self.K} {what}".rstrip(), G.qgemm_gate(y, self.a_dq, self.w_dq, self.bias), missed)

    def gate_res(self, what, y):
        from tests import _gates as G
        G.assert_gate(f"{self.kind} gate_res {self.M}x{self.N}x{self.K} {what}".rstrip(),
                      G.qgemm_gate(y, self.a_dq, self.w_dq, self.bias, "gate_res", self.res, self.gate))

    def k_split(self, run, split_min, force):
        """(cut, whole) of ``run`` with and without the K-split workspace; ``force``: `gemm_split` 1 beside the lowered `gemm_split_min`.  The cut is
        witnessed by what the producers left in the slabs (fp4 x fp8 products have 6 significant bits: most partial sums are exact in fp32 and the
        two results may agree in every bit); the flag region is left zero"""
        from diffusionkit_amd import ops
        wsp = ops.gemm_workspace(self.dev)
        y0 = run()
        wsp[:-4096].zero_()
        ops.tune("gemm_split_min", split_min)
        if force:
            ops.tune("gemm_split", 1)
        try:
            y = run(workspace=wsp)
        finally:
            ops.tune("gemm_split", -1)
            ops.tune("gemm_split_min", -1)
        assert bool(wsp[:-4096].any()), "the launch was expected to be cut along K (the producers write their accumulators into the workspace)"
        assert float((y0 != y).float().mean()) < 0.05
        assert int(wsp[-4096:].sum()) == 0
        return y, y0
