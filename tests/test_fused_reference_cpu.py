"""CPU check behind one bound of tests/test_gpu_fused_ops.py: the fused QKNorm + RoPE tail of the GEMMs sums a head's squares in another order than the
stand-alone pass does, and the test caps the share of elements in which the two device paths may differ at 1 %.  That cap is a condition, not a
measurement: an fp32 reordering moves the row's rsqrt by ~1e-7 relative, which flips a bf16 rounding with probability ~1e-7 / 2^-8 = 3e-5 per element.
Here the emulating oracle itself is run with the squares summed first-to-last and last-to-first on the inputs the GPU cases use."""
import pytest
import torch

from oracle.mmdit import Prec
from tests import _fused_cases as fc
from tests._util import BF, bf16r

SHARE_CAP = fc.SHARE_CAP


@pytest.mark.parametrize("case", [c for c in fc.KNORM_CASES if c["id"] in ("v3_mf8_fast", "v3_d64", "v4_dense_wrap_300", "v3_no_table")],
                         ids=lambda c: c["id"])
def test_reordered_square_sum_stays_under_the_share_cap(case):
    t = fc.knorm_inputs(case)
    proj = bf16r(t["A"] @ t["W"].t() + t["bias"])
    fwd, rev = (fc.knorm_oracle(case, t, proj, Prec(BF), order) for order in ("fwd", "rev"))
    own = fc.knorm_oracle(case, t, proj, Prec(BF))
    share = float((fwd != rev).float().mean())
    share_own = float((fwd != own).float().mean())
    print(f"[{case['id']}] elements that differ: first-to-last against last-to-first {share:.2e}, against the oracle's own mean {share_own:.2e}")
    assert share < SHARE_CAP / 10 and share_own < SHARE_CAP / 10
    # and a flip is one bf16 ulp of one partner of a rotated couple: far inside the per-element bound of the GPU test
    h, D = case["h"], case["D"]
    heads = own[:, :2 * h].reshape(own.shape[0], -1, D).abs().amax(dim=-1, keepdim=True)
    d = (fwd - rev)[:, :2 * h].reshape(own.shape[0], -1, D).abs()
    assert bool((d <= fc.HEAD_BOUND * heads).all())
