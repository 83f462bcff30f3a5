"""The emulation of csrc/attention_f8.hip the tests gate it with: a float64 attention on the values the kernel's MX-fp8 operands represent (plain
torch, no GPU; built from oracle/fp8.py's format definition, nothing from csrc/)."""
import torch

from oracle import fp8 as o8

LOG2E, TILE, THR, LIFT = 1.4426950408889634, 128, 4.0, 3


def emulate(q, k, v, scale):
    """q (behind norm / RoPE) / k / v [G, S, D] -> float64 [G, S, D].  Q times scale * log2 e and K are rounded to MX-fp8 along D, V along the key
    axis (blocks of 32 consecutive keys from key 0; the padding of the last block is zero and moves no maximum); the walk over 128-key tiles keeps
    the kernel's running maximum with the deferred rescale (threshold 4 in natural units), because the offset decides where P = exp2(s - m) is
    rounded: to e4m3 of p * 2^3.  The row sum is taken over the unrounded p; everything else is float64."""
    G, S, D = q.shape
    Sp = (S + TILE - 1) // TILE * TILE
    q8, k8 = o8.mx8_fake_quant(q.float() * (scale * LOG2E)).double(), o8.mx8_fake_quant(k.float()).double()
    vp = torch.zeros(G, Sp, D)
    vp[:, :S] = v.float()
    v8 = o8.mx8_fake_quant(vp.transpose(1, 2).contiguous()).transpose(1, 2).double()
    s = q8 @ k8.transpose(1, 2)
    m = torch.full((G, S, 1), -float("inf"), dtype=torch.float64)
    l, o = torch.zeros(G, S, 1, dtype=torch.float64), torch.zeros(G, S, D, dtype=torch.float64)
    for j0 in range(0, S, TILE):
        st = s[:, :, j0:j0 + TILE]
        mx = st.amax(-1, keepdim=True)
        m_new = torch.where(mx - m > THR * LOG2E, torch.maximum(m, mx), m)
        alpha = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - m_new))
        m = m_new
        p = torch.exp2(st - m)
        p8 = (p * 2.0 ** LIFT).float().to(torch.float8_e4m3fn).double() / 2.0 ** LIFT
        l, o = l * alpha + p.sum(-1, keepdim=True), o * alpha + p8 @ v8[:, j0:j0 + st.shape[-1]]
    return o / l
