"""FLUX IP-Adapter for the parity tests: the CPU oracle of a FLUX model with the adapter's decoupled image-prompt attention in its double blocks,
the operator-level references of the kernel (float64, an fp32 restatement that rounds where the kernel rounds, and its mutants) with their gate,
and a writer of the XLabs checkpoint layout.

``IPAdapterFluxOracle`` extends the pinned FLUX oracle the way ``tests/_flux_controlnet.ControlledFluxOracle`` does, from the published definition
(XLabs-AI flux-ip-adapter as diffusers' FluxIPAdapterJointAttnProcessor2_0 runs it), written from memory of the published code -- no file and no
diffusers installation exist on the development machines:

  tok  = LayerNorm_C(reshape(Linear(E -> N C)(e), [N, C]))                       once per call, rounded behind the Linear and behind the norm
  K_i  = tok Wk_i^T + bk_i,  V_i = tok Wv_i^T + bv_i                             per double block i, rounded
  ip_i = softmax(q_n K_i^T / sqrt(D)) V_i  per head                              q_n: the image queries behind QK-RMSNorm, BEFORE RoPE
  x_img <- round(x_img + scale * ip_i)     behind double block i, after fc2's gated add; single blocks take nothing

ip_i is rounded once (scores, softmax and the weighted sum are fp32 in the kernel), and the add is one rounding (the LayerNorm launch's fmaf);
the published code rounds scale * ip and the sum separately.  Arithmetic restatement only: no adapter checkpoint has been run."""
import math

import torch

from oracle.mmdit import linear, rope_apply, sdpa
from tests._flux_controlnet import ControlledFluxOracle
from tests._util import BF, randn

IP_SCALE = 0.7


class IPAdapterFluxOracle(ControlledFluxOracle):
    """``ip`` = (adapter weights by the names of weights.synth_ip_adapter_weights (fp32), IPAdapterConfig, image embeds [B or 1, E], scale) or None;
    ``ip_off``: double blocks whose adapter output is zeroed (the sensitivity condition).  ``control`` stays None: taps and the adapter exclude
    each other."""
    ip = None
    ip_off = ()

    def ip_tokens(self):
        w, c, e, _ = self.ip
        P = self.P
        y = linear(P.r(e.float()), w["ip_adapter.proj.weight"], w["ip_adapter.proj.bias"], P).reshape(e.shape[0], c.ip_adapter_tokens, c.ip_adapter_dim)
        return P.r(torch.nn.functional.layer_norm(y, (c.ip_adapter_dim,), w["ip_adapter.norm.weight"], w["ip_adapter.norm.bias"], c.norm_eps))

    def ip_attention(self, i, q_n):
        """q_n [B, H, S_i, D] -> [B, S_i, h], rounded once"""
        w = self.ip[0]
        B, H, S_i, D = q_n.shape
        tok = self.ip_tokens().expand(B, -1, -1)
        k, v = (linear(tok, w[f"ip_adapter.{i}.to_{n}_ip.weight"], w.get(f"ip_adapter.{i}.to_{n}_ip.bias"), self.P).reshape(B, -1, H, D).transpose(1, 2)
                for n in "kv")
        p = torch.softmax(q_n @ k.transpose(-1, -2) * (1.0 / math.sqrt(D)), dim=-1)
        return self.P.r(self._merge(p @ v))

    def _double_block(self, i, img, txt, tkey, rope):
        if self.ip is None or float(self.ip[3]) == 0.0:
            return super()._double_block(i, img, txt, tkey, rope)
        cfg, P = self.cfg, self.P
        pi = f"multimodal_transformer_blocks.{i}.image_transformer_block"
        pt = f"multimodal_transformer_blocks.{i}.text_transformer_block"
        skip_txt = (i == cfg.depth_multimodal - 1) and cfg.depth_unified < 1
        ii = self._pre_sdpa(img, pi, tkey, 6)
        ti = self._pre_sdpa(txt, pt, tkey, 2 if skip_txt else 6)
        S_t = txt.shape[1]
        q, k, v = (torch.cat([ti[n], ii[n]], dim=2) for n in "qkv")
        if rope is not None:
            q, k = rope_apply(q, rope, P), rope_apply(k, rope, P)
        o = self._merge(sdpa(q, k, v, 1.0 / math.sqrt(cfg.head_dim), P))
        img = self._post_sdpa(img, o[:, S_t:], ii, pi, False)
        txt = None if skip_txt else self._post_sdpa(txt, o[:, :S_t], ti, pt, False)
        if i not in self.ip_off:
            s = float(torch.tensor(self.ip[3], dtype=torch.float32))  # (the engine's scalar is fp32)
            img = P.r(img + s * self.ip_attention(i, ii["q"]))
        return img, txt


def synthetic_embeds(n, E, seed=21):
    return randn(n, E, seed=seed)


# ---- the operator ---------------------------------------------------------------------------------------------------------------------------
ROWS = [(1, 0, 5), (2, 3, 5), (2, 8, 70), (3, 5, 6)]  # (B, S_t, S_i)
D = 128


def kernel_case(h, B, S_t, S_i, N):
    """qkv [B, S_t + S_i, 3h] with raw queries of rms 3 (a projection's output is not unit-sized), a QK-norm weight that is not flat, keys of unit
    size (scores of order one: a softmax that is neither uniform nor one-hot) and values; bf16 values in fp32 tensors, CPU"""
    g = torch.Generator().manual_seed(h + 1000 * N + 100 * B + 10 * S_t + S_i)
    r = lambda *s, scale=1.0, mean=0.0: (torch.randn(*s, generator=g) * scale + mean).to(BF).float()
    return r(B, S_t + S_i, 3 * h, scale=3.0), r(D, scale=0.3, mean=1.0), r(B, N, h), r(B, N, h)


def equal_values_case(h, B, S_t, S_i, N):
    """``kernel_case`` with every key of an image carrying the SAME value row, 1 <= |v| <= 2 with random signs: whatever the weights are, the
    definition's output is that row exactly (sum p v / sum p = v), a bf16 value -- the float64 reference and the restatement have no rounding
    error, and what a fault adds stands alone.  The only case on which a second rounding can show: everywhere else it hides under the first
    (tests/test_ip_adapter_cpu.py)."""
    qkv, qn, k, v = kernel_case(h, B, S_t, S_i, N)
    g = torch.Generator().manual_seed(7 + h + N)
    row = ((1.0 + torch.rand(B, 1, h, generator=g)) * (torch.randint(0, 2, (B, 1, h), generator=g) * 2 - 1)).to(BF).float()
    return qkv, qn, k, row.expand(B, N, h).contiguous()


def rope_pairs(q, seed=5):
    """adjacent-pair rotation of every row by its own angles (the mutant 'RoPE applied to q')"""
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(q.shape[:-1] + (q.shape[-1] // 2,), generator=g, dtype=q.dtype) * 3.0
    c, s = torch.cos(ang), torch.sin(ang)
    xe, xo = q[..., 0::2], q[..., 1::2]
    return torch.stack([c * xe - s * xo, s * xe + c * xo], dim=-1).flatten(-2)


def ip_attention_ref(qkv, S_t, qn, k, v, dtype=torch.float64, eps=1e-6, mutant=None):
    """[B * S_i, h].  float64: the definition on the bf16 operands, nothing rounded.  float32: the kernel restated -- q_n rounded to bf16 (the Q
    load's expression), fp32 scores, exact softmax and weighted sum, ONE rounding.  ``mutant``: a fault of the restatement, by name."""
    f64 = dtype == torch.float64
    rnd = (lambda t: t) if f64 else (lambda t: t.to(BF).to(dtype))
    B, S, h3 = qkv.shape
    h, S_i, H = h3 // 3, S - S_t, h3 // 3 // D
    q = qkv[:, S_t:, :h].to(dtype).reshape(B, S_i, H, D)
    if mutant == "q un-normed":
        q_n = rnd(q)
    else:
        q_n = rnd(q * torch.rsqrt((q * q).mean(-1, keepdim=True) + eps) * qn.to(dtype))
    if mutant == "rope on q":
        q_n = rnd(rope_pairs(q_n))
    kk, vv = (t.to(dtype).reshape(B, -1, H, D) for t in (k, v))
    if mutant == "key N-1 dropped":
        kk, vv = kk[:, :-1], vv[:, :-1]
    if mutant == "image 1 reads image 0":
        kk, vv = kk.clone(), vv.clone()
        kk[1], vv[1] = kk[0], vv[0]
    scale = 1.0 if mutant == "no 1/sqrt(D)" else 1.0 / math.sqrt(D)
    s = torch.einsum("bshd,bnhd->bshn", q_n, kk) * scale
    p = torch.exp(s - s.amax(-1, keepdim=True))
    acc, l = torch.einsum("bshn,bnhd->bshd", p, vv), p.sum(-1, keepdim=True)
    if mutant == "output rounded twice":
        acc = rnd(acc)  # (the weighted sum rounded before it is normalised, the quotient rounded again)
    return rnd(acc / l).reshape(B * S_i, h)


MUTANTS = ("rope on q", "q un-normed", "no 1/sqrt(D)", "key N-1 dropped", "image 1 reads image 0", "output rounded twice")


def bf16_unit(x):
    """the spacing of bf16 at |x| (8 significand bits), float64"""
    x = x.double().abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(x)) - 7)


def operator_ratio(got, rest, ref):
    """The operator gate in the project's yardstick form, per (row, head): the error against float64, as the L2 norm over the head's 128 columns,
    is at most 2 x the restatement's plus one bf16 unit at the head's largest reference value.  Returns the worst ratio error / bound (<= 1: pass)."""
    got, rest, ref = (t.detach().double().cpu().reshape(-1, D) for t in (got, rest, ref))
    unit = bf16_unit(ref.abs().amax(-1))
    bound = 2.0 * torch.linalg.norm(rest - ref, dim=-1) + unit
    return float((torch.linalg.norm(got - ref, dim=-1) / bound).max())


# ---- the XLabs checkpoint layout --------------------------------------------------------------------------------------------------------------
def to_xlabs_ip_adapter(w, cfg):
    """adapter weights by this project's names -> the key table of XLabs-AI's ip_adapter.safetensors as ``flux_ip_adapter_checkpoint_to_reference``
    reads it (written from the published definition; not verified against a real file)"""
    out = {"ip_adapter_proj_model.proj.weight": w["ip_adapter.proj.weight"], "ip_adapter_proj_model.proj.bias": w["ip_adapter.proj.bias"],
           "ip_adapter_proj_model.norm.weight": w["ip_adapter.norm.weight"], "ip_adapter_proj_model.norm.bias": w["ip_adapter.norm.bias"]}
    for i in range(cfg.depth_multimodal):
        for n in "kv":
            for leaf in ("weight", "bias"):
                out[f"double_blocks.{i}.processor.ip_adapter_double_stream_{n}_proj.{leaf}"] = w[f"ip_adapter.{i}.to_{n}_ip.{leaf}"]
    return {k: v.contiguous() for k, v in out.items()}
