"""Oracle and shared cases of reference-image conditioning (FLUX.1 Kontext's token layout; plain torch, needs no GPU).

``RefCondMMDiT`` is ``oracle.mmdit.OracleMMDiT`` with one more argument to its forward: the reference latent, whose patch embedding is
concatenated behind the image rows (published Kontext sampling code: ``img = cat(img, img_cond)``, ``pred[:, :S_i]``).  Only the forward is
overridden; the blocks, the final layer and the unpatchify are the base class's.  ``rope_table_ext`` builds the table of the joint
[text | image | reference] sequence from the formulas of ``oracle.mmdit.rope_table``: the reference rows sit at (1, row, col) of their own grid.

With the project's synthetic weights (N(0, 0.02^2)) the reference barely moves the output -- an engine that ignores it would pass a model-level
parity test -- so the cases here use sharpened weights (``sharpened_weights``) and the tests compare the reference's EFFECT
delta = out(ref) - out(no ref), which is 0.14 of the output norm with them.
"""
import torch

from diffusionkit_amd.config import tiny_flux
from diffusionkit_amd.weights import synth_mmdit_weights
from oracle.mmdit import OracleMMDiT, Prec, affine_transform
from tests._util import BF, randn

TIMESTEPS = [1000.0, 752.0, 500.0]
STEP = 1
# name: (batch, latent (h, w), S_t, reference latent (h, w)).  A: no length is a multiple of any tile, the reference grid differs from the image
# grid and is not square.  B: the image stream has 496 rows, the reference starts inside a GEMM row tile and inside an attention key block, and
# the text length is fp8-legal
CASES = {"A1": (1, (8, 12), 20, (6, 10)), "A2": (2, (8, 12), 20, (6, 10)), "B": (1, (32, 32), 128, (24, 40))}


def rope_table_ext(cfg, text_len: int, h: int, w: int, rh: int = 0, rw: int = 0, index: float = 1.0, transposed: bool = False) -> torch.Tensor:
    """cos/sin table [S_t + h*w + rh*rw, D/2, 2]: text (0, 0, 0), image (0, row, col), reference (index, row, col) with the reference's own rows and
    columns counted from 0.  ``transposed`` / ``index`` build the wrong tables the tests must tell from the right one."""
    S_i, S_r = h * w, rh * rw
    pos = torch.zeros(text_len + S_i + S_r, 3, dtype=torch.float32)
    pos[text_len:text_len + S_i, 1] = torch.arange(h, dtype=torch.float32)[:, None].expand(h, w).reshape(-1)
    pos[text_len:text_len + S_i, 2] = torch.arange(w, dtype=torch.float32)[None, :].expand(h, w).reshape(-1)
    if S_r:
        rows = torch.arange(rh, dtype=torch.float32)[:, None].expand(rh, rw)
        cols = torch.arange(rw, dtype=torch.float32)[None, :].expand(rh, rw)
        if transposed:  # (the grid walked column by column)
            rows, cols = rows.t(), cols.t()
        pos[text_len + S_i:, 0] = float(index)
        pos[text_len + S_i:, 1] = rows.reshape(-1)
        pos[text_len + S_i:, 2] = cols.reshape(-1)
    outs = []
    for i, dim in enumerate(cfg.rope_axes_dim):
        scale = torch.arange(0, dim, 2, dtype=torch.float32) / dim
        omega = 1.0 / (float(cfg.rope_theta) ** scale)
        ang = pos[:, i:i + 1] * omega[None, :]
        outs.append(torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1))
    return torch.cat(outs, dim=1)


class RefCondMMDiT(OracleMMDiT):
    """``ref``: the reference latent [B or 1, rh, rw, C] or None.  taps["stream"]: the joint stream [B, S_t + S_i + S_r, h] behind the last block."""
    ref_index = 1.0
    ref_transposed = False

    def __call__(self, latent, text, timestep, taps=None, ref=None):
        if ref is None:
            return super().__call__(latent, text, timestep, taps=taps)
        cfg, P = self.cfg, self.P
        assert cfg.rope_axes_dim is not None and cfg.depth_unified > 0, "reference rows need RoPE (FLUX geometry)"
        tkey = float(timestep)
        B, Hl, Wl, _ = latent.shape
        p = cfg.patch_size
        txt = self._lin(P.r(text), "context_embedder")
        img = self._patch_embed(P.r(latent))
        S_t, S_i = txt.shape[1], img.shape[1]
        r = self._patch_embed(P.r(ref))
        img = torch.cat([img, r.expand(B, -1, -1)], dim=1)
        rope = rope_table_ext(cfg, S_t, Hl // p, Wl // p, ref.shape[1] // p, ref.shape[2] // p, self.ref_index, self.ref_transposed)
        for i in range(cfg.depth_multimodal):
            img, txt = self._double_block(i, img, txt, tkey, rope)
        x = torch.cat([txt, img], dim=1)
        for i in range(cfg.depth_unified):
            x = self._single_block(i, x, tkey, rope)
        if taps is not None:
            taps["stream"] = x.clone()
        mod = self._mod["final_layer"][tkey].chunk(2, dim=-1)
        y = affine_transform(x[:, S_t:S_t + S_i], mod[0], mod[1], cfg.layer_norm_eps, P)
        y = self._lin(y, "final_layer.linear")
        if taps is not None:
            taps["final"] = y.clone()
        return self._unpatch(y, Hl, Wl)


def sharpened_weights(cfg=None, seed=1234, factor=3.0):
    """``synth_mmdit_weights`` with the QK-norm weights and every v / o projection times ``factor``: attention that attends, and values that
    carry -- the reference rows then move the output by 0.14 of its norm instead of 1e-3"""
    named = synth_mmdit_weights(cfg or tiny_flux(), seed=seed)
    hit = 0
    for k in named:
        if k.endswith("q_norm.weight") or k.endswith("k_norm.weight") or (k.endswith(".weight") and (".v_proj" in k or ".o_proj" in k)):
            named[k] = (named[k].float() * factor).to(named[k].dtype)
            hit += 1
    assert hit > 0
    return named


def case_inputs(cfg, name):
    """text, pooled, latent, reference latent (one per batch row) of a case, bf16-representable fp32 on the CPU"""
    B, (Hl, Wl), S_t, (rh, rw) = CASES[name]
    C = cfg.vae_latent_dim
    return (randn(B, S_t, cfg.token_level_text_embed_dim, seed=3), randn(B, cfg.pooled_text_embed_dim, seed=4), randn(B, Hl, Wl, C, seed=5),
            randn(B, rh, rw, C, seed=6))


_ORACLE = {}


def oracle_case(name, steps=(STEP,)):
    """{"fp32" | "emu": {step: {"final", "stream", "final0"}}}: the oracle's taps with the reference, and its final-layer output without one
    ("final0"); computed once per case and shared -- treat as read-only"""
    key = (name, tuple(steps))
    if key not in _ORACLE:
        cfg = tiny_flux()
        wf = {k: v.float() for k, v in sharpened_weights(cfg).items()}
        text, pooled, lat, ref = case_inputs(cfg, name)
        res = {}
        for pname, P in (("fp32", Prec()), ("emu", Prec(BF))):
            m = RefCondMMDiT(cfg, wf, P)
            m.cache_modulation_params(pooled, torch.tensor(TIMESTEPS))
            res[pname] = {}
            for s in steps:
                taps, taps0 = {}, {}
                m(lat, text, TIMESTEPS[s], taps=taps, ref=ref)
                m(lat, text, TIMESTEPS[s], taps=taps0)
                res[pname][s] = {"final": taps["final"], "stream": taps["stream"], "final0": taps0["final"]}
        _ORACLE[key] = res
    return _ORACLE[key]
