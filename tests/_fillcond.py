"""Oracle and shared cases of channel-concatenated conditioning (FLUX.1 Fill / Canny / Depth; plain torch / numpy, needs no GPU).

The published FLUX sampling code's ``prepare_fill`` / ``prepare_control``, restated: every model evaluation embeds ``cat(img, img_cond)`` on the
feature axis with an ``img_in`` of 64 + F_c input columns.  ``condition_tokens_reference`` builds ``img_cond`` from the condition latent and
(Fill) the mask as reshapes / permutes; ``FillCondMMDiT`` is ``oracle.mmdit.OracleMMDiT`` with that wider patch embedding -- only the patch
embedding is overridden.  Its fp32 form is the concat-Linear itself; its bf16-emulating form rounds where the engine rounds: the latent's share
(with the bias) and the condition's share each to bf16, then their sum.

The geometries are ``tests/_refcond.py``'s, without the reference image.
"""
import numpy as np
import torch

from diffusionkit_amd.config import tiny_flux
from diffusionkit_amd.weights import synth_mmdit_weights
from oracle.mmdit import OracleMMDiT, Prec
from tests import _refcond as rc
from tests._util import BF, randn

TIMESTEPS, STEP = rc.TIMESTEPS, rc.STEP
# name: (batch, latent (h, w), S_t).  A: no length is a multiple of any tile; B: 256 image rows and a text length that is legal for fp8
CASES = {name: case[:3] for name, case in rc.CASES.items()}
# (case, F_c): Fill's width on every geometry, the control width on the batched one
RUNS = [("A1", 320), ("A2", 320), ("B", 320), ("A2", 64)]


def patchify(x: torch.Tensor, p: int = 2) -> torch.Tensor:
    """[n, Hl, Wl, C] -> [n, S_i, C * p * p], features (c, ph, pw): FLUX's space-to-depth (``patchify_via_reshape``)"""
    n, Hl, Wl, C = x.shape
    return x.reshape(n, Hl // p, p, Wl // p, p, C).permute(0, 1, 3, 5, 2, 4).reshape(n, (Hl // p) * (Wl // p), C * p * p)


def mask_channels(mask: torch.Tensor) -> torch.Tensor:
    """uint8 [n, 8 Hl, 8 Wl] -> f32 [n, Hl, Wl, 64]: mask / 255 (not binarised), 8 x 8 pixel-unshuffled, channel 8 * py + px"""
    n, H, W = mask.shape
    m = mask.to(torch.float32) / 255
    return m.reshape(n, H // 8, 8, W // 8, 8).permute(0, 1, 3, 2, 4).reshape(n, H // 8, W // 8, 64)


def condition_tokens_reference(z: torch.Tensor, mask=None, p: int = 2) -> torch.Tensor:
    """``img_cond``: z f32 [n, Hl, Wl, C] (the encoded, process_in'ed condition image), mask uint8 [1 or n, 8 Hl, 8 Wl] or None ->
    bf16 [n, S_i, p*p*C (+ 64*p*p)]: patchify(z), then (Fill) patchify of the unshuffled mask"""
    tok = patchify(z.to(torch.float32), p)
    if mask is not None:
        m = patchify(mask_channels(mask), p)
        tok = torch.cat([tok, m.expand(tok.shape[0], -1, -1)], dim=-1)
    return tok.to(BF)


def mask_column_formula(mask: np.ndarray, i: int, j: int, py: int, px: int, ph: int, pw: int):
    """the issue's index statement for token (i, j) of a 2 x 2 patchify: (column, value)"""
    return 64 + 4 * (8 * py + px) + 2 * ph + pw, np.float32(mask[16 * i + 8 * ph + py, 16 * j + 8 * pw + px]) / np.float32(255)


def make_mask(n: int, H: int, W: int, seed: int = 9) -> torch.Tensor:
    """uint8 [n, H, W] holding 0, 255 and in-between bytes: a band of each, and noise over the rest"""
    rng = np.random.RandomState(seed)
    m = rng.randint(0, 256, size=(n, H, W)).astype(np.uint8)
    m[:, : H // 4] = 0
    m[:, H // 4: H // 2, : W // 2] = 255
    m[:, -3:, -5:] = 128
    return torch.from_numpy(m)


class FillCondMMDiT(OracleMMDiT):
    """``cond``: the condition tokens [B or 1, S_i, F_c] (fp32 values of bf16 tokens).  The weight "x_embedder.proj.weight" holds F + F_c
    columns."""
    cond = None

    def __call__(self, latent, text, timestep, taps=None, cond=None):
        assert cond is not None, "a model with condition columns is always called with its condition"
        self.cond = cond
        try:
            return super().__call__(latent, text, timestep, taps=taps)
        finally:
            self.cond = None

    def _patch_embed(self, x):
        cfg, P = self.cfg, self.P
        assert cfg.patchify_via_reshape and "x_pos_embedder.pos_embed.weight" not in self.w
        t = patchify(x, cfg.patch_size)
        B, _, F = t.shape
        w = self.w["x_embedder.proj.weight"]
        w = w.reshape(w.shape[0], -1)
        b = self.w["x_embedder.proj.bias"]
        c = P.r(self.cond.to(torch.float32)).expand(B, -1, -1)
        assert w.shape[1] == F + c.shape[-1], (w.shape, F, c.shape)
        if P.act is None:  # the published statement: one Linear over the concatenated features
            return torch.cat([t, c], dim=-1) @ w.t() + b
        # the engine's rounding points: bf16(bf16(t W[:, :F]^T + b) + bf16(c W[:, F:]^T))
        return P.r(P.r(t @ w[:, :F].t() + b) + P.r(c @ w[:, F:].t()))


def weights(fc: int, sharpen: bool = False, seed: int = 1234):
    cfg = tiny_flux(condition_features=fc)
    return rc.sharpened_weights(cfg, seed=seed) if sharpen else synth_mmdit_weights(cfg, seed=seed)


SHARPEN = False  # (the plain synthetic weights already separate the wrong layouts from the bound: test_gpu_fill_cond.test_condition_effect)


def case_inputs(cfg, name, fc):
    """text, pooled, latent, condition latent, mask (None for the control width) of a case, on the CPU; one condition per batch row"""
    B, (Hl, Wl), S_t = CASES[name]
    C = cfg.vae_latent_dim
    mask = make_mask(B, 8 * Hl, 8 * Wl) if fc == 320 else None
    return (randn(B, S_t, cfg.token_level_text_embed_dim, seed=3), randn(B, cfg.pooled_text_embed_dim, seed=4), randn(B, Hl, Wl, C, seed=5),
            randn(B, Hl, Wl, C, seed=6), mask)


_ORACLE = {}


def oracle_case(name, fc, steps=(STEP,), tokens_fn=condition_tokens_reference):
    """{"fp32" | "emu": {step: {"final", "final0"}}}: the oracle's final-layer output with the condition and with an all-zero condition;
    computed once per key and shared -- treat as read-only.  ``tokens_fn``: the layout under test (the wrong layouts of the effect test)"""
    key = (name, fc, tuple(steps), tokens_fn)
    if key not in _ORACLE:
        cfg = tiny_flux(condition_features=fc)
        wf = {k: v.float() for k, v in weights(fc, SHARPEN).items()}
        text, pooled, lat, z, mask = case_inputs(cfg, name, fc)
        cond = tokens_fn(z, mask).float()
        res = {}
        for pname, P in (("fp32", Prec()), ("emu", Prec(BF))):
            m = FillCondMMDiT(cfg, wf, P)
            m.cache_modulation_params(pooled, torch.tensor(TIMESTEPS))
            res[pname] = {}
            for s in steps:
                taps, taps0 = {}, {}
                m(lat, text, TIMESTEPS[s], taps=taps, cond=cond)
                m(lat, text, TIMESTEPS[s], taps=taps0, cond=torch.zeros_like(cond))
                res[pname][s] = {"final": taps["final"], "final0": taps0["final"]}
        _ORACLE[key] = res
    return _ORACLE[key]


# ---- the two wrong layouts the effect test must tell from the right one -----------------------------------------------------------------
def tokens_mask_phpwc(z, mask=None, p: int = 2):
    """mask columns in (ph, pw, c) order instead of (c, ph, pw)"""
    tok = patchify(z.to(torch.float32), p)
    mc = mask_channels(mask)
    n, Hl, Wl, _ = mc.shape
    m = mc.reshape(n, Hl // p, p, Wl // p, p, 64).permute(0, 1, 3, 2, 4, 5).reshape(n, (Hl // p) * (Wl // p), 64 * p * p)
    return torch.cat([tok, m.expand(tok.shape[0], -1, -1)], dim=-1).to(BF)


def tokens_halves_swapped(z, mask=None, p: int = 2):
    """the mask's columns in front of the latent's"""
    t = condition_tokens_reference(z, mask, p)
    F = p * p * z.shape[-1]
    return torch.cat([t[..., F:], t[..., :F]], dim=-1).contiguous()
