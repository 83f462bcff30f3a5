"""Skip-layer guidance for the parity tests: the CPU oracle of a model that skips blocks, the step loop restated with the term, and the weights that
make a skipped block visible to the project's gates.

``SkipOracle`` is ``tests/_mmditx.MMDiTXOracle`` whose blocks in ``skip`` pass both streams through unchanged: what the engine's forked row group
computes (``MMDiTEngine.set_skip_layers``).  ``slg_loop`` is tests/test_guidance_cpu.py's ``guided_loop`` with ``sampler.slg_reference``'s term in the
evaluations ``sampler.slg_rows`` names, on two oracle instances that share weights.

``boost``: with the synthetic weights as drawn, skipping blocks of ``tiny_sd35m(depth=4, heads=4, dual=2)`` moves the fp32 oracle's output by a rel-L2
of about 0.02, and the bf16 emulation sits 0.006 - 0.007 from fp32: the project's gate (2 e_emu + 2e-3, about 0.014) could not tell a skipped block
from one that ran.  Scaling the gate chunks of the named blocks' adaLN Linears by g = 8 (a power of two: exact in every element type) makes those
blocks matter -- the ratios are asserted on the oracles alone in tests/test_slg_cpu.py before anything is compared with the GPU.

Arithmetic only, on synthetic weights: no SD3.5-medium checkpoint has been run."""
import functools

import torch

from diffusionkit_amd.config import tiny_sd35m
from diffusionkit_amd.sampler import guidance_rows, guide_reference, slg_reference, slg_rows, step_plan
from diffusionkit_amd.weights import synth_mmdit_weights
from oracle.mmdit import Prec, embed_dtype
from tests._mmditx import MMDiTXOracle
from tests._util import BF, randn
from tests.test_samplers_cpu import blend

F16 = torch.float16
TS = [1000.0, 752.0, 500.0]  # tests/test_gpu_mmditx.py's timesteps; the forward cases run step 1
G = 8.0  # the boost of every case
DEPTH = 4
SKIP_SETS = [(1, 2), (0,), (3,), (2, 3)]  # a dual and a plain block with block 0 on the live rows alone; a fork right behind the embedders; the last
#                                           block, whose text stream stops early; the last two blocks
# name -> (config, n_img, Hl, Wl, S_t): the forward cases; heads 6: h = 384 and 35 image tokens, an odd count on every tile
FORWARD = {"b3": (tiny_sd35m(depth=DEPTH, heads=4, dual=2), 1, 8, 12, 20), "heads6_35tok": (tiny_sd35m(depth=DEPTH, heads=6, dual=2), 2, 10, 14, 20)}


class SkipOracle(MMDiTXOracle):
    """``skip``: the double blocks that return their inputs (None for the text stream of the last block, as the block itself returns)"""

    def __init__(self, cfg, w, P, skip=(), **kw):
        super().__init__(cfg, w, P, **kw)
        self.skip = frozenset(int(b) for b in skip)

    def _double_block(self, i, img, txt, tkey, rope):
        if i in self.skip:
            return img, (None if i == self.cfg.depth_multimodal - 1 else txt)
        return super()._double_block(i, img, txt, tkey, rope)


def boost(weights, cfg, blocks, g):
    """a copy of reference-named MMDiT ``weights`` with the gate chunks (rows 2, 5, 8 of ``adaLN_modulation.layers.1``, weight and bias) of ``blocks``,
    both streams, scaled by ``g``; a stream with fewer chunks (the text stream of the last block has two) keeps the ones it lacks out"""
    out = dict(weights)
    h = cfg.hidden_size
    for i in blocks:
        for stream in ("image", "text"):
            for leaf in ("weight", "bias"):
                name = f"multimodal_transformer_blocks.{i}.{stream}_transformer_block.adaLN_modulation.layers.1.{leaf}"
                t = out[name].clone()
                for chunk in (2, 5, 8):
                    if (chunk + 1) * h <= t.shape[0]:
                        t[chunk * h:(chunk + 1) * h] *= g
                out[name] = t
    return out


def boosted_weights(cfg, skip, g=G, seed=1234):
    """the synthetic weights of ``cfg`` with the blocks of ``skip`` boosted, as drawn (bf16): what ``pack_mmdit`` takes"""
    return boost(synth_mmdit_weights(cfg, seed=seed), cfg, skip, g)


def forward_inputs(cfg, n_img, Hl, Wl, S_t):
    """(text, pooled, latent) of the two live groups, [2 n_img, ...]: tests/test_gpu_mmditx.py's seeds"""
    B = 2 * n_img
    return randn(B, S_t, cfg.token_level_text_embed_dim, seed=3), randn(B, cfg.pooled_text_embed_dim, seed=4), randn(B, Hl, Wl, 16, seed=5)


def _final(model, pooled, lat, text):
    model.cache_modulation_params(pooled, torch.tensor(TS))
    taps = {}
    model(lat, text, TS[1], taps=taps)
    return taps["final"]


@functools.lru_cache(maxsize=None)
def forward_refs(case, skip, f16=False):
    """{"full": {...}, "skip": {...}}: the final-layer tokens of the full model on the 2 n live rows and of the skip model on the n prompt rows, per
    oracle precision -- fp32 and emu (bf16), or with ``f16`` fp32, emu16 and emubf on fp16-rounded weights.  Computed once per case."""
    cfg, n, Hl, Wl, S_t = FORWARD[case]
    named = boosted_weights(cfg, skip)
    wf = {k: (v.to(F16) if f16 else v).float() for k, v in named.items()}
    text, pooled, lat = forward_inputs(cfg, n, Hl, Wl, S_t)
    precs = {"fp32": (Prec(), dict(embed_prec=Prec(embed_dtype(cfg)))), "emu16": (Prec(F16), {}), "emubf": (Prec(BF), {})} if f16 else \
            {"fp32": (Prec(), {}), "emu": (Prec(BF), {})}
    res = {"full": {}, "skip": {}}
    for name, (P, kw) in precs.items():
        res["full"][name] = _final(SkipOracle(cfg, wf, P, (), **kw), pooled, lat, text)
        res["skip"][name] = _final(SkipOracle(cfg, wf, P, skip, **kw), pooled[:n], lat[:n], text[:n])
    return res


def slg_loop(model, skip_model, name, x, sigmas, conditioning, pooled, cfg_weight, act, t_act=None, mode="cfg", interval=None, inpaint=None, rescale=0.7,
             eta=0.0, norm_threshold=0.0, momentum=0.0, slg_scale=0.0, slg_interval=(0.0, 1.0)):
    """tests/test_guidance_cpu.py's ``guided_loop`` with skip-layer guidance: an evaluation ``slg_rows`` names forms a third prediction k, the prompt
    row through ``skip_model`` (same weights, its modulation cached for the prompt row), and takes den + slg_scale (c - k): "cfg" in cfg_denoise's own
    fp32 expression, the other modes through ``slg_reference`` (float64, rounded to float32 once).  With ``slg_scale`` 0 it is ``guided_loop``."""
    timesteps = (t_act or act).r(sigmas * 1000.0)
    plan = step_plan(name, sigmas.numpy())
    rows = guidance_rows(plan, interval)
    srows = slg_rows(plan, rows, *slg_interval)
    skip_model.cache_modulation_params(pooled[0:1], timesteps)
    hist = m = None
    on = None
    for r, g, sl in zip(plan, rows, srows):
        if g.guided != on:
            on = g.guided
            model.cache_modulation_params(pooled if on else pooled[0:1], timesteps)
        t = float(timesteps[r.index])
        if not on:
            x_in = act.r(x)
            den = x_in - model(x_in, conditioning[0:1], t) * r.sigma
        else:
            x_in = act.r(torch.cat([x] * 2, dim=0))
            both = x_in - model(x_in, conditioning, t) * r.sigma
            c, u = both[0:1], both[1:2]
            k = x_in[0:1] - skip_model(x_in[0:1], conditioning[0:1], t) * r.sigma if sl else None
            if mode == "cfg":
                den = u + cfg_weight * (c - u)
                if sl:
                    den = den + slg_scale * (c - k)
            else:
                reads, writes = momentum != 0.0 and not g.first, momentum != 0.0 and g.feeds
                kw = dict(rescale=rescale, eta=eta, norm_threshold=norm_threshold, momentum=momentum, m=m, reads_m=reads, writes_m=writes)
                if sl:
                    den64, m = slg_reference(c.numpy(), u.numpy(), k.numpy(), cfg_weight, slg_scale, mode, **kw)
                else:
                    den64, m = guide_reference(c.numpy(), u.numpy(), cfg_weight, mode, **kw)
                den = torch.from_numpy(den64).to(torch.float32)
        d = (x - den) / r.sigma
        x_new = r.cx * x + r.cd * d + r.ch * hist if r.reads_h else r.cx * x + r.cd * d
        hist = r.hx * x + r.hd * d if r.writes_h else hist
        x = x_new
        if inpaint is not None:
            noise, x_orig, mm = inpaint
            x = blend(x, r.sigma_next, noise, x_orig, mm.to(torch.float32)[None, :, :, None])
    return x


# ---- the pipeline cases: SD3.5-medium tiny, boosted; 4 steps, CFG 5, shift 3, scale 2.5, interval (0, 0.6): the term on steps 1 and 2 -------------------
PIPE_CFG = tiny_sd35m(depth=DEPTH, heads=4, dual=2)
PIPE_SKIP = (1, 2)
STEPS, CFGW, SHIFT, SCALE, WINDOW = 4, 5.0, 3.0, 2.5, (0.0, 0.6)
HL, WL = 8, 12
SLG_KW = dict(skip_layer_guidance=SCALE, skip_layers=PIPE_SKIP, skip_layer_interval=WINDOW)


def pipe_inputs():
    """(text, pooled): [prompt, negative], tests/test_inpaint_cpu.py's seeds"""
    return randn(2, 16, PIPE_CFG.token_level_text_embed_dim, seed=7), randn(2, PIPE_CFG.pooled_text_embed_dim, seed=8)


def pipe_oracles(P, f16=False, **kw):
    """(full model, skip model) on the boosted pipeline weights, sharing them"""
    wf = {k: (v.to(F16) if f16 else v).float() for k, v in boosted_weights(PIPE_CFG, PIPE_SKIP).items()}
    return SkipOracle(PIPE_CFG, wf, P, (), **kw), SkipOracle(PIPE_CFG, wf, P, PIPE_SKIP, **kw)
