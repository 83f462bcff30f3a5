"""First-block cache on an MI355X: the two kernels against torch bit for bit, the engine's head / tail entries against dk_mmdit_forward bit
for bit, the reuse tail against its definition and the oracle's FinalLayer, the closed loop through ``denoise_latents`` against a restatement
built from OracleMMDiT's own pieces, and the state rules (errors that name the rule, an exact-size poisoned workspace, the off-engine's bytes).

Semantics (include/dk_hip.h): on the image rows of the joint stream, in the engine's element type E with one rounding per stored value,
D_cur = round_E(X1 - X0), num = sum |D_cur - D_ref|, den = sum |D_ref| per batch row; compute tail: R = round_E(X_L - X1), D_ref <- D_cur;
reuse tail: X <- round_E(X1 + R).  Every figure is printed before it is asserted.

The file name sorts in front of tests/test_gpu_fullsize.py's heavy cases on purpose: nothing here is larger than a tiny model."""
import ctypes
import functools
import math
from dataclasses import replace

import pytest
import torch

from diffusionkit_amd.config import float16_config, tiny_flux, tiny_sd3, tiny_vae, tiny_vae_encoder
from diffusionkit_amd.sampler import FixedSchedule
from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
from oracle import pipeline as op
from oracle.mmdit import OracleMMDiT, Prec, affine_transform, embed_dtype, rope_table
from tests import _engine_state as es
from tests import _footprint as fp
from tests._util import BF, psnr, randn, rel_l2
from tests.test_inpaint_cpu import half_mask, latent_mask, make_image, masked_sample_euler

pytestmark = pytest.mark.gpu

F16 = torch.float16
NAN = float("nan")
bits = fp.bits


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def yardstick_ok(hip, emu, exact, what=""):
    """the project's model-level rule (tests/test_gpu_model.py): hip-vs-fp32 <= 2 * emu-vs-fp32 + 2e-3 (relative L2)"""
    e_h, e_e = rel_l2(exact, hip), rel_l2(exact, emu)
    print(f"[block cache] {what}: rel_l2 hip-vs-fp32 {e_h:.3e}, emu-vs-fp32 {e_e:.3e}")
    assert e_h <= 2.0 * e_e + 2e-3, f"{what}: hip-vs-fp32 {e_h:.3e} > 2*emu-vs-fp32 {e_e:.3e} + 2e-3"
    return e_h, e_e


def psnr_ok(hip, emu, exact, what=""):
    """tests/test_gpu_model.py: >= 35 dB against the fp32 oracle, or within 1.5 dB of what the bf16-emulating oracle reaches"""
    p_h, p_e = psnr(exact, hip), psnr(exact, emu)
    print(f"[block cache] {what}: PSNR hip {p_h:.1f} dB, bf16-emulating oracle {p_e:.1f} dB")
    assert p_h > min(35.0, p_e - 1.5), f"{what}: PSNR hip {p_h:.1f} dB, bf16-emulating oracle {p_e:.1f} dB"


# ---- 1. the operators against torch ---------------------------------------------------------------------------------------------------
OP_SHAPES = [(2, 20, 24, 256, BF), (1, 3, 5, 3072, BF), (2, 7, 9, 2432, BF), (2, 20, 24, 1536, F16)]
OP_IDS = [f"B{b}-St{st}-Si{si}-h{h}-{'bf16' if dt == BF else 'f16'}" for b, st, si, h, dt in OP_SHAPES]


def rnd(*shape, seed, dt, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dt)


def joint_with_poisoned_text(img, S_t, dev):
    """[B, S_t + S_i, h] on the device inside NaN margins: text rows NaN, image rows = img"""
    B, S_i, h = img.shape
    x = torch.full((B, S_t + S_i, h), NAN, dtype=img.dtype)
    x[:, S_t:] = img
    return fp.guarded(x.to(dev), 4)


@pytest.mark.parametrize("B,S_t,S_i,h,dt", OP_SHAPES, ids=OP_IDS)
def test_probe_operator(dev, B, S_t, S_i, h, dt):
    """D_cur bit-identical to (x1.float() - x0.float()).to(E); num / den against float64 sums of the same rounded values to a relative 1e-4
    (at most 8 * 8 = 64 sequential additions per lane at h = 4096, 6 butterfly steps, ceil(S_i / 64) per lane and 6 more steps across the rows: about
    80 fp32 additions of non-negative terms, 80 * 2^-24 = 5e-6, 20 x headroom; one dropped row of these shapes moves a sum by >= 1e-2); two runs
    return the same bits; the text rows and everything around the operands are NaN and stay out of every result; d_ref = None: den = 0."""
    from diffusionkit_amd import ops
    x1_img, x0, dref = rnd(B, S_i, h, seed=1, dt=dt), rnd(B, S_i, h, seed=2, dt=dt), rnd(B, S_i, h, seed=3, dt=dt, scale=0.5)
    want_d = (x1_img.float() - x0.float()).to(dt)
    want_num = (want_d.double() - dref.double()).abs().sum(dim=(1, 2))
    want_den = dref.double().abs().sum(dim=(1, 2))
    runs = []
    for _ in range(2):
        x, gx = joint_with_poisoned_text(x1_img, S_t, dev)
        d, gd = fp.guarded(x0.to(dev), 4)
        r, gr = fp.guarded(dref.to(dev), 4)
        d_out, probe = ops.block_probe(x, S_t, d, r)
        torch.cuda.synchronize()
        assert d_out.data_ptr() == d.data_ptr()
        for g, what in ((gx, "x"), (gd, "d"), (gr, "d_ref")):
            g.check(f"probe: margins of {what}")
        assert same_bits(x.cpu()[:, S_t:], x1_img) and bool(torch.isnan(x.cpu()[:, :S_t].float()).all()), "the probe wrote the stream"
        assert same_bits(r.cpu(), dref), "the probe wrote d_ref"
        runs.append((d.cpu().clone(), probe.cpu().clone()))
    d_got, probe = runs[0]
    assert same_bits(d_got, want_d), f"D_cur differs from the torch expression in {int((bits(d_got) != bits(want_d)).sum())} elements"
    num, den = probe[:, 0].double(), probe[:, 1].double()
    e_n, e_d = float(((num - want_num).abs() / want_num).max()), float(((den - want_den).abs() / want_den).max())
    print(f"[block cache] probe {B}x({S_t}+{S_i})x{h} {dt}: num {num.tolist()}, den {den.tolist()}, relative error num {e_n:.2e} den {e_d:.2e}")
    assert probe.dtype == torch.float32 and bool(torch.isfinite(probe).all())
    assert e_n <= 1e-4 and e_d <= 1e-4
    assert same_bits(runs[1][0], d_got) and same_bits(runs[1][1], probe), "two runs of the probe differ"
    # without a reference: den = 0, num = sum |D_cur|
    x, _ = joint_with_poisoned_text(x1_img, S_t, dev)
    d, _ = fp.guarded(x0.to(dev), 4)
    _, probe0 = ops.block_probe(x, S_t, d, None)
    probe0 = probe0.cpu()
    assert same_bits(d.cpu(), want_d)
    assert bool((probe0[:, 1] == 0).all())
    want0 = want_d.double().abs().sum(dim=(1, 2))
    assert float(((probe0[:, 0].double() - want0).abs() / want0).max()) <= 1e-4


@pytest.mark.parametrize("B,S_t,S_i,h,dt", OP_SHAPES, ids=OP_IDS)
def test_residual_operator(dev, B, S_t, S_i, h, dt):
    """both forms bit-identical to the torch expression; the capture leaves the stream alone, the reuse leaves r and the text rows alone"""
    from diffusionkit_amd import ops
    x_img, p1 = rnd(B, S_i, h, seed=4, dt=dt), rnd(B, S_i, h, seed=5, dt=dt)
    x, gx = joint_with_poisoned_text(x_img, S_t, dev)
    r, gr = fp.guarded(p1.to(dev), 4)
    out = ops.block_residual(x, S_t, r, False)
    torch.cuda.synchronize()
    want_r = (x_img.float() - p1.float()).to(dt)
    assert out.data_ptr() == r.data_ptr() and same_bits(r.cpu(), want_r), "R = round(x - p1)"
    assert same_bits(x.cpu()[:, S_t:], x_img) and bool(torch.isnan(x.cpu()[:, :S_t].float()).all())
    # x - x = +0, every bit clear (a model whose block 0 is its only block)
    z, _ = fp.guarded(x_img.to(dev), 4)
    ops.block_residual(x, S_t, z, False)
    assert int(bits(z.cpu()).ne(0).sum()) == 0
    x2_img = rnd(B, S_i, h, seed=6, dt=dt)
    x2, gx2 = joint_with_poisoned_text(x2_img, S_t, dev)
    out = ops.block_residual(x2, S_t, r, True)
    torch.cuda.synchronize()
    assert out.data_ptr() == x2.data_ptr()
    assert same_bits(x2.cpu()[:, S_t:], (x2_img.float() + want_r.float()).to(dt)), "x = round(x + r)"
    assert bool(torch.isnan(x2.cpu()[:, :S_t].float()).all()) and same_bits(r.cpu(), want_r)
    for g, what in ((gx, "x"), (gr, "r"), (gx2, "x (reuse)")):
        g.check(f"residual: margins of {what}")


def test_operators_name_the_alignment_rule(dev):
    from diffusionkit_amd import ops
    from diffusionkit_amd._lib import DkHipError
    x = torch.zeros(1, 4, 20, dtype=BF, device=dev)
    with pytest.raises(DkHipError, match="multiple of 8"):
        ops.block_probe(x, 1, torch.zeros(1, 3, 20, dtype=BF, device=dev))
    with pytest.raises(DkHipError, match="multiple of 8"):
        ops.block_residual(x, 1, torch.zeros(1, 3, 20, dtype=BF, device=dev), True)


# ---- engines --------------------------------------------------------------------------------------------------------------------------
TS = [1000.0, 752.0, 500.0]
SD35 = replace(tiny_sd3(depth=3, heads=6), use_qk_norm=True)  # the SD3.5 shape class of tests/test_gpu_model.py::test_mmdit_forward_tiny
FP8 = replace(tiny_flux(depth_multimodal=2, depth_unified=2, heads=2), weight_dtype="fp8_e4m3")  # tests/test_gpu_fp8.py::test_mmdit_fp8_tiny


def engine_for(cfg, dev):
    from diffusionkit_amd.engine import MMDiTEngine
    named = synth_mmdit_weights(cfg, seed=1234)
    return MMDiTEngine(cfg, pack_mmdit(cfg, named, dev)), named


def inputs_for(eng, dev, B, Hl, Wl, S_t, seed0=0):
    cfg = eng.config
    text = randn(B, S_t, cfg.token_level_text_embed_dim, seed=seed0 + 3)
    pooled = randn(B, cfg.pooled_text_embed_dim, seed=seed0 + 4)
    lat = randn(B, Hl, Wl, 16, seed=seed0 + 5)
    return dict(text=text, pooled=pooled, lat=lat, text_dev=text.to(dev, eng.dtype), pooled_dev=pooled.to(dev), lat_dev=lat.to(dev))


def start(eng, shape, inp, on):
    B, Hl, Wl, S_t = shape
    eng.enable_block_cache(on)
    eng.prepare(B, (Hl, Wl), S_t, len(TS))
    eng.cache_modulation_params(inp["pooled_dev"], TS)
    return eng.patchify(inp["lat_dev"])


def peek(eng, which, shape):
    """a copy of one of the engine's internal buffers (dk_mmdit_debug_buffer) on the host"""
    torch.cuda.synchronize()
    ptr = eng.lib.dk_mmdit_debug_buffer(eng._h, which)
    assert ptr, f"debug buffer {which} is NULL"
    t = torch.empty(shape, dtype=eng.dtype, device=eng._ws.device)
    hip = ctypes.CDLL("libamdhip64.so")  # (kind 3: device to device)
    assert hip.hipMemcpy(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t(t.numel() * t.element_size()), 3) == 0
    return t.cpu()


def geometry(eng, shape):
    B, Hl, Wl, S_t = shape
    p = eng.config.patch_size
    S_i = (Hl // p) * (Wl // p)
    return B, S_t, S_i, eng.config.hidden_size


ALL_COMPUTED = [("flux_b1", tiny_flux(), (1, 8, 12, 20)), ("flux_b2", tiny_flux(), (2, 8, 12, 20)), ("sd3_b2", tiny_sd3(), (2, 8, 12, 20)),
                ("sd35", SD35, (2, 8, 12, 20)), ("sd3_depth1", tiny_sd3(depth=1), (2, 8, 12, 20)),
                ("sd3_f16", float16_config(tiny_sd3()), (2, 8, 12, 20)), ("flux_fp8", FP8, (1, 8, 8, 128))]


# ---- 2. cache on, every step computed = cache off -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cfg,shape", ALL_COMPUTED, ids=[c[0] for c in ALL_COMPUTED])
def test_every_step_computed_equals_cache_off(dev, name, cfg, shape):
    """forward_head + forward_tail(reuse=False) gives forward_tokens' tokens bit for bit at every cached step; dk_mmdit_forward on the
    cache-enabled engine does too; the probe reports den = 0 before the first computed step and finite sums behind it"""
    eng, _ = engine_for(cfg, dev)
    inp = inputs_for(eng, dev, *shape)
    tok = start(eng, shape, inp, False)
    assert eng.lib.dk_mmdit_debug_buffer(eng._h, 3) is None
    off = [eng.forward_tokens(tok, inp["text_dev"], i).cpu() for i in range(len(TS))]
    tok = start(eng, shape, inp, True)
    B, S_t, S_i, h = geometry(eng, shape)
    for i in range(len(TS)):
        probe = eng.forward_head(tok, inp["text_dev"], i).cpu()
        out = eng.forward_tail(i, False).cpu()
        print(f"[block cache] {name} step {i}: probe (num, den) {probe.tolist()}")
        assert probe.shape == (B, 2) and bool(torch.isfinite(probe).all()) and bool((probe[:, 0] > 0).all())
        assert bool((probe[:, 1] == 0).all()) if i == 0 else bool((probe[:, 1] > 0).all())
        assert same_bits(out, off[i]), f"{name}: step {i} through head + compute tail differs from forward_tokens"
        assert bool(torch.isfinite(out.float()).all())
    again = eng.forward_tokens(tok, inp["text_dev"], 1).cpu()
    assert same_bits(again, off[1]), "dk_mmdit_forward on a cache-enabled engine"
    if cfg.depth_multimodal + cfg.depth_unified == 1:  # block 0 is the only block: the tail's range is empty, R is all +0
        assert int(bits(peek(eng, 3, (B * S_i, h))).ne(0).sum()) == 0
        eng.forward_head(tok, inp["text_dev"], 2)
        x1 = peek(eng, 0, (B, S_t + S_i, h))
        out = eng.forward_tail(2, True).cpu()
        assert same_bits(peek(eng, 0, (B, S_t + S_i, h)), x1), "reuse with R = +0 must reproduce X1"
        assert same_bits(out, off[2])


# ---- 3. reuse does what it says ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cfg", [("flux", tiny_flux()), ("sd3_f16", float16_config(tiny_sd3()))])
def test_reuse_tail(dev, name, cfg):
    shape = (2, 8, 12, 20)
    eng, named = engine_for(cfg, dev)
    E = eng.dtype
    inp_a, inp_b = inputs_for(eng, dev, *shape), inputs_for(eng, dev, *shape, seed0=50)
    tok_a = start(eng, shape, inp_a, True)
    tok_b = eng.patchify(inp_b["lat_dev"])
    B, S_t, S_i, h = geometry(eng, shape)
    a, b = 0, 1
    eng.forward_head(tok_a, inp_a["text_dev"], a)
    eng.forward_tail(a, False)
    R, D_ref = peek(eng, 3, (B, S_i, h)), peek(eng, 4, (B, S_i, h))
    assert int(bits(R).ne(0).sum()) > 0 and bool(torch.isfinite(R.float()).all())
    probe = eng.forward_head(tok_b, inp_a["text_dev"], b).cpu()
    X1 = peek(eng, 0, (B, S_t + S_i, h))
    D_cur = peek(eng, 5, (B, S_i, h))
    out = eng.forward_tail(b, True).cpu()
    X = peek(eng, 0, (B, S_t + S_i, h))
    assert same_bits(X[:, S_t:], (X1[:, S_t:].float() + R.float()).to(E)), "image rows != round_E(X1 + R)"
    assert same_bits(X[:, :S_t], X1[:, :S_t]), "the reuse tail touched the text rows"
    assert same_bits(peek(eng, 3, (B, S_i, h)), R) and same_bits(peek(eng, 4, (B, S_i, h)), D_ref), "the reuse tail changed R / D_ref"
    # the probe of step b against its definition on the engine's own buffers
    want_num = (D_cur.double() - D_ref.double()).abs().sum(dim=(1, 2))
    want_den = D_ref.double().abs().sum(dim=(1, 2))
    print(f"[block cache] {name}: probe {probe.tolist()}, from the buffers num {want_num.tolist()} den {want_den.tolist()}")
    assert float(((probe[:, 0].double() - want_num).abs() / want_num).max()) <= 1e-4
    assert float(((probe[:, 1].double() - want_den).abs() / want_den).max()) <= 1e-4
    # tokens_out: the oracle's FinalLayer on that same stream
    wf = {k: (v.to(E).float() if E == F16 else v.float()) for k, v in named.items()}
    res = {}
    for pname, P in (("fp32", Prec()), ("emu", Prec(E))):
        # (an fp16 engine against the fp32 oracle: the timestep embedding in the model's own dtype, as tests/test_gpu_f16_model.py's oracles)
        m = OracleMMDiT(cfg, wf, P, embed_prec=Prec(embed_dtype(cfg)) if E == F16 else None)
        m.cache_modulation_params(inp_a["pooled"], torch.tensor(TS))
        mod = m._mod["final_layer"][TS[b]].chunk(2, dim=-1)
        res[pname] = m._lin(affine_transform(X[:, S_t:].float(), mod[0], mod[1], cfg.layer_norm_eps, P), "final_layer.linear")
    yardstick_ok(out.float(), res["emu"], res["fp32"], f"{name}: FinalLayer behind the reuse tail")


# ---- 4. closed loop through denoise_latents ----------------------------------------------------------------------------------------------
class CachedOracle:
    """OracleMMDiT's own pieces in the order of the cached step, as a model ``oracle.pipeline.cfg_denoise`` can call: call number i of a run
    (``cache_modulation_params`` starts one) reuses iff i is in ``skip``.  D, R and the reuse are rounded through the model's Prec.r."""

    def __init__(self, cfg, weights, P, skip):
        self.m, self.cfg, self.P, self.skip = OracleMMDiT(cfg, weights, P), cfg, P, frozenset(skip)
        self.step, self.R, self.D_ref, self.rel = 0, None, None, []

    def cache_modulation_params(self, pooled, timesteps):
        self.m.cache_modulation_params(pooled, timesteps)
        self.step, self.R, self.D_ref, self.rel = 0, None, None, []

    def __call__(self, latent, text, timestep):
        m, cfg, P = self.m, self.cfg, self.P
        tkey = float(timestep)
        B, Hl, Wl, _ = latent.shape
        txt = m._lin(P.r(text), "context_embedder")
        img0 = m._patch_embed(P.r(latent))
        S_t = txt.shape[1]
        rope = rope_table(cfg, S_t, Hl // cfg.patch_size, Wl // cfg.patch_size) if cfg.rope_axes_dim is not None else None
        img1, txt = m._double_block(0, img0, txt, tkey, rope)
        D = P.r(img1 - img0)
        if self.D_ref is None:
            self.rel.append(math.inf)
        else:
            num, den = (D - self.D_ref).abs().sum(dim=(1, 2)), self.D_ref.abs().sum(dim=(1, 2))
            self.rel.append(float((num / den).max()))
        if self.step in self.skip:
            img = P.r(img1 + self.R)
        else:
            img = img1
            for i in range(1, cfg.depth_multimodal):
                img, txt = m._double_block(i, img, txt, tkey, rope)
            if cfg.depth_unified > 0:
                x = torch.cat([txt, img], dim=1)
                for i in range(cfg.depth_unified):
                    x = m._single_block(i, x, tkey, rope)
                img = x[:, S_t:]
            self.R, self.D_ref = P.r(img - img1), D
        self.step += 1
        mod = m._mod["final_layer"][tkey].chunk(2, dim=-1)
        y = m._lin(affine_transform(img, mod[0], mod[1], cfg.layer_norm_eps, P), "final_layer.linear")
        return m._unpatch(y, Hl, Wl)


LOOP = {"flux": (tiny_flux(), 1.0, 0.0, False), "sd3_cfg": (tiny_sd3(), 3.0, 5.0, False), "flux_masked": (tiny_flux(), 1.0, 0.0, True)}
STEPS, HL, WL, SEED = 4, 8, 8, 0
RGB, HALF = make_image(HL * 8, WL * 8, seed=1), half_mask(HL * 8, WL * 8)


@functools.lru_cache(maxsize=None)
def loop_inputs(name):
    cfg, shift, cfgw, _ = LOOP[name]
    rows = 2 if cfgw > 0 else 1
    return randn(rows, 16, cfg.token_level_text_embed_dim, seed=7), randn(rows, cfg.pooled_text_embed_dim, seed=8)


def loop_pipe(name, dev):
    from diffusionkit_amd.pipeline import DiffusionPipeline, FluxPipeline
    cfg, shift, _, _ = LOOP[name]
    kw = dict(w16=True, a16=True, shift=shift, mmdit_config=cfg, vae_config=tiny_vae(), vae_encoder_config=tiny_vae_encoder(), device=dev, text_len=16)
    return FluxPipeline(**kw) if cfg.is_flux else DiffusionPipeline(model_version="argmaxinc/mlx-stable-diffusion-3-medium", **kw)


def loop_run(pipe, name, dev, block_cache):
    _, _, cfgw, masked = LOOP[name]
    text, pooled = loop_inputs(name)
    kw = dict(image_path=RGB, mask_path=HALF) if masked else {}
    if block_cache is not None:
        kw["block_cache"] = block_cache
    lat, iter_time = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=STEPS, cfg_weight=cfgw, latent_size=(HL, WL), seed=SEED, **kw)
    assert lat.shape == (1, HL, WL, 16) and lat.dtype == torch.float32 and len(iter_time) == STEPS
    return lat.cpu(), pipe.last_block_cache


@pytest.mark.parametrize("name", list(LOOP))
def test_closed_loop(dev, name):
    """4 steps, latent 8 x 8, seed 0.  threshold 0 is the run without the option bit for bit; inf skips exactly steps 1 and 2; FixedSchedule([1, 2])
    takes the same decisions and stays within the project's gates of the restated loop (fp32 and bf16-emulating) taking them too."""
    cfg, shift, cfgw, masked = LOOP[name]
    pipe = loop_pipe(name, dev)
    plain, rec = loop_run(pipe, name, dev, None)
    assert rec is None and not pipe.mmdit.block_cache
    zero, rec = loop_run(pipe, name, dev, 0.0)
    print(f"[block cache] {name} threshold 0: {rec}")
    assert same_bits(zero, plain), "block_cache=0.0 differs from block_cache=None"
    assert rec["threshold"] == 0.0 and rec["skipped"] == [] and rec["computed"] == [0, 1, 2, 3] and len(rec["rel"]) == STEPS
    assert rec["rel"][0] == math.inf and all(0.0 < r < math.inf for r in rec["rel"][1:])
    rels_all_computed = rec["rel"]
    inf_run, rec = loop_run(pipe, name, dev, float("inf"))
    print(f"[block cache] {name} threshold inf: {rec}")
    assert rec["skipped"] == [1, 2] and rec["computed"] == [0, 3]
    assert not same_bits(inf_run, plain) and bool(torch.isfinite(inf_run).all())
    fixed, rec = loop_run(pipe, name, dev, FixedSchedule([1, 2]))
    assert rec["skipped"] == [1, 2] and rec["computed"] == [0, 3] and rec["threshold"] is None
    assert same_bits(fixed, inf_run), "the same decisions must give the same latent"
    rels_skipped = rec["rel"]
    again, rec = loop_run(pipe, name, dev, None)  # (and the option leaves nothing behind)
    assert rec is None and same_bits(again, plain)
    # the restatement
    text, pooled = loop_inputs(name)
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    fmt = "flux" if cfg.is_flux else "sd3"
    t_act = None if cfg.is_flux else Prec(F16)  # SD3 timesteps: fp16 (quirk Q1)
    res, rels = {}, {}
    for pname, P in (("fp32", Prec()), ("emu", Prec(BF))):
        m = CachedOracle(cfg, wf, P, [1, 2])
        if masked:  # (from the pipeline's own encoded image: the VAE encoder's error is in none of the three)
            x_orig = pipe.latent_format.process_in(pipe.encode_image_to_latents(RGB, seed=SEED)).cpu()
            sigmas = op.get_sigmas(shift, cfg.is_flux, STEPS)
            x = masked_sample_euler(m, x_orig, latent_mask(HALF), SEED, sigmas, text, pooled, cfgw, Prec(BF), t_act=t_act)
            res[pname] = op.process_out(x, fmt)
        else:
            res[pname] = op.denoise_latents(m, text, pooled, STEPS, cfgw, (HL, WL), SEED, shift, cfg.is_flux, Prec(BF), t_act=t_act)
        rels[pname] = m.rel
    print(f"[block cache] {name}: rel per step, engine (all computed) {rels_all_computed}, engine (1, 2 skipped) {rels_skipped}, "
          f"restatement fp32 {rels['fp32']}, bf16-emulating {rels['emu']}")
    yardstick_ok(fixed, res["emu"], res["fp32"], f"{name}: steps 1 and 2 skipped")
    psnr_ok(fixed, res["emu"], res["fp32"], f"{name}: steps 1 and 2 skipped")


def test_generate_image_and_cli_record(dev, tmp_path):
    """generate_image(block_cache=) keeps the reference's return shape and logs the record; --block-cache reaches it"""
    from diffusionkit_amd import cli
    pipe = loop_pipe("flux", dev)
    img, log = pipe.generate_image("a cat", num_steps=STEPS, latent_size=(HL, WL), seed=SEED, verbose=False, block_cache=float("inf"))
    assert img.size == (WL * 8, HL * 8) and log["denoising"]["block_cache"]["skipped"] == [1, 2] and len(log["denoising"]["iter_time"]) == STEPS
    _, log = pipe.generate_image("a cat", num_steps=STEPS, latent_size=(HL, WL), seed=SEED, verbose=False)
    assert "block_cache" not in log["denoising"] and pipe.last_block_cache is None
    over = dict(mmdit_config=tiny_flux(), vae_config=tiny_vae(), text_len=20)
    argv = ["--prompt", "a cat", "--steps", "4", "--seed", "7", "--height", "64", "--width", "64", "-o", str(tmp_path / "out.png")]
    _, log = cli.main(argv + ["--block-cache", "inf"], pipeline_overrides=over)
    assert log["denoising"]["block_cache"]["skipped"] == [1, 2] and log["denoising"]["block_cache"]["threshold"] == math.inf


# ---- 5. state -------------------------------------------------------------------------------------------------------------------------------
def test_state_errors_name_the_rule(dev):
    from diffusionkit_amd._lib import DkHipError
    shape = (2, 8, 12, 20)
    eng, _ = engine_for(tiny_flux(), dev)
    inp = inputs_for(eng, dev, *shape)
    with pytest.raises(DkHipError, match="block cache"):  # the option is off
        tok = start(eng, shape, inp, False)
        eng.forward_head(tok, inp["text_dev"], 0)
    tok = start(eng, shape, inp, True)
    with pytest.raises(DkHipError, match="pending head"):  # a tail without a head
        eng.forward_tail(0, False)
    eng.forward_head(tok, inp["text_dev"], 0)
    with pytest.raises(DkHipError, match="valid cache"):  # reuse right after prepare: nothing was computed yet
        eng.forward_tail(0, True)
    eng.forward_tail(0, False)  # (the refused call left the head pending)
    with pytest.raises(DkHipError, match="pending head"):  # ... and a tail consumes it
        eng.forward_tail(0, False)
    eng.forward_head(tok, inp["text_dev"], 1)
    with pytest.raises(DkHipError, match="same step"):  # a tail for another step than the pending head
        eng.forward_tail(2, True)
    want = eng.forward_tail(1, True).cpu()
    eng.cache_modulation_params(inp["pooled_dev"], TS)  # new modulation parameters: the cache is no longer theirs
    eng.forward_head(tok, inp["text_dev"], 1)
    with pytest.raises(DkHipError, match="valid cache"):
        eng.forward_tail(1, True)
    eng.forward_tail(1, False)
    eng.forward_head(tok, inp["text_dev"], 2)
    eng.forward_tokens(tok, inp["text_dev"], 2)  # dk_mmdit_forward drops the pending head and keeps the cache
    with pytest.raises(DkHipError, match="pending head"):
        eng.forward_tail(2, True)
    eng.forward_head(tok, inp["text_dev"], 2)
    eng.forward_tail(2, True)
    eng.reset_block_cache()
    eng.forward_head(tok, inp["text_dev"], 2)
    with pytest.raises(DkHipError, match="valid cache"):
        eng.forward_tail(2, True)
    assert bool(torch.isfinite(want.float()).all())


def compute_reuse_compute(eng, shape, inp):
    tok = start(eng, shape, inp, True)
    outs = []
    for i, reuse in enumerate((False, True, False)):
        probe = eng.forward_head(tok, inp["text_dev"], i)
        outs += [probe.cpu(), eng.forward_tail(i, reuse).cpu()]
    torch.cuda.synchronize()
    return tuple(outs)


@pytest.mark.parametrize("name,cfg,shape", [("flux", tiny_flux(), (2, 8, 12, 20)), ("flux_fp8", FP8, (1, 8, 8, 128))])
def test_exact_size_poisoned_workspace(dev, name, cfg, shape):
    """compute, reuse, compute in a workspace of exactly dk_mmdit_workspace_bytes bytes filled with 0xFF (NaN in every element type): nothing
    outside it is written, and probes and tokens equal the same run in a zero-filled workspace bit for bit"""
    from diffusionkit_amd.engine import MMDiTEngine
    packed = pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1234), dev)
    eng0 = MMDiTEngine(cfg, packed)
    inp = inputs_for(eng0, dev, *shape)
    off = eng0.lib.dk_mmdit_workspace_bytes(eng0._h, *shape, len(TS))
    eng0.enable_block_cache(True)
    nbytes = eng0.lib.dk_mmdit_workspace_bytes(eng0._h, *shape, len(TS))
    assert nbytes > off
    ws = es.GuardedWorkspace(nbytes, dev)
    outs = {}
    for label, fill in (("zero", es.FILL_ZERO), ("nan", es.FILL_NAN)):
        eng = MMDiTEngine(cfg, packed)
        eng.enable_block_cache(True)
        ws.fill(fill)
        es.lend(eng, ws, nbytes)
        outs[label] = compute_reuse_compute(eng, shape, inp)
        assert eng._ws.data_ptr() == ws.interior(nbytes).data_ptr() and eng._ws.numel() == nbytes
        ws.check(nbytes, f"{name} block cache [{label}]", fill=fill)
    es.assert_identical(outs, f"{name}: compute, reuse, compute")


PINNED = [(tiny_flux(), (1, 8, 8, 16, 3), 136310272), (tiny_sd3(), (2, 8, 8, 16, 3), 67543040)]  # tests/test_abi_and_host.py's values


@pytest.mark.parametrize("cfg,args,want", PINNED, ids=["flux", "sd3"])
def test_cache_off_keeps_the_workspace_bytes(dev, cfg, args, want):
    """with the cache off dk_mmdit_workspace_bytes is the parent's value: before the option was ever touched and after on / off again"""
    eng, _ = engine_for(cfg, dev)
    before = eng.lib.dk_mmdit_workspace_bytes(eng._h, *args)
    eng.enable_block_cache(True)
    on = eng.lib.dk_mmdit_workspace_bytes(eng._h, *args)
    eng.enable_block_cache(False)
    after = eng.lib.dk_mmdit_workspace_bytes(eng._h, *args)
    print(f"[block cache] workspace bytes {args}: off {before}, on {on}, off again {after}")
    assert before == want and after == want and on > want
