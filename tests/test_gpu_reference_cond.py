"""Reference-image conditioning (FLUX.1 Kontext's token layout) on the GPU: the RoPE table for two grids, the engine against the oracle of
tests/_refcond.py on sharpened weights -- its output, the EFFECT of the reference (so that an engine that ignores or misplaces it fails), and
the reference rows of the stream themselves -- the hoist, "off means off", poisoned state, the first-block cache, fp8, and the pipeline.

Arithmetic parity only: no Kontext checkpoint exists where this suite runs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from diffusionkit_amd import _lib, ops
from diffusionkit_amd.config import fp8_config, tiny_flux, tiny_vae, tiny_vae_encoder
from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights, synth_vae_encoder_weights
from oracle import fp8 as o8
from oracle import pipeline as op
from oracle.mmdit import OracleMMDiT, Prec, affine_transform, rope_table
from oracle.vae import OracleVAEEncoder, sample_latent
from tests import _engine_state as es
from tests import _footprint as fp
from tests import _refcond as rc
from tests._util import BF, psnr, randn, rel_l2

pytestmark = pytest.mark.gpu

bits = fp.bits
TS, STEP = rc.TIMESTEPS, rc.STEP
CASE_NAMES = list(rc.CASES)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


def yardstick_ok(hip, emu, exact, what=""):
    """the project's model-level rule (tests/test_gpu_model.py): hip-vs-fp32 <= 2 * emu-vs-fp32 + 2e-3 (relative L2)"""
    e_h, e_e = rel_l2(exact, hip), rel_l2(exact, emu)
    print(f"[reference] {what}: rel_l2 hip-vs-fp32 {e_h:.3e}, emu-vs-fp32 {e_e:.3e}")
    assert e_h <= 2.0 * e_e + 2e-3, f"{what}: hip-vs-fp32 {e_h:.3e} > 2*emu-vs-fp32 {e_e:.3e} + 2e-3"
    return e_h, e_e


def psnr_ok(hip, emu, exact, what=""):
    """tests/test_gpu_model.py: >= 35 dB against the fp32 oracle, or within 1.5 dB of what the bf16-emulating oracle reaches"""
    p_h, p_e = psnr(exact, hip), psnr(exact, emu)
    print(f"[reference] {what}: PSNR hip {p_h:.1f} dB, bf16-emulating oracle {p_e:.1f} dB")
    assert p_h > min(35.0, p_e - 1.5), f"{what}: PSNR hip {p_h:.1f} dB, bf16-emulating oracle {p_e:.1f} dB"


# ---- 1. the table ----------------------------------------------------------------------------------------------------------------------
AXES, THETA = (16, 56, 56), 10000.0


@pytest.mark.parametrize("S_t,gh,gw", [(5, 8, 73), (20, 4, 6)])
def test_rope_table_segments(dev, S_t, gh, gw):
    rh, rw = 3, 5
    one = ops.rope_table(S_t, gh, gw, AXES, THETA, dev)
    seg1 = ops.rope_table_segments(S_t, [(gh, gw, 0)], AXES, THETA, dev)
    assert same_bits(seg1, one), "one segment (gh, gw, 0) != dk_rope_table_f32"
    two = ops.rope_table_segments(S_t, [(gh, gw, 0), (rh, rw, 1)], AXES, THETA, dev)
    S_i, S_r, a0 = gh * gw, rh * rw, AXES[0] // 2
    assert two.shape == (S_t + S_i + S_r, sum(AXES) // 2, 2)
    assert same_bits(two[:S_t + S_i].contiguous(), one), "the first rows of the two-segment table != the one-segment table"
    own = ops.rope_table_segments(S_t, [(rh, rw, 0)], AXES, THETA, dev)  # the same kernel on the reference grid alone
    assert same_bits(two[S_t + S_i:, a0:].contiguous(), own[S_t:, a0:].contiguous()), "reference rows, axes 1 and 2"
    # axis 0 at index 1: cos / sin of omega itself -- within what the one-grid table already differs from the CPU table by (measured here)
    cfg = tiny_flux()
    assert tuple(cfg.rope_axes_dim) == AXES and float(cfg.rope_theta) == THETA
    bound = float((one.cpu() - rope_table(cfg, S_t, gh, gw)).abs().max())
    want = rc.rope_table_ext(cfg, S_t, gh, gw, rh, rw)
    err0 = float((two[S_t + S_i:, :a0].cpu() - want[S_t + S_i:, :a0]).abs().max())
    print(f"[reference] table ({S_t}, {gh}, {gw}): one-grid table vs CPU max |d| {bound:.3e}, reference rows axis 0 {err0:.3e}")
    assert err0 <= bound, (err0, bound)
    assert bool((two[S_t + S_i:, :a0, 0] < 1.0).any()), "axis 0 of the reference rows is at index 0"


def test_rope_table_segments_refuses(dev):
    with pytest.raises(_lib.DkHipError, match="segments"):
        ops.rope_table_segments(4, [], AXES, THETA, dev)
    with pytest.raises(_lib.DkHipError, match="1 to 4"):
        ops.rope_table_segments(4, [(2, 2, i) for i in range(5)], AXES, THETA, dev)


# ---- the engine on the cases of tests/_refcond.py ------------------------------------------------------------------------------------------
def build(dev, cfg=None):
    from diffusionkit_amd.engine import MMDiTEngine
    cfg = cfg or tiny_flux()
    named = rc.sharpened_weights(cfg)
    return MMDiTEngine(cfg, pack_mmdit(cfg, named, dev)), named


def peek(eng, which, shape):
    """a copy of one of the engine's internal buffers (dk_mmdit_debug_buffer) on the host"""
    torch.cuda.synchronize()
    ptr = eng.lib.dk_mmdit_debug_buffer(eng._h, which)
    assert ptr, f"debug buffer {which} is NULL"
    t = torch.empty(shape, dtype=eng.dtype, device=eng._ws.device)
    hip = ctypes.CDLL("libamdhip64.so")  # (kind 3: device to device)
    assert hip.hipMemcpy(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t(t.numel() * t.element_size()), 3) == 0
    return t.cpu()


def geometry(eng, name):
    B, (Hl, Wl), S_t, (rh, rw) = rc.CASES[name]
    p = eng.config.patch_size
    return B, S_t, (Hl // p) * (Wl // p), (rh // p) * (rw // p), eng.config.hidden_size


def start(eng, name, dev, ref=True, per_image=True, block_cache=False):
    """prepare + cache for a case -> (tokens, text) on the device; ``ref`` False: the same inputs on an engine without a reference grid"""
    B, (Hl, Wl), S_t, rhw = rc.CASES[name]
    text, pooled, lat, r = rc.case_inputs(eng.config, name)
    eng.enable_block_cache(block_cache)
    eng.prepare(B, (Hl, Wl), S_t, len(TS), reference_size=rhw if ref else None)
    eng.cache_modulation_params(pooled.to(dev), TS)
    if ref:
        eng.cache_reference((r if per_image else r[:1]).to(dev), per_image=per_image)
    return eng.patchify(lat.to(dev)), text.to(dev, eng.dtype)


@functools.lru_cache(maxsize=None)
def engine_case(dev, name):
    """one engine run per case, shared by the tests below (read-only): tokens with the reference, the joint stream behind the last block,
    and the tokens of a no-reference engine on the same inputs"""
    eng, _ = build(dev)
    B, S_t, S_i, S_r, h = geometry(eng, name)
    tok, text = start(eng, name, dev)
    out = eng.forward_tokens(tok, text, STEP).cpu()
    stream = peek(eng, 0, (B, S_t + S_i + S_r, h))
    eng0, _ = build(dev)
    tok0, text0 = start(eng0, name, dev, ref=False)
    out0 = eng0.forward_tokens(tok0, text0, STEP).cpu()
    return {"out": out, "stream": stream, "out0": out0}


# ---- 2. output parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_output_parity(dev, name):
    got, res = engine_case(dev, name), rc.oracle_case(name)
    f, e = res["fp32"][STEP], res["emu"][STEP]
    assert got["out"].shape == f["final"].shape and bool(torch.isfinite(got["out"].float()).all())
    yardstick_ok(got["out"].float(), e["final"], f["final"], f"{name}: tokens_out")
    psnr_ok(got["out"].float(), e["final"], f["final"], f"{name}: tokens_out")


# ---- 3. the reference matters, and matters correctly ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_reference_effect(dev, name):
    """delta = out(reference) - out(no reference): 1.0 for an engine that ignores the reference, 1.2 for one that walks its grid transposed,
    0.25 - 0.30 for one that leaves it at index 0 (measured on the oracle); the bound is twice the bf16-emulating oracle's own figure + 0.02"""
    got, res = engine_case(dev, name), rc.oracle_case(name)
    f, e = res["fp32"][STEP], res["emu"][STEP]
    d32, de = f["final"] - f["final0"], e["final"] - e["final0"]
    dh = got["out"].float() - got["out0"].float()
    share, e_e, e_h = float(d32.norm() / f["final"].norm()), rel_l2(d32, de), rel_l2(d32, dh)
    print(f"[reference] {name}: delta is {share:.3f} of the output norm; rel_l2(delta) hip-vs-fp32 {e_h:.3f}, emu-vs-fp32 {e_e:.3f}")
    assert share >= 0.05, "the inputs stopped discriminating"
    assert e_e <= 0.2, "the bf16-emulating oracle no longer reproduces the reference's effect: the bound below would say nothing"
    assert e_h <= 2.0 * e_e + 0.02, f"{name}: the reference's effect on the output: {e_h:.3f} > 2 * {e_e:.3f} + 0.02"


# ---- 4. the reference rows themselves ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_stream_rows(dev, name):
    got, res = engine_case(dev, name), rc.oracle_case(name)
    f, e = res["fp32"][STEP]["stream"], res["emu"][STEP]["stream"]
    x = got["stream"].float()
    B, (Hl, Wl), S_t, _ = rc.CASES[name]
    S_i = (Hl // 2) * (Wl // 2)
    assert x.shape == f.shape
    for what, sl in (("text rows", slice(0, S_t)), ("image rows", slice(S_t, S_t + S_i)), ("reference rows", slice(S_t + S_i, None))):
        yardstick_ok(x[:, sl], e[:, sl], f[:, sl], f"{name}: {what} of the final stream")


# ---- 5. hoist and broadcast ----------------------------------------------------------------------------------------------------------------
def test_broadcast_equals_per_image(dev):
    name = "A2"
    eng, _ = build(dev)
    B, (Hl, Wl), S_t, rhw = rc.CASES[name]
    _, _, _, r = rc.case_inputs(eng.config, name)
    tok, text = start(eng, name, dev, per_image=False)  # (one reference, r[:1], for both batch rows)
    one = eng.forward_tokens(tok, text, STEP).cpu()
    eng.cache_reference(r[:1].repeat(B, 1, 1, 1).to(dev), per_image=True)
    rep = eng.forward_tokens(tok, text, STEP).cpu()
    assert same_bits(one, rep), "per_image = 0 != per_image = 1 with the reference repeated"
    eng.cache_reference(r.to(dev), per_image=True)
    assert not same_bits(eng.forward_tokens(tok, text, STEP).cpu(), one), "another reference for batch row 1 changed nothing"


def test_hoisted_reference_serves_every_step(dev):
    name, steps = "A1", (0, 2)
    eng, _ = build(dev)
    tok, text = start(eng, name, dev)
    res = rc.oracle_case(name, steps=steps)
    for s in steps:  # (one cache_reference in front of both)
        out = eng.forward_tokens(tok, text, s).float().cpu()
        yardstick_ok(out, res["emu"][s]["final"], res["fp32"][s]["final"], f"{name}: step {s}")
        psnr_ok(out, res["emu"][s]["final"], res["fp32"][s]["final"], f"{name}: step {s}")


def test_forward_without_cached_reference_is_refused(dev):
    name = "A1"
    eng, _ = build(dev)
    B, (Hl, Wl), S_t, rhw = rc.CASES[name]
    text, pooled, lat, r = rc.case_inputs(eng.config, name)
    eng.prepare(B, (Hl, Wl), S_t, len(TS), reference_size=rhw)
    eng.cache_modulation_params(pooled.to(dev), TS)
    tok = eng.patchify(lat.to(dev))
    with pytest.raises(_lib.DkHipError, match="dk_mmdit_cache_reference"):
        eng.forward_tokens(tok, text.to(dev, BF), STEP)
    S = S_t + tok.shape[1] + eng.reference_tokens()
    with pytest.raises(_lib.DkHipError, match="dk_mmdit_cache_reference"):
        eng.run_blocks(torch.zeros(B, S, eng.config.hidden_size, dtype=BF, device=dev), STEP, 0)
    eng.cache_reference(r.to(dev), per_image=True)
    eng.forward_tokens(tok, text.to(dev, BF), STEP)
    eng.prepare(B, (Hl, Wl), S_t, len(TS) + 1, reference_size=rhw)  # (prepare invalidates it)
    eng.cache_modulation_params(pooled.to(dev), TS)
    with pytest.raises(_lib.DkHipError, match="dk_mmdit_cache_reference"):
        eng.forward_tokens(tok, text.to(dev, BF), STEP)
    with pytest.raises(_lib.DkHipError, match="reference latent"):  # (another grid than the prepared one)
        eng.cache_reference(r[:, :4].contiguous().to(dev), per_image=True)
    with pytest.raises(_lib.DkHipError, match="reference tokens shape"):  # (two references, one batch row)
        eng.cache_reference(torch.cat([r, r], 0).to(dev), per_image=True)


# ---- 6. off means off ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A2", "B"])
def test_grid_off_again_equals_never_on(dev, name):
    eng, _ = build(dev)
    tok, text = start(eng, name, dev)
    eng.forward_tokens(tok, text, STEP)
    tok, text = start(eng, name, dev, ref=False)
    out = eng.forward_tokens(tok, text, STEP).cpu()
    assert same_bits(out, engine_case(dev, name)["out0"]), "an engine whose reference grid was turned off != one that never had it"
    fresh, _ = build(dev)
    B, (Hl, Wl), S_t, _ = rc.CASES[name]
    assert eng.lib.dk_mmdit_workspace_bytes(eng._h, B, Hl, Wl, S_t, len(TS)) == fresh.lib.dk_mmdit_workspace_bytes(fresh._h, B, Hl, Wl, S_t, len(TS))


def tiny_pipe(dev):
    from diffusionkit_amd.pipeline import FluxPipeline
    return FluxPipeline(w16=True, a16=True, mmdit_config=tiny_flux(), vae_config=tiny_vae(), vae_encoder_config=tiny_vae_encoder(), device=dev,
                        text_len=16)


def test_generate_image_without_the_keyword(dev):
    pipe = tiny_pipe(dev)
    img_a, log_a = pipe.generate_image("a cat", num_steps=2, latent_size=(8, 12), seed=3, verbose=False)
    img_b, log_b = pipe.generate_image("a cat", num_steps=2, latent_size=(8, 12), seed=3, verbose=False, reference_image_path=None)
    assert img_a.tobytes() == img_b.tobytes()
    assert set(log_a) == set(log_b) and set(log_a["denoising"]) == set(log_b["denoising"]) and "reference" not in log_a["denoising"]
    assert pipe.last_reference is None


# ---- 7. state --------------------------------------------------------------------------------------------------------------------------------
FP8 = fp8_config(tiny_flux(), "speed")


@pytest.mark.parametrize("name,cfg", [("A2", None), ("B", None), ("B", FP8)], ids=["A2", "B", "B-fp8"])
def test_exact_size_poisoned_workspace(dev, name, cfg):
    """an exact-size workspace that is all NaN before prepare, and NaN slack behind tokens_out: finite outputs, the bits of a clean run"""
    B, (Hl, Wl), S_t, rhw = rc.CASES[name]
    outs = {}
    for label, fill in (("zeros", es.FILL_ZERO), ("nan", es.FILL_NAN)):
        eng, _ = build(dev, cfg)
        _lib.check(eng.lib.dk_mmdit_set_reference_grid(eng._h, *rhw), "dk_mmdit_set_reference_grid")
        eng.reference_size = tuple(rhw)
        nbytes = eng.lib.dk_mmdit_workspace_bytes(eng._h, B, Hl, Wl, S_t, len(TS))
        ws = es.GuardedWorkspace(nbytes, dev)
        ws.fill(fill)
        es.lend(eng, ws, nbytes)
        tok, text = start(eng, name, dev)
        assert eng._ws.data_ptr() == ws.interior(nbytes).data_ptr(), "the engine did not keep the lent workspace"
        n = tok.numel()
        slab = torch.full((n + 4096,), float("nan"), dtype=eng.dtype, device=dev)
        out = eng.forward_tokens(tok, text, STEP, tokens_out=slab[:n].view(tok.shape))
        torch.cuda.synchronize()
        ws.check(nbytes, f"{name} ({label})", fill)
        assert bool(torch.isnan(slab[n:].float()).all()), "the slack behind tokens_out was written"
        outs[label] = out.clone().cpu()
    if cfg is None:
        outs["plain"] = engine_case(dev, name)["out"]
    es.assert_identical(outs, f"{name}: poisoned exact-size workspace")


# ---- 8. first-block cache ------------------------------------------------------------------------------------------------------------------
def test_block_cache_reuse_tail_with_reference(dev):
    """the header's definition with a reference: X1 + R on the S_i image rows, text AND reference rows as block 0 left them, then the final layer"""
    name = "A2"
    eng, named = build(dev)
    B, S_t, S_i, S_r, h = geometry(eng, name)
    S = S_t + S_i + S_r
    tok, text = start(eng, name, dev, block_cache=True)
    _, pooled, _, _ = rc.case_inputs(eng.config, name)
    a, b = 0, 1
    probe = eng.forward_head(tok, text, a).cpu()
    assert probe.shape == (B, 2) and bool((probe[:, 1] == 0).all())
    eng.forward_tail(a, False)
    R = peek(eng, 3, (B, S_i, h))
    assert int(bits(R).ne(0).sum()) > 0 and bool(torch.isfinite(R.float()).all())
    eng.forward_head(tok, text, b)
    X1 = peek(eng, 0, (B, S, h))
    out = eng.forward_tail(b, True).cpu()
    X = peek(eng, 0, (B, S, h))
    img = slice(S_t, S_t + S_i)
    assert same_bits(X[:, img], (X1[:, img].float() + R.float()).to(BF)), "image rows != round(X1 + R)"
    assert same_bits(X[:, :S_t], X1[:, :S_t]), "the reuse tail touched the text rows"
    assert same_bits(X[:, S_t + S_i:], X1[:, S_t + S_i:]), "the reuse tail touched the reference rows"
    wf = {k: v.float() for k, v in named.items()}
    res = {}
    for pname, P in (("fp32", Prec()), ("emu", Prec(BF))):
        m = OracleMMDiT(eng.config, wf, P)
        m.cache_modulation_params(pooled, torch.tensor(TS))
        mod = m._mod["final_layer"][TS[b]].chunk(2, dim=-1)
        res[pname] = m._lin(affine_transform(X[:, img].float(), mod[0], mod[1], eng.config.layer_norm_eps, P), "final_layer.linear")
    yardstick_ok(out.float(), res["emu"], res["fp32"], "FinalLayer behind the reuse tail")
    # head + compute tail = forward
    eng.reset_block_cache()
    eng.forward_head(tok, text, STEP)
    assert same_bits(eng.forward_tail(STEP, False).cpu(), engine_case(dev, name)["out"]), "head + compute tail != dk_mmdit_forward"


# ---- 9. fp8 --------------------------------------------------------------------------------------------------------------------------------
def test_fp8_with_reference(dev):
    """case B on the all-fp8 engine.  tests/test_gpu_fp8.py's tiny model-forward test (test_mmdit_fp8_tiny) bounds the engine against the
    fake-quantising oracle (2 * emu + 2e-3, > 35 dB) and, against the un-quantised model, by what the bf16-emulating fake-quant oracle reaches
    less 3 dB; the same three here, the un-quantised model being the bf16 ENGINE's output for the case"""
    name = "B"
    eng, named = build(dev, FP8)
    tok, text = start(eng, name, dev)
    out = eng.forward_tokens(tok, text, STEP).float().cpu()
    assert bool(torch.isfinite(out).all())
    cfg = FP8
    t, pooled, lat, r = rc.case_inputs(cfg, name)
    fq, paq = o8.fake_quant_block_weights(cfg, named), o8.policy_act_quant(cfg)
    res = {}
    for pname, P in (("fq_emu", Prec(BF)), ("fq_fp32", Prec())):
        m = rc.RefCondMMDiT(cfg, fq, P, act_quant=paq)
        m.cache_modulation_params(pooled, torch.tensor(TS))
        taps = {}
        m(lat, t, TS[STEP], taps=taps, ref=r)
        res[pname] = taps["final"]
    bf16 = engine_case(dev, name)["out"].float()
    e_h, e_e = rel_l2(res["fq_fp32"], out), rel_l2(res["fq_fp32"], res["fq_emu"])
    p_fq, p_h, p_e = psnr(res["fq_fp32"], out), psnr(bf16, out), psnr(bf16, res["fq_emu"])
    print(f"[reference] fp8 {name}: rel_l2 vs fake-quant fp32 oracle {e_h:.3e} (bf16-emulating: {e_e:.3e}), PSNR {p_fq:.1f} dB; against the "
          f"bf16 engine {p_h:.1f} dB (bf16-emulating fake-quant oracle: {p_e:.1f} dB)")
    assert e_h <= 2.0 * e_e + 2e-3, (e_h, e_e)
    assert p_fq > 35.0
    assert p_h > p_e - 3.0


# ---- 10. the pipeline ------------------------------------------------------------------------------------------------------------------------
class WithReference:
    """a ``RefCondMMDiT`` with its reference bound, as a model ``oracle.pipeline`` can call"""

    def __init__(self, model, ref):
        self.model, self.ref = model, ref

    def cache_modulation_params(self, pooled, timesteps):
        self.model.cache_modulation_params(pooled, timesteps)

    def __call__(self, latent, text, timestep):
        return self.model(latent, text, timestep, ref=self.ref)


def reference_rgb(H=48, W=80, seed=4):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(yy * 255 // H), (xx * 255 // W), ((yy + xx) * 255 // (H + W))], -1)
    return np.clip(base + rng.randint(-20, 20, size=(H, W, 3)), 0, 255).astype(np.uint8)


def test_pipeline_with_reference(dev, tmp_path):
    from PIL import Image
    cfg, ecfg = tiny_flux(), tiny_vae_encoder()
    pipe = tiny_pipe(dev)
    rgb = reference_rgb()
    path = str(tmp_path / "ref.png")
    Image.fromarray(rgb).save(path)
    seeds = [0, 1]
    text = randn(1, 16, cfg.token_level_text_embed_dim, seed=7)
    pooled = randn(1, cfg.pooled_text_embed_dim, seed=8)
    run = lambda **kw: pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=2, cfg_weight=0.0, latent_size=(8, 12), seed=seeds,
                                            reference_image_path=path, **kw)
    lat, iter_time = run()
    assert lat.shape == (2, 8, 12, 16) and len(iter_time) == 2
    assert pipe.last_reference == {"size": (48, 80), "tokens": 15}
    assert pipe.mmdit.reference_size == (6, 10)
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    ewf = {k: v.float() for k, v in synth_vae_encoder_weights(ecfg, seed=1234 + 2).items()}
    image = torch.from_numpy((rgb.astype(np.float32) / 255) * 2 - 1.0)[None]
    res = {}
    for pname, P in (("fp32", Prec()), ("emu", Prec(BF))):
        hidden = OracleVAEEncoder(ecfg, ewf, P)(image)
        mean = sample_latent(hidden, torch.zeros(1, 6, 10, hidden.shape[-1] // 2))
        model = WithReference(rc.RefCondMMDiT(cfg, wf, P), op.process_in(mean, "flux"))
        res[pname] = torch.cat([op.denoise_latents(model, text, pooled, 2, 0.0, (8, 12), s, 1.0, True, Prec(BF)) for s in seeds], 0)
    p_h, p_e = psnr(res["fp32"], lat), psnr(res["fp32"], res["emu"])
    print(f"[reference] pipeline: final latent PSNR {p_h:.1f} dB against the closed-loop fp32 oracle (bf16-emulating oracle: {p_e:.1f} dB)")
    assert p_h > 35.0
    # a list with one reference per seed, the same image twice: the same latents
    lat2, _ = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=2, cfg_weight=0.0, latent_size=(8, 12), seed=seeds,
                                   reference_image_path=[path, rgb])
    assert same_bits(lat2.cpu(), lat.cpu())
    # the first-block cache at threshold 0 computes every step: the same latents
    lat3, _ = run(block_cache=0.0)
    assert same_bits(lat3.cpu(), lat.cpu()), "block_cache = 0 with a reference != no block cache"
    assert pipe.last_block_cache["skipped"] == []
    # the log, and the other step entries: they complete with finite output
    img, log = pipe.generate_image("a cat", num_steps=2, latent_size=(8, 12), seed=seeds, verbose=False, reference_image_path=path)
    assert log["denoising"]["reference"] == {"size": (48, 80), "tokens": 15} and img.size == (96, 128)
    lat4, _ = run(sampler="ab2")
    assert lat4.shape == lat.shape and bool(torch.isfinite(lat4).all())
    init = reference_rgb(64, 128, seed=5)
    mask = np.zeros((64, 128), dtype=np.uint8)
    mask[:, 64:] = 255
    lat5, _ = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=2, cfg_weight=0.0, latent_size=(8, 16), seed=seeds,
                                   image_path=init, mask_path=mask, reference_image_path=path)
    assert lat5.shape == (2, 8, 16, 16) and bool(torch.isfinite(lat5).all())
    # and the next call without the keyword runs without the reference rows
    pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=2, cfg_weight=0.0, latent_size=(8, 12), seed=seeds)
    assert pipe.mmdit.reference_size == (0, 0) and pipe.last_reference is None
