"""Engine state on an MI355X: poisoned exact-size workspaces and engine reuse (tests/_engine_state.py, proved in tests/test_engine_state_cpu.py).

Every engine (dk_mmdit_*, dk_vae_decode, dk_vae_encode) carves its buffers out of one caller-supplied workspace which the Python wrappers
allocate with torch.empty and keep when a later shape needs fewer bytes.  Some carved regions are written by no launch and read by tile-shaped
kernels (pad rows of the MX-fp8 buffers, the spare scale block, the [T, Tp) score columns, channel and pitch padding, the K-split slabs and the
attention key-split partials).  Three properties, none of which the single-run parity tests see:

  a. contents: the result does not depend on bytes the engine never wrote -- the same call sequence on a workspace filled with 0x00, with 0xFF
     (NaN in every element type, the E8M0 NaN code) and left stale by a run at a larger shape gives bit-identical, finite outputs;
  b. bounds: the workspace is exactly ``dk_*_workspace_bytes`` long between two 1 MiB margins, which are intact after every run;
  c. reuse: one engine object driven through a sequence of problems equals, bit for bit and at every stop, a fresh engine that has only ever
     seen that problem.

No tolerance appears: an assertion is bit equality with a run the suite already gates against the oracle (tiny cases are put through that
gate once more, from the 0xFF run), or byte equality of a guard.  The attention kernels clamp pad query rows to the last real row, so their
deferred-rescale vote is a function of real data, and bit equality is the right expectation for them too.

The file name sorts behind tests/test_gpu_fullsize.py on purpose (see the head of tests/test_gpu_vae_f16.py)."""
from dataclasses import replace

import numpy as np
import pytest
import torch

from diffusionkit_amd.config import (FLUX_SCHNELL, SD3_2b, VAEDecoderConfig, VAEEncoderConfig, float16_config, float16_vae_config, tiny_flux,
                                     tiny_sd3, tiny_vae, tiny_vae_encoder)
from diffusionkit_amd.weights import pack_mmdit, pack_vae, synth_mmdit_weights, synth_vae_encoder_weights, synth_vae_weights
from oracle import pipeline as op
from oracle.mmdit import OracleMMDiT, Prec
from oracle.vae import OracleVAEDecoder, OracleVAEEncoder
from tests import _engine_state as es
from tests._util import BF, bf16r, psnr, randn, rel_l2

pytestmark = pytest.mark.gpu

F16 = torch.float16
TS = [1000.0, 752.0, 500.0]
FILLS = (("zero", es.FILL_ZERO), ("nan", es.FILL_NAN))


@pytest.fixture(scope="module")
def packed_for(dev):
    """(config, seed) -> (source tensors, packed device tensors); a width-sized weight set is drawn once for all its cases and dropped with the module"""
    cache, drawn = {}, {}

    def get(cfg, seed=1234):
        if (cfg, seed) not in cache:
            # (the draw does not depend on the element types: one per geometry, shared by the bf16 / float16 / fp8 forms)
            geom = replace(cfg, activation_dtype="bfloat16", weight_dtype="bfloat16", fp8_bf16_double_blocks=0)
            if (geom, seed) not in drawn:
                drawn[(geom, seed)] = synth_mmdit_weights(geom, seed=seed)
            cache[(cfg, seed)] = (drawn[(geom, seed)], pack_mmdit(cfg, drawn[(geom, seed)], dev))
        return cache[(cfg, seed)]
    yield get
    cache.clear()
    drawn.clear()


def dtype_of(cfg):
    return F16 if cfg.activation_dtype == "float16" else BF


def mmdit_inputs(cfg, dev, B, Hl, Wl, S_t, seed0=0):
    """tests/test_gpu_model.py's forward_case inputs (seeds 3 / 4 / 5) for seed0 = 0"""
    dt = dtype_of(cfg)
    S = S_t + (Hl // cfg.patch_size) * (Wl // cfg.patch_size)
    return dict(text=randn(B, S_t, cfg.token_level_text_embed_dim, seed=seed0 + 3).to(dev, dt), pooled=randn(B, cfg.pooled_text_embed_dim, seed=seed0 + 4).to(dev),
                lat=randn(B, Hl, Wl, 16, seed=seed0 + 5).to(dev), x=randn(B, S, cfg.hidden_size, seed=seed0 + 840).to(dev, dt))


def mmdit_prepared_steps(eng, shape, inp, ts, before_forward=None):
    """prepare -> cache_modulation_params, then one thunk per output of mmdit_sequence (the interleaving tests call them in turn with other work)"""
    B, Hl, Wl, S_t = shape
    eng.prepare(B, (Hl, Wl), S_t, len(ts))
    eng.cache_modulation_params(inp["pooled"], ts)
    if before_forward is not None:
        before_forward(eng)
    tok = eng.patchify(inp["lat"])
    steps = [lambda i=i: eng.forward_tokens(tok, inp["text"], i) for i in range(len(ts))]
    return steps + [lambda: eng.run_blocks(inp["x"], len(ts) - 1, 0, eng.config.depth_multimodal + eng.config.depth_unified)]


def mmdit_sequence(eng, shape, inp, ts, before_forward=None):
    """prepare -> cache_modulation_params -> forward_tokens at every cached step -> run_blocks over the whole range; nothing refills the workspace
    in between (prepare writes the RoPE table, the cropped positional table and the K-split flags)"""
    outs = tuple(step() for step in mmdit_prepared_steps(eng, shape, inp, ts, before_forward))
    torch.cuda.synchronize()
    return outs


def mmdit_contents_case(dev, cfg, packed, shape, big, ts, what, after_run=None, before_forward=None):
    """the three runs of one case on one guarded allocation; returns label -> outputs.  ``big``: the strictly larger problem of the stale run."""
    from diffusionkit_amd.engine import MMDiTEngine
    probe = MMDiTEngine(cfg, packed)
    nbytes = probe.lib.dk_mmdit_workspace_bytes(probe._h, *shape, len(ts))
    nbig = probe.lib.dk_mmdit_workspace_bytes(probe._h, *big, len(ts))
    assert nbig > nbytes, (nbig, nbytes)
    ws = es.GuardedWorkspace(nbig, dev)
    inp, inp_big = mmdit_inputs(cfg, dev, *shape), mmdit_inputs(cfg, dev, *big, seed0=100)
    outs = {}

    def run(eng, label, fill):
        es.lend(eng, ws, nbytes)
        outs[label] = mmdit_sequence(eng, shape, inp, ts, before_forward)
        assert eng._ws.data_ptr() == ws.interior(nbytes).data_ptr() and eng._ws.numel() == nbytes  # (the wrapper kept the lent buffer)
        ws.check(nbytes, f"{what} [{label}]", fill=fill)
        if after_run is not None:
            after_run(eng, ws.interior(nbytes), label)

    for label, fill in FILLS:
        ws.fill(fill)
        run(MMDiTEngine(cfg, packed), label, fill)
    # stale: no refill -- the 0xFF run's leftovers under a run of the same engine at the larger shape, then the case's shape in the same buffer
    eng = MMDiTEngine(cfg, packed)
    es.lend(eng, ws, nbig)
    mmdit_sequence(eng, big, inp_big, ts)
    ws.check(nbig, f"{what} [the larger run in front of the stale one]", fill=es.FILL_NAN)
    run(eng, "stale", None)
    es.assert_identical(outs, what)
    return outs


# ---- 2a. MMDiT, tiny configurations: B = 2, latent 8 x 12, S_t = 20, three timesteps -------------------------------------------------------
def _oracle_finals(cfg, wf, inp_cpu, ts, step, precs, **kw):
    res = {}
    for name, (P, extra) in precs.items():
        m = OracleMMDiT(cfg, wf, P, **extra, **kw)
        m.cache_modulation_params(inp_cpu["pooled"], torch.tensor(ts))
        taps = {}
        m(inp_cpu["lat"], inp_cpu["text"], ts[step], taps=taps)
        res[name] = taps["final"]
    return res


def _cpu_inputs(cfg, B, Hl, Wl, S_t):
    return dict(text=randn(B, S_t, cfg.token_level_text_embed_dim, seed=3), pooled=randn(B, cfg.pooled_text_embed_dim, seed=4), lat=randn(B, Hl, Wl, 16, seed=5))


TINY_BF16 = [("flux", tiny_flux()),                                            # RoPE and single blocks
             ("sd3", tiny_sd3()),                                              # learned positional crop, conv patchify, text stream skipped in the last block
             ("sd35", replace(tiny_sd3(depth=3, heads=6), use_qk_norm=True))]  # QK-norm without RoPE


@pytest.mark.parametrize("name,cfg", TINY_BF16, ids=[n for n, _ in TINY_BF16])
def test_mmdit_tiny_contents_and_bounds(dev, packed_for, name, cfg):
    from tests.test_gpu_model import yardstick_ok
    shape, big = (2, 8, 12, 20), (3, 16, 16, 32)
    named, packed = packed_for(cfg)
    outs = mmdit_contents_case(dev, cfg, packed, shape, big, TS, f"mmdit tiny {name}")
    res = _oracle_finals(cfg, {k: v.float() for k, v in named.items()}, _cpu_inputs(cfg, *shape), TS, 1, {"fp32": (Prec(), {}), "emu": (Prec(BF), {})})
    got = outs["nan"][1].float()
    yardstick_ok(got, res["emu"], res["fp32"], f"{name}, from the 0xFF workspace")  # tests/test_gpu_model.py::test_mmdit_forward_tiny's gate
    assert psnr(res["fp32"], got) > 35.0


def test_mmdit_tiny_f16_contents_and_bounds(dev, packed_for):
    from oracle.mmdit import embed_dtype
    from tests.test_gpu_f16_model import gate
    base = tiny_sd3()
    cfg = float16_config(base)
    shape, big = (2, 8, 12, 20), (3, 16, 16, 32)
    named, packed = packed_for(cfg)
    outs = mmdit_contents_case(dev, cfg, packed, shape, big, TS, "mmdit tiny sd3 float16")
    assert outs["nan"][1].dtype == F16
    wf = {k: v.to(F16).float() for k, v in named.items()}
    res = _oracle_finals(base, wf, _cpu_inputs(base, *shape), TS, 1, {"fp32": (Prec(), dict(embed_prec=Prec(embed_dtype(base)))), "emu16": (Prec(F16), {}),
                                                                       "emubf": (Prec(BF), {})})
    gate(outs["nan"][1].float(), res["emu16"], res["emubf"], res["fp32"], "tiny sd3 float16, from the 0xFF workspace")  # test_mmdit_forward_tiny_f16's gate


_T22 = tiny_flux(depth_multimodal=2, depth_unified=2, heads=2)
FP8_POLICY = replace(_T22, weight_dtype="fp8_e4m3", fp8_bf16_double_blocks=1)  # (the bf16 HID of block 0 coexists with the fp8 buffers)


# (B, latent, S_t) of tests/test_gpu_fp8_ragged.py's COMPOSE_CASES: 256 aligned image rows; 2 x 360 = 720 image rows, pad rows up to 768 in front
# of the text rows
@pytest.mark.parametrize("B,Hl,Wl,S_t,big", [(1, 32, 32, 128, (2, 32, 32, 128)), (2, 40, 36, 128, (2, 48, 40, 256))], ids=["aligned", "ragged"])
def test_mmdit_tiny_fp8_contents_and_bounds(dev, packed_for, B, Hl, Wl, S_t, big):
    from oracle import fp8 as o8
    from tests.test_gpu_fp8_ragged import COMPOSE_CASES
    cfg = FP8_POLICY
    assert (cfg, B, Hl, Wl, S_t) in COMPOSE_CASES
    named, packed = packed_for(cfg)
    outs = mmdit_contents_case(dev, cfg, packed, (B, Hl, Wl, S_t), big, TS, f"mmdit tiny fp8 B={B} {Hl}x{Wl}")
    fq, plain, paq = o8.fake_quant_block_weights(cfg, named), {k: v.float() for k, v in named.items()}, o8.policy_act_quant(cfg)
    inp = _cpu_inputs(cfg, B, Hl, Wl, S_t)
    res = _oracle_finals(cfg, fq, inp, TS, 1, {"fq_emu": (Prec(BF), dict(act_quant=paq)), "fq_fp32": (Prec(), dict(act_quant=paq))})
    res["fp32"] = _oracle_finals(cfg, plain, inp, TS, 1, {"fp32": (Prec(), {})})["fp32"]
    out = outs["nan"][1].float().cpu()
    # the gates of tests/test_gpu_fp8_ragged.py::_engine_gates (= test_gpu_fp8.py::test_mmdit_fp8_tiny)
    e_h, e_e = rel_l2(res["fq_fp32"], out), rel_l2(res["fq_fp32"], res["fq_emu"])
    p_fq, p_un, p_emu = psnr(res["fq_fp32"], out), psnr(res["fp32"], out), psnr(res["fp32"], res["fq_emu"])
    print(f"[workspace fp8 B={B}] from the 0xFF workspace: hip-vs-fq {e_h:.3e}, emu-vs-fq {e_e:.3e}; PSNR vs fake-quant {p_fq:.1f} dB, vs un-quantised {p_un:.1f} dB "
          f"(emulation {p_emu:.1f} dB)")
    assert e_h <= 2.0 * e_e + 2e-3, (e_h, e_e)
    assert p_fq > 35.0
    assert p_un > p_emu - 3.0


def test_mmdit_tiny_guidance_contents_and_bounds(dev, packed_for):
    """FLUX.1-dev's guidance embedding (gemb / g1 / gvec scratch rows), as tests/test_gpu_fp8.py::test_guidance_embedding builds it: B = 1, two timesteps"""
    from tests.test_gpu_model import yardstick_ok
    cfg = replace(tiny_flux(), guidance_embed=True)
    ts, shape = [1000.0, 752.0], (1, 8, 12, 20)
    named, packed = packed_for(cfg)
    outs = mmdit_contents_case(dev, cfg, packed, shape, (2, 16, 16, 32), ts, "mmdit tiny guidance")
    res = _oracle_finals(cfg, {k: v.float() for k, v in named.items()}, _cpu_inputs(cfg, *shape), ts, 1, {"fp32": (Prec(), {}), "emu": (Prec(BF), {})}, guidance=3.5)
    yardstick_ok(outs["nan"][1].float(), res["emu"], res["fp32"], "guidance 3.5, from the 0xFF workspace")


# ---- 2a. MMDiT at production width (depth 1 + 1): the 256-row GEMMs, their K split, attention5 and its key-split region exist only here ----------
# No oracle: the zero-fill run is what the width tests of tests/test_gpu_model.py, test_gpu_fp8.py and test_gpu_f16_model.py already gate.
TS2 = [1000.0, 752.0]
FLUX_W = replace(FLUX_SCHNELL, depth_multimodal=1, depth_unified=1)
SD3_W = replace(SD3_2b, depth_multimodal=2, hidden_size_override=1536)


def test_flux_width_ragged_rows(dev, packed_for):
    """B = 2, latent 104 x 104: S_i = 2704 is ragged against every tile height; S = 2960 is no multiple of 256, so the phase-alternating attention
    kernel (attention4.hip) runs"""
    _, packed = packed_for(FLUX_W)
    mmdit_contents_case(dev, FLUX_W, packed, (2, 104, 104, 256), (2, 112, 112, 256), TS2, "flux width 104 x 104")


def test_flux_width_k_split_flags(dev, packed_for):
    """B = 1, latent 64 x 64 (512 x 512 pixels): fc2 (1024 image + 256 text rows, K = 12288) and linear2 (1280 rows, K = 15360) are 60 tiles cut
    along K.  The plan is recorded before the forward, so the case cannot pass vacuously; after every run the flag region of the engine's
    K-split workspace (dk_mmdit_debug_buffer(2)), error word included, is zero."""
    from tests.test_dispatch_plan import plan
    _, packed = packed_for(FLUX_W)
    h = FLUX_W.hidden_size
    seen = []

    def before_forward(eng):
        lib = eng.lib
        for what, p in (("fc2", plan(1024, h, 4 * h, M2=256, lda=lib.dk_weight_pitch(4 * h), ldw=lib.dk_weight_pitch(4 * h))),
                        ("linear2", plan(1280, h, 5 * h, lda=lib.dk_weight_pitch(5 * h), ldw=lib.dk_weight_pitch(5 * h)))):
            print(f"[workspace k-split] {what}: kernel {p.kernel}, {p.tiles} tiles, {p.split_tiles} cut into {p.k_pieces} K ranges, {p.workgroups} workgroups")
            assert p.split_tiles > 0 and p.k_pieces >= 2, f"{what} is not cut along K at this shape: the case would prove nothing"
        seen.append("plan")

    def after_run(eng, interior, label):
        ptr = eng.lib.dk_mmdit_debug_buffer(eng._h, 2)
        n, off = eng.lib.dk_gemm_workspace_bytes(), ptr - interior.data_ptr()
        assert ptr and 0 <= off and off + n <= interior.numel(), f"the K-split workspace [{off}, {off + n}) lies outside the lent workspace"
        flags = interior[off + n - 4096:off + n]  # the flag region: the last 4096 bytes (word 512: the error word)
        assert int(flags.view(torch.int32)[512]) == 0, f"[{label}] a finisher gave up waiting for its producers (error word set)"
        bad = torch.nonzero(flags)
        assert bad.numel() == 0, f"[{label}] the K-split flag region is not zero after the forward, first byte {int(bad[0]) if bad.numel() else -1}"
        seen.append(label)

    mmdit_contents_case(dev, FLUX_W, packed, (1, 64, 64, 256), (1, 72, 72, 256), TS2, "flux width 64 x 64 (K split)", after_run, before_forward)
    assert seen.count("plan") == 3 and [s for s in seen if s != "plan"] == ["zero", "nan", "stale"]


def test_flux_width_attention5(dev, packed_for):
    """B = 1, latent 128 x 128, two steps: S = 4352 = 17 x 256 selects attention5.hip (D = 128, S >= 2048, S % 256 == 0), under the engine's own
    attention workspace.  408 query blocks leave a last round of 152 on 256 compute units, which no key split shortens: the launch is whole here;
    the key-split partials are the next test's."""
    _, packed = packed_for(FLUX_W)
    mmdit_contents_case(dev, FLUX_W, packed, (1, 128, 128, 256), (1, 136, 136, 256), TS2, "flux width 128 x 128 (attention5)")


def test_flux_width_attention5_key_split(dev, packed_for):
    """B = 2, latent 64 x 96: S = 1792 = 7 x 256, 336 query blocks = one round + 80, and the 80 are cut into two key ranges (160 workgroups) whose
    partial O / l / exponent rows go through the engine's AWS region and dk_attn5_merge_kernel.  That the split engages: with
    dk_tune_set("attn_split", 0) the summation order, hence some bits, change."""
    from diffusionkit_amd import ops
    from diffusionkit_amd.engine import MMDiTEngine
    _, packed = packed_for(FLUX_W)
    shape = (2, 64, 96, 256)
    outs = mmdit_contents_case(dev, FLUX_W, packed, shape, (2, 72, 104, 256), TS2, "flux width 64 x 96 (attention5 key split)")
    try:
        ops.tune("attn_split", 0)
        whole = mmdit_sequence(MMDiTEngine(FLUX_W, packed), shape, mmdit_inputs(FLUX_W, dev, *shape), TS2)
    finally:
        ops.tune("attn_split", -1)
    assert bool(torch.isfinite(whole[1].float()).all())
    assert not torch.equal(whole[1], outs["zero"][1]), "the key split did not engage at this shape: the case does not reach the AWS region"
    assert rel_l2(whole[1].float(), outs["zero"][1].float()) < 4e-3  # (tests/test_gpu_model.py::test_attention_kernels_agree_inside_the_model's bound)


def test_flux_width_interleaved_workspaces(dev, packed_for):
    """Two engines of one width on one host thread and stream, forwards alternating: engine 1 at B = 2, latent 64 x 96 (attention5's key split goes
    through ITS attention region: test_flux_width_attention5_key_split), engine 2 at B = 1, latent 64 x 64 (fc2 / linear2 are cut along K through ITS
    K-split region: test_flux_width_k_split_flags).  Each launch gets its regions as arguments from the engine that builds it, so every output
    equals that engine's solo sequence, the idle engine's whole workspace is byte for byte the same before and after the other one's call, and both
    pairs of margins are intact."""
    from diffusionkit_amd.engine import MMDiTEngine
    _, packed = packed_for(FLUX_W)
    shapes = [(2, 64, 96, 256), (1, 64, 64, 256)]
    inps = [mmdit_inputs(FLUX_W, dev, *s, seed0=50 * i) for i, s in enumerate(shapes)]
    solo = [mmdit_sequence(MMDiTEngine(FLUX_W, packed), s, inp, TS2) for s, inp in zip(shapes, inps)]
    engs = [MMDiTEngine(FLUX_W, packed) for _ in shapes]
    nbytes = [e.lib.dk_mmdit_workspace_bytes(e._h, *s, len(TS2)) for e, s in zip(engs, shapes)]
    wss = [es.GuardedWorkspace(n, dev) for n in nbytes]
    for e, ws, n in zip(engs, wss, nbytes):
        ws.fill(es.FILL_NAN)
        es.lend(e, ws, n)
    steps = [mmdit_prepared_steps(e, s, inp, TS2) for e, s, inp in zip(engs, shapes, inps)]
    torch.cuda.synchronize()
    got = [[], []]
    for k in range(len(steps[0])):
        for a, idle in ((0, 1), (1, 0)):
            before = wss[idle].interior(nbytes[idle]).clone()
            got[a].append(steps[a][k]())
            torch.cuda.synchronize()
            d = wss[idle].interior(nbytes[idle]) != before
            assert not bool(d.any()), (f"call {k} of engine {a + 1} changed the idle engine {idle + 1}'s workspace, first at byte "
                                       f"{int(torch.nonzero(d)[0])} of {nbytes[idle]}")
    for i, (e, ws, n) in enumerate(zip(engs, wss, nbytes)):
        assert e._ws.data_ptr() == ws.interior(n).data_ptr() and e._ws.numel() == n
        ws.check(n, f"interleaved flux width, engine {i + 1} {shapes[i]}", fill=es.FILL_NAN)
        es.assert_identical({"solo": solo[i], "interleaved": tuple(got[i])}, f"interleaved flux width, engine {i + 1} {shapes[i]}")


def test_flux_width_fp8_ragged_rows(dev, packed_for):
    """the fp8 configuration at width, B = 2, latent 104 x 104: 5408 image rows, pad rows up to 5504 in front of the text rows of XN8 / ATT8 / HC8"""
    cfg = replace(FLUX_W, weight_dtype="fp8_e4m3")
    _, packed = packed_for(cfg)
    mmdit_contents_case(dev, cfg, packed, (2, 104, 104, 256), (2, 112, 112, 256), TS2, "flux width fp8 104 x 104")


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "float16"])
def test_sd3_width_contents_and_bounds(dev, packed_for, f16):
    """SD3-medium width (h = 1536, D = 64): B = 2, latent 64 x 64, S_t = 154"""
    cfg = float16_config(SD3_W) if f16 else SD3_W
    _, packed = packed_for(cfg)
    mmdit_contents_case(dev, cfg, packed, (2, 64, 64, 154), (2, 72, 72, 154), TS2, f"sd3 width {'float16' if f16 else 'bf16'}")


# ---- 2a. VAE ---------------------------------------------------------------------------------------------------------------------------------
def vae_contents_case(dev, make_engine, nbytes_of, call, x, x_big, what):
    """``make_engine()`` -> a fresh wrapper; ``nbytes_of(eng, x)`` -> the engine's own workspace size for input x; ``call(eng, x)`` -> tuple of outputs"""
    probe = make_engine()
    nbytes, nbig = nbytes_of(probe, x), nbytes_of(probe, x_big)
    assert nbig > nbytes, (nbig, nbytes)
    ws = es.GuardedWorkspace(nbig, dev)
    x, x_big = x.to(dev), x_big.to(dev)
    outs = {}

    def run(eng, label, fill):
        es.lend(eng, ws, nbytes)
        outs[label] = call(eng, x)
        torch.cuda.synchronize()
        assert eng._ws.data_ptr() == ws.interior(nbytes).data_ptr() and eng._ws.numel() == nbytes
        ws.check(nbytes, f"{what} [{label}]", fill=fill)

    for label, fill in FILLS:
        ws.fill(fill)
        run(make_engine(), label, fill)
    eng = make_engine()
    es.lend(eng, ws, nbig)
    call(eng, x_big)
    torch.cuda.synchronize()
    ws.check(nbig, f"{what} [the larger run in front of the stale one]", fill=es.FILL_NAN)
    run(eng, "stale", None)
    es.assert_identical(outs, what)
    return outs


def _decoder(dev, prod, f16):
    from diffusionkit_amd.engine import VAEDecoderEngine
    vcfg = VAEDecoderConfig() if prod else tiny_vae()
    named = synth_vae_weights(vcfg, seed=4321)
    c = float16_vae_config(vcfg) if f16 else vcfg
    w = pack_vae(c, named, dev)
    return vcfg, named, (lambda: VAEDecoderEngine(c, w))


def _decode(eng, z):
    return eng.decode(z, want_raw=True)  # (img f32, u8, raw)


def _decoder_bytes(eng, z):
    return eng.lib.dk_vae_workspace_bytes(eng._h, z.shape[0], z.shape[1], z.shape[2])


def _latent(B, h, w, seed=11):
    return torch.randn(B, h, w, 16, generator=torch.Generator().manual_seed(seed))


# tiny_vae(), latent 6 x 10: T = 60 tokens, Tp = 64 -- the score-matrix path with its [T, Tp) pad columns and V^T pad rows; 8 x 8: T = Tp = 64
@pytest.mark.parametrize("hw,big", [((6, 10), (8, 12)), ((8, 8), (8, 12))], ids=["6x10", "8x8"])
@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "float16"])
def test_vae_decoder_tiny_contents_and_bounds(dev, f16, hw, big):
    vcfg, named, make = _decoder(dev, False, f16)
    z = _latent(2, *hw)
    outs = vae_contents_case(dev, make, _decoder_bytes, _decode, z, _latent(2, *big, seed=12), f"vae decoder tiny {hw} {'float16' if f16 else 'bf16'}")
    img, u8, raw = outs["nan"]
    if f16:
        from tests.test_gpu_vae_f16 import PRECS, f16r, gate  # tests/test_gpu_vae_f16.py::decode_case's raw gate
        wf = {k: v.to(F16).float() for k, v in named.items()}
        res = {n: OracleVAEDecoder(vcfg, wf, P)(f16r(z)) for n, P in PRECS}
        gate(raw[..., :3].float(), res["emu16"], res["emubf"], res["fp32"], f"decoder tiny {hw} raw, from the 0xFF workspace")
    else:
        from tests.test_gpu_model import yardstick_ok  # tests/test_gpu_model.py::test_vae_decode_tiny's gates
        wf = {k: v.float() for k, v in named.items()}
        res = {n: OracleVAEDecoder(vcfg, wf, P)(bf16r(z)) for n, P in (("fp32", Prec()), ("emu", Prec(BF)))}
        yardstick_ok(raw[..., :3].float(), res["emu"], res["fp32"], f"vae raw {hw}, from the 0xFF workspace")
        assert psnr(torch.clip(res["fp32"] / 2 + 0.5, 0, 1), img) > 35.0


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "float16"])
def test_vae_decoder_production_contents_and_bounds(dev, f16):
    """production channel plan, B = 2, latent 10 x 14: the C = 512 flash attention at T = 140 (V^T padded to Tp = 192 rows), conv tiles ragged against
    every stage (80 x 112 pixels)"""
    _, _, make = _decoder(dev, True, f16)
    vae_contents_case(dev, make, _decoder_bytes, _decode, _latent(2, 10, 14, seed=13), _latent(2, 12, 16, seed=14),
                      f"vae decoder production 10 x 14 {'float16' if f16 else 'bf16'}")


def _encoder(dev, prod, f16):
    from diffusionkit_amd.engine import VAEEncoderEngine
    cfg = VAEEncoderConfig() if prod else tiny_vae_encoder()
    named = synth_vae_encoder_weights(cfg, seed=99 if prod else 8765)
    c = float16_vae_config(cfg) if f16 else cfg
    w = pack_vae(c, named, dev)
    return cfg, named, (lambda: VAEEncoderEngine(c, w))


def _encode(eng, image):
    return (eng.encode(image),)  # the moments


def _encoder_bytes(eng, image):
    return eng.lib.dk_vae_encoder_workspace_bytes(eng._h, image.shape[0], image.shape[1], image.shape[2])


def _image(B, H, W, seed=0):
    """an image in [-1, 1] as oracle.pipeline.read_image_array makes it (which takes the pipeline's multiples of 64 only; the engine takes multiples of 8)"""
    from tests.test_gpu_model import _test_image
    img = torch.from_numpy((_test_image(H, W, seed=seed).astype(np.float32) / 255) * 2 - 1.0)[None]
    if H % 64 == 0 and W % 64 == 0:
        assert torch.equal(img, op.read_image_array(_test_image(H, W, seed=seed)))
    return torch.cat([img, -img], 0) if B == 2 else img


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "float16"])
def test_vae_encoder_tiny_contents_and_bounds(dev, f16):
    cfg, named, make = _encoder(dev, False, f16)
    img = _image(2, 64, 64)
    outs = vae_contents_case(dev, make, _encoder_bytes, _encode, img, _image(2, 128, 64, seed=1), f"vae encoder tiny 64 x 64 {'float16' if f16 else 'bf16'}")
    hid = outs["nan"][0][..., :cfg.out_channels].float()
    if f16:
        from tests.test_gpu_vae_f16 import PRECS, gate  # tests/test_gpu_vae_f16.py::encode_case's gate
        wf = {k: v.to(F16).float() for k, v in named.items()}
        res = {n: OracleVAEEncoder(cfg, wf, P)(img) for n, P in PRECS}
        gate(hid, res["emu16"], res["emubf"], res["fp32"], "encoder tiny moments, from the 0xFF workspace")
    else:
        from tests.test_gpu_model import yardstick_ok  # tests/test_gpu_model.py::test_vae_encode_tiny's gate
        wf = {k: v.float() for k, v in named.items()}
        res = {n: OracleVAEEncoder(cfg, wf, P)(img) for n, P in (("fp32", Prec()), ("emu", Prec(BF)))}
        yardstick_ok(hid, res["emu"], res["fp32"], "vae encoder moments, from the 0xFF workspace")


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "float16"])
def test_vae_encoder_production_contents_and_bounds(dev, f16):
    """production plan, image 80 x 112: 10 x 14 = 140 tokens in the mid block, stride-2 stages ragged against the 16 x 16 tiles"""
    _, _, make = _encoder(dev, True, f16)
    vae_contents_case(dev, make, _encoder_bytes, _encode, _image(1, 80, 112, seed=3), _image(1, 96, 128, seed=4),
                      f"vae encoder production 80 x 112 {'float16' if f16 else 'bf16'}")


# ---- interleaved element types: bf16 and float16 engines and stand-alone operators in turn on one host thread and stream ---------------------------
def test_interleaved_element_types_one_thread(dev, packed_for):
    """A bf16 and a float16 tiny SD3 engine and the tiny VAE decoder in both element types, stepped round-robin; between two engine steps one
    stand-alone float16 ops.linear and one bf16 ops.attention.  The element type of a launch is an argument of whatever builds it: every engine
    output equals the same engine's solo run, every stand-alone result the same call made before any of these engines existed.
    The attention (D = 128, S = 2048, 96 query blocks on 256 compute units) is cut into two key ranges through the host thread's own attention
    workspace, which no engine call consults or moves."""
    from diffusionkit_amd import ops
    from diffusionkit_amd.engine import MMDiTEngine
    x, w, b = randn(154, 256, seed=60).to(dev, F16), randn(384, 256, seed=61, scale=0.08).to(dev, F16), randn(384, seed=62, scale=0.1).to(dev, F16)
    qkv = randn(1, 2048, 3 * 12 * 128, seed=63).to(dev, BF)
    standalone = lambda: (ops.linear(x, w, b), ops.attention(qkv, 12, 128))
    alone = standalone()
    try:
        ops.tune("attn_split", 0)
        whole = ops.attention(qkv, 12, 128)
    finally:
        ops.tune("attn_split", -1)
    assert not torch.equal(whole, alone[1]), "the key split did not engage: the stand-alone attention does not reach the thread's workspace"

    shape, z = (2, 8, 12, 20), _latent(2, 6, 10).to(dev)
    cfgs = [tiny_sd3(), float16_config(tiny_sd3())]
    mm = [(cfg, packed_for(cfg)[1], mmdit_inputs(cfg, dev, *shape)) for cfg in cfgs]
    makes = [_decoder(dev, False, f16)[2] for f16 in (False, True)]
    solo = [mmdit_sequence(MMDiTEngine(cfg, packed), shape, inp, TS) for cfg, packed, inp in mm] + [_decode(make(), z) for make in makes]
    torch.cuda.synchronize()

    steps = [mmdit_prepared_steps(MMDiTEngine(cfg, packed), shape, inp, TS) for cfg, packed, inp in mm]
    decoders = [make() for make in makes]
    got, between = [[], [], [], []], []
    for r in range(len(TS) + 1):
        for j in range(4):
            got[j].append(steps[j][r]() if j < 2 else _decode(decoders[j - 2], z))
            between.append(standalone())
    torch.cuda.synchronize()
    for j, name in enumerate(("tiny sd3 bf16", "tiny sd3 float16")):
        assert got[j][0].dtype == dtype_of(cfgs[j])
        es.assert_identical({"solo": solo[j], "interleaved": tuple(got[j])}, f"interleaved element types, {name}")
    for j, name in ((2, "vae decoder bf16"), (3, "vae decoder float16")):
        for r, out in enumerate(got[j]):
            es.assert_identical({"solo": solo[j], "interleaved": out}, f"interleaved element types, {name}, round {r + 1}")
    for i, out in enumerate(between):
        es.assert_identical({"no engine alive": alone, "between engine steps": out}, f"stand-alone linear / attention behind engine step {i + 1}")


# ---- 2b. reuse: one object through a sequence of problems against fresh objects -----------------------------------------------------------------
def _problem_inputs(cfg, dev, B, Hl, Wl, S_t):
    """seeded by the problem, so that a problem that comes back gets the inputs it had"""
    return mmdit_inputs(cfg, dev, B, Hl, Wl, S_t, seed0=1000 * B + 10 * Hl + Wl)


def _drive(eng, prob, inp, cached_ctx, expect_refusal):
    """one stop: prepare, modulation cache, every step's output (through cache_context + text=None where ``cached_ctx``).  ``expect_refusal``: a context
    cached for an EARLIER problem must not survive this prepare"""
    B, Hl, Wl, S_t, n = prob
    eng.prepare(B, (Hl, Wl), S_t, n)
    eng.cache_modulation_params(inp["pooled"], TS[:n])
    tok = eng.patchify(inp["lat"])
    if expect_refusal:
        with pytest.raises(Exception, match="cache_context"):
            eng.forward_tokens(tok, None, 0)
    if cached_ctx:
        eng.cache_context(inp["text"])
    outs = tuple(eng.forward_tokens(tok, None if cached_ctx else inp["text"], i) for i in range(n))
    torch.cuda.synchronize()
    return outs


REUSE_STOPS = [(2, 8, 12, 20, 3), (1, 16, 16, 32, 2), (2, 8, 12, 20, 3), (2, 8, 8, 20, 3), (3, 8, 12, 20, 1)]
REUSE_CFGS = [("flux", tiny_flux(), {}), ("sd3", tiny_sd3(), {}), ("fp8", FP8_POLICY, {20: 128, 32: 256})]  # (fp8: text lengths are multiples of 128)


@pytest.mark.parametrize("name,cfg,st_map", REUSE_CFGS, ids=[n for n, _, _ in REUSE_CFGS])
def test_mmdit_reuse_equals_fresh_engines(dev, packed_for, name, cfg, st_map):
    from diffusionkit_amd.engine import MMDiTEngine
    _, packed = packed_for(cfg)
    reused = MMDiTEngine(cfg, packed)
    seen = []
    for i, (B, Hl, Wl, S_t, n) in enumerate(REUSE_STOPS):
        prob = (B, Hl, Wl, st_map.get(S_t, S_t), n)
        inp = _problem_inputs(cfg, dev, *prob[:4])
        ctx = i % 2 == 1  # cache_context on every second stop
        got = _drive(reused, prob, inp, ctx, expect_refusal=i > 0 and (i - 1) % 2 == 1)
        want = _drive(MMDiTEngine(cfg, packed), prob, inp, ctx, expect_refusal=False)
        es.assert_identical({"fresh engine": want, "reused engine": got}, f"{name} stop {i + 1} {prob}")
        seen.append(got)
    es.assert_identical({"first visit": seen[0], "the same problem again": seen[2]}, f"{name}: stop 3 repeats stop 1")


def test_mmdit_reuse_guidance_change(dev, packed_for):
    """eng.guidance changed between two stops of the SAME shape (prepare returns early; the modulation cache must still be rebuilt from the new value)"""
    from diffusionkit_amd.engine import MMDiTEngine
    cfg = replace(tiny_flux(), guidance_embed=True)
    _, packed = packed_for(cfg)
    prob = (2, 8, 12, 20, 3)
    inp = _problem_inputs(cfg, dev, *prob[:4])
    reused, outs = MMDiTEngine(cfg, packed), {}
    for g in (3.5, 1.0):
        reused.guidance = g
        outs[g] = _drive(reused, prob, inp, False, False)
        fresh = MMDiTEngine(cfg, packed)
        fresh.guidance = g
        es.assert_identical({"fresh engine": _drive(fresh, prob, inp, False, False), "reused engine": outs[g]}, f"guidance {g}")
    assert not any(torch.equal(a, b) for a, b in zip(outs[3.5], outs[1.0])), "the new guidance value did not reach the modulation table"


VAE_REUSE_LATENTS = [(16, 8), (8, 8), (6, 10), (16, 8)]


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "float16"])
def test_vae_decoder_reuse_equals_fresh_engines(dev, f16):
    _, _, make = _decoder(dev, False, f16)
    reused = make()
    for B in (2, 1):
        for i, hw in enumerate(VAE_REUSE_LATENTS):
            z = _latent(B, *hw, seed=20 + hw[0] + hw[1]).to(dev)
            got, want = _decode(reused, z), _decode(make(), z)
            torch.cuda.synchronize()
            es.assert_identical({"fresh engine": want, "reused engine": got}, f"vae decoder B={B} stop {i + 1} latent {hw}")


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "float16"])
def test_vae_encoder_reuse_equals_fresh_engines(dev, f16):
    _, _, make = _encoder(dev, False, f16)
    reused = make()
    for B in (2, 1):
        for i, hw in enumerate(VAE_REUSE_LATENTS):
            img = _image(B, 8 * hw[0], 8 * hw[1], seed=hw[0] + hw[1]).to(dev)
            got, want = _encode(reused, img), _encode(make(), img)
            torch.cuda.synchronize()
            es.assert_identical({"fresh engine": want, "reused engine": got}, f"vae encoder B={B} stop {i + 1} image {(8 * hw[0], 8 * hw[1])}")


@pytest.mark.parametrize("family", ["flux", "sd3_cfg"])
def test_pipeline_reuse_equals_fresh_pipelines(dev, family):
    """denoise_latents at 8 x 12, 8 x 8, 8 x 12 with one seed on one pipeline object: stops 1 and 3 are bit-identical and every stop equals a fresh pipeline's"""
    from diffusionkit_amd.pipeline import DiffusionPipeline, FluxPipeline
    if family == "flux":
        cfg, cfgw, rows = tiny_flux(), 0.0, 1
        make = lambda: FluxPipeline(w16=True, a16=True, mmdit_config=cfg, vae_config=tiny_vae(), device=dev, text_len=16)
    else:
        cfg, cfgw, rows = tiny_sd3(), 5.0, 2
        make = lambda: DiffusionPipeline(w16=True, a16=True, shift=3.0, mmdit_config=cfg, vae_config=tiny_vae(), device=dev, text_len=16)
    text = randn(rows, 16, cfg.token_level_text_embed_dim, seed=7).to(dev, BF)
    pooled = randn(rows, cfg.pooled_text_embed_dim, seed=8).to(dev, BF)
    run = lambda pipe, size: pipe.denoise_latents(text, pooled, num_steps=3, cfg_weight=cfgw, latent_size=size, seed=0)[0].clone()
    reused, got = make(), []
    for i, size in enumerate([(8, 12), (8, 8), (8, 12)]):
        got.append(run(reused, size))
        es.assert_identical({"fresh pipeline": run(make(), size), "reused pipeline": got[-1]}, f"{family} pipeline stop {i + 1} latent {size}")
    es.assert_identical({"first visit": got[0], "the same size again": got[2]}, f"{family} pipeline: stop 3 repeats stop 1")
    assert got[0].shape == (1, 8, 12, 16) and got[1].shape == (1, 8, 8, 16)
