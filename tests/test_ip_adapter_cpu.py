"""FLUX IP-Adapter without a GPU: the oracle (scale 0 is the pinned oracle; every double block's adapter moves the output by ten times the GPU
gate), the operator gate proved on the restatement's mutants, the XLabs loader, configuration and packing, the C ABI's refusals on a host-only
handle, the command line, the pipeline's refusals and sharding.

The operator gate and the mutant "output rounded twice": the gate grants twice the restatement's error plus one bf16 unit, and a second
rounding to the same format adds at most the first one's error, so wherever the restatement itself carries a rounding error the mutant hides under
it -- 0.56 .. 0.66 of the bound on the four general cases (h 256 N 4: 0.56, N 7: 0.66; h 3072 N 4: 0.63; N 16: 0.63), printed by the test, not
rejected there and not claimed.  It is proved where it can show: on ``equal_values_case`` (every key of an image carries the same value row, so the
definition's output is that bf16 row exactly and the restatement's error is zero) the gate's bound is the one bf16 unit alone, and the mutant misses
it by 5.2 x .. 6.0 x.  The GPU file runs the kernel on the same case.  The five other mutants miss the gate by 170 x and more on the general cases
(on the equal-values case the four that only move the weights cannot show: the weights cancel)."""
import ctypes
from dataclasses import replace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from diffusionkit_amd import cli
from diffusionkit_amd.config import (FLUX_IP_ADAPTER, MMDIT_CKPT, IPAdapterConfig, fp8_config, tiny_flux, tiny_flux_controlnet, tiny_ip_adapter,
                                     tiny_sd3, validate_ip_adapter)
from diffusionkit_amd.model_io import CheckpointError, flux_ip_adapter_checkpoint_to_reference, load_ip_adapter_checkpoint
from diffusionkit_amd.pipeline import _check_ip_adapter_config, _ip_adapter_options
from diffusionkit_amd.weights import ip_adapter_weight_shapes, pack_ip_adapter, synth_ip_adapter_weights, synth_mmdit_weights
from oracle.mmdit import OracleMMDiT, Prec
from tests import _ip_adapter as IP
from tests._ip_adapter import IP_SCALE, IPAdapterFluxOracle, synthetic_embeds, to_xlabs_ip_adapter
from tests._util import BF, randn, rel_l2
from tests.test_mmditx_cpu import last_error, make_handle

GATE_ABS = 2e-3  # the absolute term of tests/test_gpu_model.py's yardstick_ok
IPC = tiny_ip_adapter()
B, HL, WL, S_T, TS = 2, 8, 12, 20, [1000.0, 752.0, 500.0]


# ---- the oracle -------------------------------------------------------------------------------------------------------------------------
def _inputs(cfg):
    return randn(B, S_T, cfg.token_level_text_embed_dim, seed=3), randn(B, cfg.pooled_text_embed_dim, seed=4), randn(B, HL, WL, 16, seed=5)


def _final(m, cfg, ip, off=()):
    text, pooled, lat = _inputs(cfg)
    m.ip, m.ip_off = ip, off
    m.cache_modulation_params(pooled, torch.tensor(TS))
    streams = {}
    m(lat, text, TS[1], taps=streams)
    return streams["final"]


def test_every_site_moves_the_oracle_by_ten_times_the_gate():
    """tiny_flux(3, 2), N = 4: zeroing the adapter of any ONE double block moves the fp32 oracle's final output by >= 10 x the GPU gate,
    2 err(emu) + 2e-3, so an engine that misses one add site -- block 1's and block 2's LayerNorm launch, single block 0's -- cannot pass
    tests/test_gpu_ip_adapter.py.  With scale 0, and without the adapter, the subclass returns the pinned oracle's values exactly."""
    cfg = tiny_flux(3, 2)
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    wa = {k: v.float() for k, v in synth_ip_adapter_weights(cfg, IPC, seed=2468).items()}
    ip = (wa, IPC, synthetic_embeds(B, IPC.embed_dim), IP_SCALE)
    m = IPAdapterFluxOracle(cfg, wf, Prec())
    full = _final(m, cfg, ip)
    gate = 2 * rel_l2(full, _final(IPAdapterFluxOracle(cfg, wf, Prec(BF)), cfg, ip)) + GATE_ABS
    for i in range(cfg.depth_multimodal):
        moved = rel_l2(full, _final(m, cfg, ip, off=(i,)))
        print(f"double block {i}: zeroing its adapter moves the output by {moved:.3e} (10 x gate {10 * gate:.3e})")
        assert moved >= 10 * gate, f"double block {i}: zeroing its adapter moves the output by {moved:.3e} only"
    text, pooled, lat = _inputs(cfg)
    base = OracleMMDiT(cfg, wf, Prec())
    base.cache_modulation_params(pooled, torch.tensor(TS))
    streams = {}
    base(lat, text, TS[1], taps=streams)
    assert torch.equal(_final(m, cfg, None), streams["final"]) and torch.equal(_final(m, cfg, ip[:3] + (0.0,)), streams["final"])
    assert torch.equal(_final(m, cfg, ip, off=(0, 1, 2)), streams["final"])


def test_oracle_per_image_prompts_and_no_single_blocks():
    """image b sees its own prompt: swapping the two embeddings changes both images; (3, 0): the forward without single blocks takes the adapter too"""
    cfg = tiny_flux(3, 0)
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    wa = {k: v.float() for k, v in synth_ip_adapter_weights(cfg, IPC, seed=2468).items()}
    emb = synthetic_embeds(B, IPC.embed_dim)
    m = IPAdapterFluxOracle(cfg, wf, Prec())
    a, plain = _final(m, cfg, (wa, IPC, emb, IP_SCALE)), _final(m, cfg, None)
    b = _final(m, cfg, (wa, IPC, emb.flip(0), IP_SCALE))
    shared = _final(m, cfg, (wa, IPC, emb[:1], IP_SCALE))
    assert rel_l2(plain, a) > 10 * GATE_ABS and all(rel_l2(a[i], b[i]) > GATE_ABS for i in range(B))
    # (image 0 keeps its prompt -- up to the summation order of a broadcast operand on the host -- and image 1 takes image 0's)
    assert rel_l2(a[0], shared[0]) < 1e-5 and rel_l2(a[1], shared[1]) > GATE_ABS


# ---- the operator gate --------------------------------------------------------------------------------------------------------------------
GATE_CASES = [(256, (2, 3, 5), 4), (256, (2, 8, 70), 7), (3072, (2, 3, 5), 4), (256, (3, 5, 6), 16)]


@pytest.mark.parametrize("mutant", IP.MUTANTS)
def test_operator_gate_rejects(mutant):
    """the fp32 restatement passes its own gate below half the bound (2 e / (2 e + unit) < 1/2 by construction: stated, not discovered); the mutant
    misses it.  "output rounded twice" is proved on the equal-values operands of the same shapes, where a second rounding is not hidden under the
    first (module docstring); its figures on the general cases are printed beside."""
    twice = mutant == "output rounded twice"
    for h, (b, s_t, s_i), n in GATE_CASES:
        operands = (IP.equal_values_case if twice else IP.kernel_case)(h, b, s_t, s_i, n)
        ref, rest, got = (IP.ip_attention_ref(*operands[:1], s_t, *operands[1:], dt, mutant=m)
                          for dt, m in ((torch.float64, None), (torch.float32, None), (torch.float32, mutant)))
        r0, r = IP.operator_ratio(rest, rest, ref), IP.operator_ratio(got, rest, ref)
        line = f"h {h} rows {(b, s_t, s_i)} N {n}: restatement {r0:.3f}, '{mutant}' {r:.2f}"
        if twice:
            qkv, qn, k, v = IP.kernel_case(h, b, s_t, s_i, n)
            ref_g, rest_g = IP.ip_attention_ref(qkv, s_t, qn, k, v), IP.ip_attention_ref(qkv, s_t, qn, k, v, torch.float32)
            general = IP.operator_ratio(IP.ip_attention_ref(qkv, s_t, qn, k, v, torch.float32, mutant=mutant), rest_g, ref_g)
            line += f" on equal values; on the general operands {general:.2f} (hidden under the first rounding: not claimed)"
        print(line)
        assert r0 <= 0.5
        assert not torch.equal(got, rest), f"mutant '{mutant}' left the result bit-identical"
        assert r > 1.0, f"mutant '{mutant}' at {r:.2f} of the bound: the gate does not reject it"


def test_equal_values_case_is_exact():
    """what makes the case a proof: the definition's output is the shared value row, the restatement returns it bit for bit, and its gate ratio is 0"""
    for h, (b, s_t, s_i), n in GATE_CASES:
        qkv, qn, k, v = IP.equal_values_case(h, b, s_t, s_i, n)
        want = v[:, :1].expand(b, s_i, h).reshape(b * s_i, h)
        assert bool((want.abs() >= 1).all()) and bool((want.abs() <= 2).all())
        assert float((IP.ip_attention_ref(qkv, s_t, qn, k, v) - want.double()).abs().max()) < 1e-14
        assert torch.equal(IP.ip_attention_ref(qkv, s_t, qn, k, v, torch.float32), want)


def test_restatement_matches_the_oracle_method():
    """the operator's float64 definition is the oracle's ``ip_attention`` on the same operands (one definition, two spellings)"""
    h, b, s_t, s_i, n = 256, 2, 3, 5, 4
    qkv, qn, k, v = IP.kernel_case(h, b, s_t, s_i, n)
    ref = IP.ip_attention_ref(qkv, s_t, qn, k, v)
    q = qkv[:, s_t:, :h].double().reshape(b, s_i, 2, 128)
    q_n = (q * torch.rsqrt((q * q).mean(-1, keepdim=True) + 1e-6) * qn.double()).transpose(1, 2)
    kk, vv = (t.double().reshape(b, n, 2, 128).transpose(1, 2) for t in (k, v))
    want = (torch.softmax(q_n @ kk.transpose(-1, -2) / 128 ** 0.5, -1) @ vv).transpose(1, 2).reshape(b * s_i, h)
    assert float((ref - want).abs().max()) < 1e-12


# ---- configuration, packing, loader --------------------------------------------------------------------------------------------------------
def test_config_and_packing():
    assert (FLUX_IP_ADAPTER.ip_adapter_tokens, FLUX_IP_ADAPTER.ip_adapter_dim, FLUX_IP_ADAPTER.embed_dim) == (4, 4096, 768)
    cfg = tiny_flux(3, 2)
    validate_ip_adapter(cfg, IPC)
    for bad, msg in ((tiny_sd3(), "FLUX family"), (fp8_config(cfg), "fp8"), (tiny_flux(3, 2, condition_features=64), "condition width"),
                     (tiny_flux_controlnet(2, 1), "ControlNet")):
        with pytest.raises(ValueError, match=msg):
            validate_ip_adapter(bad, IPC)
    for bad in (replace(cfg, activation_dtype="float16"), replace(cfg, use_qk_norm=False), tiny_flux(3, 2, heads=4, head_dim=64)):
        with pytest.raises(ValueError, match="needs bfloat16 activations, head_dim 128 and QK-norm"):
            validate_ip_adapter(bad, IPC)
    for bad in (replace(IPC, ip_adapter_tokens=0), replace(IPC, ip_adapter_tokens=128)):
        with pytest.raises(ValueError, match=r"\[1, 16\]"):
            validate_ip_adapter(cfg, bad)
    with pytest.raises(ValueError, match="multiple of 64"):
        validate_ip_adapter(cfg, replace(IPC, ip_adapter_dim=100))
    w = synth_ip_adapter_weights(cfg, IPC)
    h, C, N, E = cfg.hidden_size, IPC.ip_adapter_dim, IPC.ip_adapter_tokens, IPC.embed_dim
    assert ip_adapter_weight_shapes(cfg, IPC)["ip_adapter.proj.weight"] == (N * C, E) and len(w) == 4 + 4 * 3
    p = pack_ip_adapter(cfg, IPC, w, "cpu")
    kv, kb = p["ip_adapter.kv.weight"], p["ip_adapter.kv.bias"]
    assert tuple(kv.shape) == (3 * 2 * h, C) and tuple(kb.shape) == (3 * 2 * h,)
    for i in range(3):
        for j, leaf in enumerate(("to_k_ip", "to_v_ip")):
            r0 = (2 * i + j) * h
            for t, whole, name in ((p[f"ip_adapter.{i}.{leaf}.weight"], kv, "weight"), (p[f"ip_adapter.{i}.{leaf}.bias"], kb, "bias")):
                assert t.data_ptr() == whole[r0:].data_ptr() and torch.equal(t, w[f"ip_adapter.{i}.{leaf}.{name}"]) and t.is_contiguous()
    nobias = {k: v for k, v in w.items() if not k.endswith("_ip.bias")}
    assert not bool(pack_ip_adapter(cfg, IPC, nobias, "cpu")["ip_adapter.kv.bias"].any())  # (biases are used when present)
    with pytest.raises(ValueError, match="missing"):
        pack_ip_adapter(cfg, IPC, {k: v for k, v in w.items() if k != "ip_adapter.1.to_v_ip.weight"}, "cpu")


def test_loader_round_trip_and_foreign_layouts(tmp_path):
    import os
    from safetensors.torch import save_file
    cfg = tiny_flux(3, 2)
    w = synth_ip_adapter_weights(cfg, IPC)
    sd = to_xlabs_ip_adapter(w, cfg)
    assert "double_blocks.2.processor.ip_adapter_double_stream_v_proj.bias" in sd and "ip_adapter_proj_model.norm.weight" in sd
    path = os.path.join(tmp_path, "ip_adapter.safetensors")
    save_file(sd, path)
    for src in (path, sd, w):
        got = load_ip_adapter_checkpoint(src, cfg, IPC)
        assert set(got) == set(w) and all(torch.equal(got[k], w[k]) for k in w)
    nobias = {k: v for k, v in sd.items() if not k.endswith("_proj.bias") or k.startswith("ip_adapter_proj_model")}
    assert set(flux_ip_adapter_checkpoint_to_reference(nobias, cfg, IPC)) == {k for k in w if not k.endswith("_ip.bias")}
    z = torch.zeros(4, 4, dtype=BF)
    for key, msg in (("single_blocks.0.processor.ip_adapter_single_stream_k_proj.weight", "InstantX"),
                     ("double_blocks.0.processor.ip_adapter_single_stream_k_proj.weight", "InstantX"),
                     ("image_proj.net.0.weight", "MLP / resampler projection"), ("ip_adapter_proj_model.layers.0.weight", "MLP / resampler projection"),
                     ("transformer_blocks.0.attn.processor.to_k_ip.weight", "unknown IP-Adapter checkpoint key"),
                     ("double_blocks.3.processor.ip_adapter_double_stream_k_proj.weight", "3 double blocks")):
        with pytest.raises(CheckpointError, match=msg):
            flux_ip_adapter_checkpoint_to_reference(dict(sd, **{key: z}), cfg, IPC)
    with pytest.raises(CheckpointError, match="lacks 1 tensors"):
        flux_ip_adapter_checkpoint_to_reference({k: v for k, v in sd.items() if k != "ip_adapter_proj_model.norm.bias"}, cfg, IPC)
    with pytest.raises(CheckpointError, match="expected"):
        flux_ip_adapter_checkpoint_to_reference(sd, cfg, replace(IPC, ip_adapter_tokens=8))


# ---- the C ABI on a host-only handle ----------------------------------------------------------------------------------------------------
def test_abi_refusals_without_a_gpu():
    lib, h = make_handle(tiny_flux(3, 2))
    assert lib.dk_abi_version() == 5
    shape = (2, 8, 12, 20, 3)
    plain = lib.dk_mmdit_workspace_bytes(h, *shape)
    setip = lambda n, c, m=h: lib.dk_mmdit_set_ip_adapter(m, n, c)
    for n, c, msg in ((0, 256, "between 1 and 16"), (17, 256, "between 1 and 16"), (4, 100, "multiple of 64"), (4, 0, "multiple of 64")):
        assert setip(n, c) != 0 and msg in last_error(lib)
    assert lib.dk_mmdit_set_ip_scale(h, ctypes.c_float(0.5)) != 0 and "needs an IP-Adapter" in last_error(lib)
    assert lib.dk_mmdit_set_ip_scale(h, ctypes.c_float(0.0)) == 0
    assert lib.dk_mmdit_workspace_bytes(h, *shape) == plain
    assert setip(4, 256) == 0, last_error(lib)
    want = 3 * 2 * 4 * 2 * 256 * 2 + 2 * 24 * 256 * 2  # the K / V cache [depth, B N, 2h] and one ip buffer [B S_i, h]
    assert want <= lib.dk_mmdit_workspace_bytes(h, *shape) - plain < want + 512
    assert lib.dk_mmdit_set_ip_scale(h, ctypes.c_float(float("inf"))) != 0 and "finite" in last_error(lib)
    # beside the adapter: taps, the block cache, a reference grid, a condition width and the forks refuse, each naming it
    taps, one = ctypes.c_void_p(256), (ctypes.c_int32 * 1)(1)
    assert lib.dk_mmdit_set_flux_control_taps(h, taps, 1, 1, ctypes.c_float(0.7)) != 0 and "IP-Adapter" in last_error(lib)
    assert lib.dk_mmdit_set_block_cache(h, 1) != 0 and "IP-Adapter" in last_error(lib)
    assert lib.dk_mmdit_set_reference_grid(h, 8, 8) != 0 and "IP-Adapter" in last_error(lib)
    assert lib.dk_mmdit_set_condition_width(h, 64) != 0 and "IP-Adapter" in last_error(lib)
    lib, h0 = make_handle(tiny_flux(3, 0))  # (the forks are the SD3 family's by depth_unified == 0: a FLUX model without single blocks reaches the rule)
    assert setip(4, 256, h0) == 0, last_error(lib)
    assert lib.dk_mmdit_set_skip_layers(h0, one, 1, 1) != 0 and "IP-Adapter" in last_error(lib)
    assert lib.dk_mmdit_set_perturbed_attention(h0, one, 1, 1) != 0 and "IP-Adapter" in last_error(lib)
    assert lib.dk_mmdit_set_dual_attention(h0, 1) != 0 and "IP-Adapter" in last_error(lib)
    lib.dk_mmdit_destroy(h0)
    # non-bf16 activations: fp16 is the head_dim 64, depth_unified 0 family's; a FLUX-geometry handle of that shape takes it, and then no adapter
    half = replace(tiny_flux(2, 0, heads=4, head_dim=64), rope_axes_dim=(8, 28, 28))
    lib, hf = make_handle(half)
    assert lib.dk_mmdit_set_activation_dtype(hf, 1) == 0, last_error(lib)
    assert setip(4, 256, hf) != 0 and "an IP-Adapter needs bf16 activations" in last_error(lib)
    lib.dk_mmdit_destroy(hf)
    assert setip(0, 0) == 0 and lib.dk_mmdit_workspace_bytes(h, *shape) == plain  # (off again: the plain carve)
    # ... and the other way round
    for setter, undo, msg in ((lambda: lib.dk_mmdit_set_block_cache(h, 1), lambda: lib.dk_mmdit_set_block_cache(h, 0), "block cache"),
                              (lambda: lib.dk_mmdit_set_reference_grid(h, 8, 8), lambda: lib.dk_mmdit_set_reference_grid(h, 0, 0), "reference grid"),
                              (lambda: lib.dk_mmdit_set_condition_width(h, 64), lambda: lib.dk_mmdit_set_condition_width(h, 0), "condition width"),
                              (lambda: lib.dk_mmdit_set_flux_control_taps(h, taps, 1, 1, ctypes.c_float(0.7)),
                               lambda: lib.dk_mmdit_set_flux_control_taps(h, None, 0, 0, ctypes.c_float(0.0)), "control taps")):
        assert setter() == 0, last_error(lib)
        assert setip(4, 256) != 0 and msg in last_error(lib)
        assert undo() == 0
    lib.dk_mmdit_destroy(h)
    lib, h8 = make_handle(tiny_flux(2, 2), fp8=True)
    assert setip(4, 256, h8) != 0 and "fp8" in last_error(lib)
    lib.dk_mmdit_destroy(h8)
    lib, hs = make_handle(tiny_sd3())
    assert setip(4, 256, hs) != 0 and "SD3 geometry is refused" in last_error(lib)
    lib.dk_mmdit_destroy(hs)
    lib, hc = make_handle(tiny_flux_controlnet(2, 1))
    assert lib.dk_mmdit_set_flux_control_net(hc, 1) == 0 and setip(4, 256, hc) != 0 and "control-net engine" in last_error(lib)
    lib.dk_mmdit_destroy(hc)
    # the kernel's entry: N and D outside the build are refused by name before anything is launched
    p = ctypes.c_void_p(256)
    call = lambda n, d: lib.dk_ip_attention_bf16(p, 768, 5, 8, 3, p, p, p, 256, 1, n, 256, d, ctypes.c_float(0.1), ctypes.c_float(1e-6), p, None)
    assert call(17, 128) != 0 and "[1, 16]" in last_error(lib)
    assert call(0, 128) != 0 and "[1, 16]" in last_error(lib)
    assert call(4, 64) != 0 and "head_dim must be 128" in last_error(lib)


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def parse(argv):
    return cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args(argv)


def test_cli_parsing_and_refusals():
    base = ["--prompt", "x", "--model-version", "argmaxinc/mlx-FLUX.1-schnell", "--ip-adapter", "ip.safetensors", "--ip-adapter-embeds", "e.npy"]
    r = cli.resolve(parse(base + ["--ip-adapter-scale", "0.6", "--sampler", "heun"]))
    assert (r["ip_adapter_ckpt"], r["ip_adapter_image_embeds"], r["ip_adapter_scale"], r["flux"]) == ("ip.safetensors", "e.npy", 0.6, True)
    assert "ip_adapter_scale" not in cli.resolve(parse(base)) and "ip_adapter_ckpt" not in cli.resolve(parse(["--prompt", "x"]))
    with pytest.raises(ValueError, match="need --ip-adapter"):
        cli.resolve(parse(["--prompt", "x", "--ip-adapter-scale", "0.5"]))
    with pytest.raises(ValueError, match="needs --ip-adapter-embeds"):
        cli.resolve(parse(["--prompt", "x", "--ip-adapter", "ip.safetensors"]))
    with pytest.raises(ValueError, match="needs a FLUX model version"):
        cli.resolve(parse(["--prompt", "x", "--model-version", "argmaxinc/mlx-stable-diffusion-3-medium"] + base[4:]))
    for argv, msg in ((["--fp8", "quality"], "--fp8"), (["--block-cache", "0.1"], "--block-cache"), (["--reference-image-path", "r.png"], "--reference-image-path"),
                      (["--condition", "control", "--condition-image-path", "c.png"], "--condition"),
                      (["--controlnet", "cn.safetensors", "--controlnet-image-path", "e.png", "--controlnet-blocks", "2", "2"], "--controlnet")):
        with pytest.raises(ValueError, match=f"--ip-adapter cannot run together with {msg}"):
            cli.resolve(parse(base + argv))


# ---- the pipeline's refusals ----------------------------------------------------------------------------------------------------------
def stub(cfg, flux=True, condition=None):
    return SimpleNamespace(mmdit_config=cfg, _IS_FLUX=flux, condition=condition)


def test_constructor_refusals():
    with pytest.raises(ValueError, match="FLUX family's.*SD3 and SD3.5"):
        _check_ip_adapter_config(stub(tiny_sd3(), flux=False), None, None)
    with pytest.raises(ValueError, match="fp8"):
        _check_ip_adapter_config(stub(fp8_config(tiny_flux())), IPC, None)
    with pytest.raises(ValueError, match="condition="):
        _check_ip_adapter_config(stub(tiny_flux(condition_features=64), condition="control"), IPC, None)
    with pytest.raises(ValueError, match="controlnet_ckpt"):
        _check_ip_adapter_config(stub(tiny_flux()), IPC, {"some": "controlnet"})
    with pytest.raises(ValueError, match="bfloat16 activations"):
        _check_ip_adapter_config(stub(replace(tiny_flux(), activation_dtype="float16")), IPC, None)
    with pytest.raises(ValueError, match="IPAdapterConfig"):
        _check_ip_adapter_config(stub(tiny_flux()), tiny_flux(), None)
    with pytest.raises(ValueError, match=r"\[1, 16\].*InstantX"):
        _check_ip_adapter_config(stub(tiny_flux()), replace(IPC, ip_adapter_tokens=128), None)
    p = stub(tiny_flux(3, 2))
    _check_ip_adapter_config(p, None, None)
    assert p.ip_adapter_config is FLUX_IP_ADAPTER
    _check_ip_adapter_config(p, IPC, None)
    assert p.ip_adapter_config is IPC


def test_call_refusals():
    e = np.zeros(IPC.embed_dim, dtype=np.float32)
    without, with_ip = SimpleNamespace(ip_adapter_config=None), SimpleNamespace(ip_adapter_config=IPC)
    opts = lambda pipe, n=1, **kw: _ip_adapter_options(pipe, kw.get("embeds"), kw.get("scale", 1.0), n, kw.get("cfg", 0.0), kw.get("block_cache"),
                                                       kw.get("reference"))
    assert opts(without) is None and opts(without, reference=e) is None
    with pytest.raises(ValueError, match="need a pipeline built with an IP-Adapter"):
        opts(without, embeds=e)
    with pytest.raises(ValueError, match="need a pipeline built with an IP-Adapter"):
        opts(without, scale=0.5)
    with pytest.raises(ValueError, match="needs ip_adapter_image_embeds in every call"):
        opts(with_ip)
    with pytest.raises(ValueError, match="cfg_weight > 0.*negative image embeds"):
        opts(with_ip, embeds=e, cfg=3.5)
    with pytest.raises(ValueError, match="block_cache"):
        opts(with_ip, embeds=e, block_cache=0.1)
    with pytest.raises(ValueError, match="reference_image_path"):
        opts(with_ip, embeds=e, reference="r.png")
    with pytest.raises(ValueError, match="finite"):
        opts(with_ip, embeds=e, scale=float("nan"))
    with pytest.raises(ValueError, match=f"E = {IPC.embed_dim}"):
        opts(with_ip, embeds=np.zeros(IPC.embed_dim + 1, dtype=np.float32))
    with pytest.raises(ValueError, match="3 image embeddings for 2 seeds"):
        opts(with_ip, n=2, embeds=[e, e, e])
    assert opts(with_ip, embeds=e, scale=0.5)["scale"] == 0.5
    assert opts(with_ip, embeds=e)["embeds"].shape == (1, IPC.embed_dim) and opts(with_ip, n=2, embeds=[e, e])["embeds"].shape == (2, IPC.embed_dim)
    assert opts(with_ip, n=2, embeds=torch.zeros(2, IPC.embed_dim))["embeds"].shape == (2, IPC.embed_dim)


def test_sharding_is_refused():
    from diffusionkit_amd import dist
    with pytest.raises(ValueError, match="IP-Adapter cannot run under multi-GPU sharding"):
        dist.generate_sharded(SimpleNamespace(controlnet=None, ip_adapter_config=IPC), "x", [0, 1], 0, 2)
    with pytest.raises(ValueError, match="IP-Adapter cannot run under multi-GPU sharding"):
        dist.generate_sharded(SimpleNamespace(controlnet=None, ip_adapter_config=None), "x", [0, 1], 0, 2, ip_adapter_image_embeds=np.zeros(4))
