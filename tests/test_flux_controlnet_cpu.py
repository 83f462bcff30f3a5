"""FLUX ControlNet without a GPU: the index rule, the checkpoint loader, the configuration and the packed names, the C ABI's refusals on a
host-only handle, the command line, the pipeline's refusals, and the condition that makes the GPU parity test of the main engine mean
something -- every one of its seven tap sites moves the fp32 oracle's output by ten times the gate's absolute term."""
import ctypes
from dataclasses import replace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from diffusionkit_amd import cli
from diffusionkit_amd.config import (FLUX_DEV, MMDIT_CKPT, fp8_config, flux_controlnet_config, tiny_flux, tiny_flux_controlnet, tiny_sd3,
                                     tiny_sd3_controlnet, validate_control_net, validate_control_net_flux)
from diffusionkit_amd.model_io import CheckpointError, flux_controlnet_checkpoint_to_reference, load_controlnet_checkpoint
from diffusionkit_amd.pipeline import DiffusionPipeline, _controlnet_options
from diffusionkit_amd.weights import adaln_order, pack_mmdit, synth_mmdit_weights
from oracle.mmdit import OracleMMDiT, Prec
from tests._flux_controlnet import (TAP_SCALE, ControlledFluxOracle, FluxControlNetOracle, flux_tap_index, sd3_tap_index, synthetic_taps,
                                    to_diffusers_flux_controlnet)
from tests._util import randn, rel_l2
from tests.test_mmditx_cpu import last_error, make_handle

GATE_ABS = 2e-3  # the absolute term of tests/test_gpu_model.py's yardstick_ok
FLUX = "argmaxinc/mlx-FLUX.1-schnell"


# ---- the index rule -------------------------------------------------------------------------------------------------------------------
def test_tap_index_is_diffusers_rule_in_integers():
    for depth in range(1, 65):
        for n in range(1, depth + 1):
            for g in range(depth):
                want = int(g // np.ceil(depth / n))
                assert flux_tap_index(g, n, depth) == want and 0 <= want < n
    assert [flux_tap_index(g, 3, 4) for g in range(4)] == [0, 0, 1, 1]
    assert [sd3_tap_index(g, 3, 4) for g in range(4)] == [0, 0, 1, 2]  # (the SD3 rule differs at depth 4, n 3)
    assert [flux_tap_index(g, 2, 3) for g in range(3)] == [0, 0, 1] and [flux_tap_index(g, 5, 19) for g in (0, 3, 4, 18)] == [0, 0, 1, 4]


# ---- configuration and packing --------------------------------------------------------------------------------------------------------
def test_config_and_validators():
    c = flux_controlnet_config(5, 10)
    assert c.control_net_flux and not c.control_net and (c.depth_multimodal, c.depth_unified, c.hidden_size, c.num_heads, c.head_dim) == (5, 10, 3072, 24, 128)
    assert c.guidance_embed and c.rope_axes_dim == FLUX_DEV.rope_axes_dim and c.num_modulation_rows() == 5 * 12 + 10 * 3
    t = tiny_flux_controlnet()
    assert (t.depth_multimodal, t.depth_unified, t.hidden_size) == (2, 2, 256) and t.num_modulation_rows() == tiny_flux().num_modulation_rows() - 2
    assert "final_layer" not in adaln_order(t) and "final_layer" in adaln_order(tiny_flux())
    t0 = tiny_flux_controlnet(3, 0)
    assert t0.num_modulation_rows() == 2 * 12 + 8  # (the last text stream ends after attention: two rows)
    assert flux_controlnet_config(2, 1, fp8_config(tiny_flux())).weight_dtype == "bfloat16"
    for bad in (replace(tiny_sd3(), control_net_flux=True), replace(t, weight_dtype="fp8_e4m3"), replace(t, condition_features=64),
                replace(t, control_net=True)):
        with pytest.raises(ValueError, match="control_net_flux"):
            validate_control_net_flux(bad)
    for args in ((0, 2), (2, -1)):
        with pytest.raises(ValueError, match="n_double >= 1"):
            flux_controlnet_config(*args)
    with pytest.raises(ValueError, match="SD3 family"):  # (control_net stays the SD3 family's field)
        validate_control_net(replace(tiny_flux(), control_net=True))
    validate_control_net_flux(tiny_flux())  # (off: nothing to check)


def test_packing_names_and_a_plain_pack_is_what_it_was():
    cfg = tiny_flux_controlnet(2, 2)
    named = synth_mmdit_weights(cfg, seed=4321)
    h = cfg.hidden_size
    assert named["controlnet_x_embedder.proj.weight"].shape == (h, 1, 1, 64) and not any(k.startswith("final_layer") for k in named)
    packed = pack_mmdit(cfg, named, "cpu")
    assert packed["controlnet_x_embedder.proj.weight"].shape == (h, 64) and packed["adaLN.weight"].shape == (cfg.num_modulation_rows() * h, h)
    for kind in ("controlnet_blocks", "controlnet_single_blocks"):
        assert [k for k in sorted(packed) if k.startswith(kind + ".")] == [f"{kind}.{i}.{leaf}" for i in range(2) for leaf in ("bias", "weight")]
        assert packed[f"{kind}.1.weight"].shape == (h, h)
    assert "final_layer.linear.weight" not in packed and "pos_embed_input.proj.weight" not in packed
    with pytest.raises(ValueError, match="64 input features"):
        pack_mmdit(cfg, dict(named, **{"controlnet_x_embedder.proj.weight": torch.zeros(h, 1, 1, 128, dtype=torch.bfloat16)}), "cpu")
    # the weights of the shared layers are the plain model's stream, and a plain pack has no ControlNet tensor
    main = tiny_flux(2, 2)
    plain_named = synth_mmdit_weights(main, seed=4321)
    shared = [k for k in plain_named if not k.startswith("final_layer")]
    assert all(torch.equal(plain_named[k], named[k]) for k in shared)
    plain = pack_mmdit(main, plain_named, "cpu")
    assert "final_layer.linear.weight" in plain and not any("controlnet" in k for k in plain)
    assert plain["adaLN.weight"].shape[0] == main.num_modulation_rows() * h


# ---- the loader -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depths", [(2, 2), (3, 0)], ids=["2+2", "3+0"])
@pytest.mark.parametrize("guidance", [False, True], ids=["plain", "guidance"])
def test_loader_round_trip(depths, guidance):
    cfg = tiny_flux_controlnet(*depths, guidance_embed=guidance)
    w = synth_mmdit_weights(cfg, seed=4321)
    sd = to_diffusers_flux_controlnet(w, cfg)
    assert "controlnet_x_embedder.weight" in sd and sd["x_embedder.weight"].shape == (cfg.hidden_size, 64)
    assert ("time_text_embed.guidance_embedder.linear_1.weight" in sd) == guidance
    if depths[1]:
        assert sd["single_transformer_blocks.0.proj_out.weight"].shape == (cfg.hidden_size, 5 * cfg.hidden_size)
    back = flux_controlnet_checkpoint_to_reference(sd, cfg)
    assert set(back) == set(w) and all(torch.equal(back[k], w[k]) for k in w)
    assert set(load_controlnet_checkpoint(sd, cfg)) == set(w) and set(load_controlnet_checkpoint(w, cfg)) == set(w)


def test_loader_refusals():
    cfg = tiny_flux_controlnet(2, 2)
    sd = to_diffusers_flux_controlnet(synth_mmdit_weights(cfg, seed=4321), cfg)
    h = cfg.hidden_size
    drop = lambda k: {n: t for n, t in sd.items() if n != k}
    with pytest.raises(CheckpointError, match="controlnet_single_blocks.1.bias"):
        flux_controlnet_checkpoint_to_reference(drop("controlnet_single_blocks.1.bias"), cfg)
    with pytest.raises(CheckpointError, match="controlnet_x_embedder"):
        flux_controlnet_checkpoint_to_reference(drop("controlnet_x_embedder.weight"), cfg)
    with pytest.raises(CheckpointError, match="unknown FLUX ControlNet checkpoint key: transformer_blocks.0.attn.to_z.weight"):
        flux_controlnet_checkpoint_to_reference(dict(sd, **{"transformer_blocks.0.attn.to_z.weight": torch.zeros(h, h)}), cfg)
    with pytest.raises(CheckpointError, match="unknown FLUX ControlNet checkpoint key: norm_out.linear.weight"):
        flux_controlnet_checkpoint_to_reference(dict(sd, **{"norm_out.linear.weight": torch.zeros(2 * h, h)}), cfg)
    with pytest.raises(CheckpointError, match="controlnet_mode_embedder"):  # (a Union model)
        flux_controlnet_checkpoint_to_reference(dict(sd, **{"controlnet_mode_embedder.weight": torch.zeros(10, h)}), cfg)
    with pytest.raises(CheckpointError, match="input_hint_block"):  # (the XLabs layout)
        flux_controlnet_checkpoint_to_reference(dict(sd, **{"input_hint_block.0.weight": torch.zeros(16, 3, 3, 3)}), cfg)
    with pytest.raises(CheckpointError, match=r"\(2, 1\) of each"):
        flux_controlnet_checkpoint_to_reference(sd, tiny_flux_controlnet(2, 1))
    with pytest.raises(CheckpointError, match="guidance_embed = False"):
        flux_controlnet_checkpoint_to_reference(dict(sd, **{"time_text_embed.guidance_embedder.linear_1.weight": torch.zeros(h, 256)}), cfg)
    with pytest.raises(CheckpointError, match="control_net_flux=True"):
        flux_controlnet_checkpoint_to_reference(sd, tiny_flux(2, 2))
    with pytest.raises(CheckpointError, match="expected"):
        flux_controlnet_checkpoint_to_reference(dict(sd, **{"controlnet_x_embedder.weight": torch.zeros(h, 128)}), cfg)


# ---- the C ABI on a host-only handle ----------------------------------------------------------------------------------------------------
def test_abi_refusals_without_a_gpu():
    taps = ctypes.c_void_p(256)  # (a 16-byte-aligned address that is never read: every call below ends in the setter)
    lib, h = make_handle(tiny_flux(4, 3))
    assert lib.dk_abi_version() == 5
    set_taps = lambda nd, ns, m=h: lib.dk_mmdit_set_flux_control_taps(m, taps, nd, ns, ctypes.c_float(0.7))
    # the SD3 entries keep refusing FLUX geometry
    assert lib.dk_mmdit_set_control_net(h, 1) != 0 and "SD3 family" in last_error(lib)
    assert lib.dk_mmdit_set_control_taps(h, taps, 2, ctypes.c_float(1.0)) != 0 and "SD3 family" in last_error(lib)
    for nd, ns, msg in ((5, 0, "n_double_taps"), (-1, 2, "n_double_taps"), (0, 4, "n_single_taps")):
        assert set_taps(nd, ns) != 0 and msg in last_error(lib)
    assert lib.dk_mmdit_set_flux_control_taps(h, ctypes.c_void_p(264), 1, 1, ctypes.c_float(1.0)) != 0 and "16-byte aligned" in last_error(lib)
    for nd, ns in ((3, 2), (4, 3), (4, 0), (0, 3), (1, 1)):
        assert set_taps(nd, ns) == 0, last_error(lib)
    # while taps are set: a reference grid, a condition width and the block cache refuse; cleared, they are legal again
    assert lib.dk_mmdit_set_reference_grid(h, 8, 8) != 0 and "control taps" in last_error(lib)
    assert lib.dk_mmdit_set_condition_width(h, 64) != 0 and "control taps" in last_error(lib)
    assert lib.dk_mmdit_set_block_cache(h, 1) != 0 and "control taps" in last_error(lib)
    assert lib.dk_mmdit_set_flux_control_taps(h, None, 0, 0, ctypes.c_float(0.0)) == 0
    # ... and the other way round, each with its reason
    assert lib.dk_mmdit_set_reference_grid(h, 8, 8) == 0
    assert set_taps(1, 1) != 0 and "reference grid" in last_error(lib)
    assert lib.dk_mmdit_set_reference_grid(h, 0, 0) == 0 and lib.dk_mmdit_set_condition_width(h, 64) == 0
    assert set_taps(1, 1) != 0 and "condition width" in last_error(lib)
    assert lib.dk_mmdit_set_condition_width(h, 0) == 0 and lib.dk_mmdit_set_block_cache(h, 1) == 0
    assert set_taps(1, 1) != 0 and "block cache" in last_error(lib)
    assert lib.dk_mmdit_set_block_cache(h, 0) == 0 and set_taps(1, 1) == 0
    lib.dk_mmdit_destroy(h)
    # fp8 Linears
    lib, h8 = make_handle(tiny_flux(2, 2), fp8=True)
    assert set_taps(1, 1, h8) != 0 and "fp8" in last_error(lib)
    assert lib.dk_mmdit_set_flux_control_net(h8, 1) != 0 and "fp8" in last_error(lib)
    lib.dk_mmdit_destroy(h8)
    # SD3 geometry takes neither FLUX entry
    lib, hs = make_handle(tiny_sd3())
    assert set_taps(1, 0, hs) != 0 and "FLUX family" in last_error(lib)
    assert lib.dk_mmdit_set_flux_control_net(hs, 1) != 0 and "FLUX family" in last_error(lib)
    lib.dk_mmdit_destroy(hs)
    # the control-net engine: no final layer rows, no taps of its own, and depth_unified == 0 is legal
    for cfg in (tiny_flux_controlnet(2, 2), tiny_flux_controlnet(3, 0)):
        lib, hc = make_handle(cfg)
        rows = lib.dk_mmdit_mod_rows(hc)
        assert lib.dk_mmdit_set_flux_control_net(hc, 1) == 0, last_error(lib)
        assert lib.dk_mmdit_mod_rows(hc) == rows - 2 == cfg.num_modulation_rows()
        assert set_taps(1, 0, hc) != 0 and "control-net engine" in last_error(lib)
        assert lib.dk_mmdit_set_block_cache(hc, 1) != 0 and "control-net engine" in last_error(lib)
        lib.dk_mmdit_destroy(hc)


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def parse(argv):
    return cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args(argv)


def test_cli_parsing_and_refusals():
    base = ["--prompt", "x", "--controlnet", "cn.safetensors", "--controlnet-image-path", "edges.png"]
    r = cli.resolve(parse(base + ["--controlnet-blocks", "5", "10", "--controlnet-scale", "0.6", "--sampler", "heun"]))
    c = r["controlnet_config"]
    assert c.control_net_flux and (c.depth_multimodal, c.depth_unified, c.hidden_size) == (5, 10, 3072)
    assert (r["controlnet_ckpt"], r["controlnet_image_path"], r["controlnet_scale"], r["flux"]) == ("cn.safetensors", "edges.png", 0.6, True)
    with pytest.raises(ValueError, match="SD3 model version"):  # (without the flag: the line an SD3-only build answered with)
        cli.resolve(parse(base))
    with pytest.raises(ValueError, match="--controlnet-blocks"):
        cli.resolve(parse(base))
    for argv, msg in ((["--fp8", "quality"], "--fp8"), (["--block-cache", "0.1"], "--block-cache"), (["--reference-image-path", "r.png"], "--reference-image-path"),
                      (["--condition", "control", "--condition-image-path", "c.png"], "--condition")):
        with pytest.raises(ValueError, match=msg):
            cli.resolve(parse(base + ["--controlnet-blocks", "2", "2"] + argv))
    with pytest.raises(ValueError, match="need --controlnet"):
        cli.resolve(parse(["--prompt", "x", "--controlnet-blocks", "2", "2"]))
    with pytest.raises(ValueError, match="FLUX family's"):
        cli.resolve(parse(base + ["--model-version", "argmaxinc/mlx-stable-diffusion-3-medium", "--controlnet-blocks", "2", "2"]))
    with pytest.raises(ValueError, match="n_double >= 1"):
        cli.resolve(parse(base + ["--controlnet-blocks", "0", "2"]))
    with pytest.raises(SystemExit):
        parse(base + ["--controlnet-blocks", "5"])


# ---- the pipeline's refusals ----------------------------------------------------------------------------------------------------------
def stub(cfg, flux=True, condition=None):
    return SimpleNamespace(mmdit_config=cfg, _IS_FLUX=flux, condition=condition)


def test_constructor_refusals():
    check = DiffusionPipeline._check_controlnet_config
    with pytest.raises(ValueError, match="SD3 family.*names its ControlNet's depths"):
        check(stub(tiny_flux()), None)
    with pytest.raises(ValueError, match="control_net_flux=True"):
        check(stub(tiny_flux()), tiny_flux())
    with pytest.raises(ValueError, match="control_net_flux=True"):
        check(stub(tiny_flux()), tiny_sd3_controlnet())
    with pytest.raises(ValueError, match="fp8"):
        check(stub(fp8_config(tiny_flux())), tiny_flux_controlnet())
    with pytest.raises(ValueError, match="condition="):
        check(stub(tiny_flux(condition_features=64), condition="control"), tiny_flux_controlnet())
    for bad in (tiny_flux_controlnet(3, 2), tiny_flux_controlnet(2, 3), tiny_flux_controlnet(2, 2, heads=4)):
        with pytest.raises(ValueError, match="does not fit the model"):
            check(stub(tiny_flux(2, 2)), bad)
    with pytest.raises(ValueError, match="FLUX ControlNet's"):
        check(stub(tiny_sd3(), flux=False), tiny_flux_controlnet())
    p = stub(tiny_flux(4, 3))
    check(p, tiny_flux_controlnet(2, 1))
    assert p.controlnet_config.control_net_flux and (p.controlnet_config.depth_multimodal, p.controlnet_config.depth_unified) == (2, 1)


def test_call_refusals():
    image = np.zeros((64, 96, 3), dtype=np.uint8)
    without, with_cn = SimpleNamespace(controlnet=None), SimpleNamespace(controlnet=object())
    opts = lambda pipe, **kw: _controlnet_options(pipe, kw.get("image"), kw.get("scale", 1.0), kw.get("interval"), 1, (64, 96), kw.get("block_cache"), None, None,
                                                  kw.get("reference"), kw.get("condition"))
    assert opts(without) is None and opts(without, reference=image) is None  # (a reference alone is no ControlNet keyword)
    with pytest.raises(ValueError, match="need a pipeline built with a ControlNet"):
        opts(without, image=image)
    with pytest.raises(ValueError, match="needs controlnet_image_path in every call"):
        opts(with_cn)
    with pytest.raises(ValueError, match="reference_image_path"):
        opts(with_cn, image=image, reference=image)
    with pytest.raises(ValueError, match="condition"):
        opts(with_cn, image=image, condition="control")
    with pytest.raises(ValueError, match="block_cache"):
        opts(with_cn, image=image, block_cache=0.1)
    assert opts(with_cn, image=image, scale=0.5)["scale"] == 0.5


def test_sharding_is_refused():
    from diffusionkit_amd import dist
    with pytest.raises(ValueError, match="cannot run under multi-GPU sharding"):
        dist.generate_sharded(SimpleNamespace(controlnet=object()), "x", [0, 1], 0, 2)
    with pytest.raises(ValueError, match="cannot run under multi-GPU sharding"):
        dist.generate_sharded(SimpleNamespace(controlnet=None), "x", [0, 1], 0, 2, controlnet_image_path="e.png")


# ---- the oracles ----------------------------------------------------------------------------------------------------------------------
B, HL, WL, S_T, TS = 2, 8, 12, 20, [1000.0, 752.0, 500.0]


def _inputs(cfg):
    return randn(B, S_T, cfg.token_level_text_embed_dim, seed=3), randn(B, cfg.pooled_text_embed_dim, seed=4), randn(B, HL, WL, 16, seed=5)


def _final(m, cfg, control):
    text, pooled, lat = _inputs(cfg)
    m.control = control
    m.cache_modulation_params(pooled, torch.tensor(TS))
    streams = {}
    m(lat, text, TS[1], taps=streams)
    return streams["final"]


def test_every_tap_site_moves_the_oracle_by_ten_times_the_gate():
    """(4 double, 3 single) with one tap per block: zeroing any ONE tap moves the fp32 oracle's final output by >= 10 x 2e-3 (rel-L2, the gate's
    measure), so an engine that misses one site -- or indexes it wrongly -- cannot pass tests/test_gpu_flux_controlnet.py's (4, 3) case.  A
    condition on the synthetic taps (tests/_flux_controlnet.py: TAP_STD, TAP_SCALE), not a measurement of any engine."""
    cfg = tiny_flux(4, 3)
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    taps = synthetic_taps(7, B, (HL // 2) * (WL // 2), cfg.hidden_size)
    m = ControlledFluxOracle(cfg, wf, Prec())
    full = _final(m, cfg, (taps, 4, TAP_SCALE))
    for j in range(7):
        t = taps.clone()
        t[j] = 0
        moved = rel_l2(full, _final(m, cfg, (t, 4, TAP_SCALE)))
        assert moved >= 10 * GATE_ABS, f"tap {j}: zeroing it moves the output by {moved:.3e} only"
    # without taps, and with zero taps, the subclass is the pinned oracle
    plain = _final(m, cfg, None)
    text, pooled, lat = _inputs(cfg)
    base = OracleMMDiT(cfg, wf, Prec())
    base.cache_modulation_params(pooled, torch.tensor(TS))
    streams = {}
    base(lat, text, TS[1], taps=streams)
    assert torch.equal(plain, streams["final"]) and torch.equal(_final(m, cfg, (torch.zeros_like(taps), 4, TAP_SCALE)), plain)


def test_index_rule_shows_in_the_oracle():
    """(3, 2) taps on (4, 3): swapping double taps 1 and 2 -- where the SD3 rule would read tap 2 behind block 3 and the FLUX rule never does --
    leaves blocks 0 .. 3 reading taps 0, 0, 1, 1: the output moves exactly when tap 1 changes"""
    cfg = tiny_flux(4, 3)
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    taps = synthetic_taps(5, B, (HL // 2) * (WL // 2), cfg.hidden_size)
    m = ControlledFluxOracle(cfg, wf, Prec())
    full = _final(m, cfg, (taps, 3, TAP_SCALE))
    unused = taps.clone()
    unused[2] = 0  # (double tap 2: never read under ceil(4 / 3) = 2)
    assert torch.equal(_final(m, cfg, (unused, 3, TAP_SCALE)), full)
    used = taps.clone()
    used[1] = 0
    assert rel_l2(full, _final(m, cfg, (used, 3, TAP_SCALE))) >= 10 * GATE_ABS


def test_controlnet_oracle_shapes_and_no_single_blocks():
    for depths in ((2, 2), (3, 0)):
        cfg = tiny_flux_controlnet(*depths)
        wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=4321).items()}
        text, pooled, lat = _inputs(cfg)
        m = FluxControlNetOracle(cfg, wf, Prec())
        m.cache_modulation_params(pooled, torch.tensor(TS))
        ctrl = randn(1, HL, WL, 16, seed=6)
        taps = m(lat, text, TS[1], ctrl)
        assert tuple(taps.shape) == (sum(depths), B, (HL // 2) * (WL // 2), cfg.hidden_size) and bool(torch.isfinite(taps).all())
        assert torch.equal(taps, m(lat, text, TS[1], ctrl.expand(B, -1, -1, -1)))  # (a shared control image is a repeated one)
        assert rel_l2(taps, m(lat, text, TS[1], randn(1, HL, WL, 16, seed=7))) > 0.05
