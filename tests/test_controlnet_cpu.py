"""SD3 ControlNet without a GPU: the two new oracles tied to the pinned one, the tap-index and interval rules, the diffusers-layout loader,
the packed names, the command line and every refusal of the pipeline that needs no device."""
from dataclasses import replace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from diffusionkit_amd import cli
from diffusionkit_amd.config import (MMDIT_CKPT, SD3_2b, SD3_5_MEDIUM, SD3_CONTROLNET_6, fp8_config, tiny_flux, tiny_sd3, tiny_sd3_controlnet, tiny_sd35m,
                                     validate_control_net)
from diffusionkit_amd.model_io import CheckpointError, load_controlnet_checkpoint, sd3_controlnet_checkpoint_to_reference
from diffusionkit_amd.pipeline import DiffusionPipeline, _controlnet_options, controlnet_step_active
from diffusionkit_amd.weights import adaln_order, mmdit_weight_shapes, pack_mmdit, synth_mmdit_weights
from oracle.mmdit import OracleMMDiT, Prec
from tests._controlnet import ControlledOracle, ControlNetOracle, tap_index, to_diffusers_sd3_controlnet, with_full_last_block
from tests._util import BF, randn

SD3 = "argmaxinc/mlx-stable-diffusion-3-medium"
TS = [1000.0, 752.0]
B, HL, WL, S_T = 2, 8, 12, 20


def case(cfg):
    return (randn(B, S_T, cfg.token_level_text_embed_dim, seed=3), randn(B, cfg.pooled_text_embed_dim, seed=4), randn(B, HL, WL, 16, seed=5),
            randn(B, HL, WL, 16, seed=6))


def controlnet_taps(cfg, w, P=None, full_last=False):
    text, pooled, lat, ctrl = case(cfg)
    m = ControlNetOracle(cfg, {k: v.float() for k, v in w.items()}, P or Prec(), full_last=full_last)
    m.cache_modulation_params(pooled, torch.tensor(TS))
    return m(lat, text, TS[1], ctrl)


# ---- the oracles ----------------------------------------------------------------------------------------------------------------------
def test_zero_tap_linears_give_zero_taps_and_the_pinned_oracle():
    """with zero controlnet_blocks -- a fresh ControlNet -- every tap is exactly zero, and a main model that adds them is OracleMMDiT value for value"""
    cn_cfg, cfg = tiny_sd3_controlnet(depth=2, heads=4), tiny_sd3(depth=3, heads=4)
    w = synth_mmdit_weights(cn_cfg, seed=4321)
    assert float(w["controlnet_blocks.0.weight"].float().abs().max()) > 0 and float(w["pos_embed_input.proj.weight"].float().abs().max()) > 0
    taps = controlnet_taps(cn_cfg, {k: (torch.zeros_like(v) if k.startswith("controlnet_blocks.") else v) for k, v in w.items()})
    assert tuple(taps.shape) == (2, B, (HL // 2) * (WL // 2), cn_cfg.hidden_size) and not bool(taps.any())
    text, pooled, lat, _ = case(cfg)
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    for P in (Prec(), Prec(BF)):
        outs = []
        for cls, control in ((OracleMMDiT, None), (ControlledOracle, (taps, 0.7)), (ControlledOracle, None)):
            m = cls(cfg, wf, P)
            if cls is ControlledOracle:
                m.control = control
            m.cache_modulation_params(pooled, torch.tensor(TS))
            outs.append(m(lat, text, TS[1]))
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert float(controlnet_taps(cn_cfg, w).abs().max()) > 0  # (and the synthetic ControlNet's taps are not zero)


def test_last_blocks_text_half_changes_no_tap():
    """the published model runs the last block's text stream through its post-attention half; the engine stops it after attention: equal taps"""
    cfg = tiny_sd3_controlnet(depth=2, heads=4)
    w = synth_mmdit_weights(cfg, seed=4321)
    for P in (Prec(), Prec(BF)):
        assert torch.equal(controlnet_taps(cfg, with_full_last_block(w, cfg), P, full_last=True), controlnet_taps(cfg, w, P))


def test_controlled_oracle_adds_the_taps_by_the_rule():
    """depth 3 with 2 taps: tap 0 behind blocks 0 and 1, nothing behind block 2 -- restated on the streams the base class hands out"""
    cfg = tiny_sd3(depth=3, heads=4)
    text, pooled, lat, _ = case(cfg)
    taps = randn(2, B, (HL // 2) * (WL // 2), cfg.hidden_size, seed=11, scale=0.1)
    m = ControlledOracle(cfg, {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}, Prec())
    m.cache_modulation_params(pooled, torch.tensor(TS))
    m.control = (taps, 0.7)
    got = {}
    m(lat, text, TS[1], taps=got)
    m.control = None
    img, txt = got["embed_img"], got["embed_txt"]
    s = float(torch.tensor(0.7, dtype=torch.float32))
    for i in range(3):
        img, txt = m._double_block(i, img, txt, TS[1], None)
        if i < 2:
            img = img + s * taps[0]
        assert torch.equal(img, got[f"double{i}_img"])


# ---- the rules ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,n", [(24, 6), (24, 12), (38, 19), (3, 2), (4, 4), (5, 1)])
def test_tap_index_is_diffusers_float_rule(depth, n):
    interval_control = depth / n
    assert [tap_index(g, n, depth) for g in range(depth - 1)] == [int(g / interval_control) for g in range(depth - 1)]
    assert all(0 <= tap_index(g, n, depth) < n for g in range(depth))


def test_interval_rule_against_hand_written_step_sets():
    steps = lambda n, interval: [i for i in range(n) if controlnet_step_active(i, n, interval)]
    for n in (1, 4, 28):
        assert steps(n, None) == steps(n, (0, 1)) == steps(n, (0.0, 1.0)) == list(range(n))
        assert steps(n, (0.6, 0.4)) == [] and steps(n, (0.5, 0.5)) == []
    assert steps(1, (0, 0.5)) == [] and steps(1, (0.1, 1)) == []
    assert steps(4, (0, 0.5)) == [0, 1] and steps(4, (0.25, 0.75)) == [1, 2] and steps(4, (0.5, 1)) == [2, 3] and steps(4, (0, 0.67)) == [0, 1]
    assert steps(4, (0.3, 1)) == [2, 3] and steps(4, (0, 0.74)) == [0, 1]
    assert steps(28, (0, 0.67)) == list(range(18)) and steps(28, (0.5, 1)) == list(range(14, 28)) and steps(28, (0.2, 0.25)) == [6]
    assert steps(3, (0, 0.67)) == [0, 1]


# ---- the loader -----------------------------------------------------------------------------------------------------------------------
def test_loader_round_trip_and_last_context_slice():
    cfg = tiny_sd3_controlnet(depth=2, heads=4)
    h = cfg.hidden_size
    w = synth_mmdit_weights(cfg, seed=4321)
    for src in (w, with_full_last_block(w, cfg)):
        sd = to_diffusers_sd3_controlnet(src, cfg)
        assert tuple(sd["transformer_blocks.1.norm1_context.linear.weight"].shape) == (6 * h, h) and "transformer_blocks.1.attn.to_add_out.weight" in sd
        assert tuple(sd["pos_embed_input.proj.weight"].shape) == (h, 16, 2, 2) and "transformer_blocks.0.attn.add_k_proj.bias" in sd
        back = sd3_controlnet_checkpoint_to_reference(sd, cfg)
        assert set(back) == set(w) == set(mmdit_weight_shapes(cfg))
        for k in w:
            assert torch.equal(back[k], w[k]), k
        assert not any(k.startswith("final_layer") for k in back)
    # the last norm1_context keeps rows [0, 2h): shift_msa and scale_msa of the full module
    full = with_full_last_block(w, cfg)
    k = "multimodal_transformer_blocks.1.text_transformer_block.adaLN_modulation.layers.1.weight"
    assert tuple(full[k].shape) == (6 * h, h) and torch.equal(back[k], full[k][:2 * h]) and tuple(back[k].shape) == (2 * h, h)
    assert "multimodal_transformer_blocks.1.text_transformer_block.attn.o_proj.weight" not in back
    # load_controlnet_checkpoint: the diffusers layout, a file of it, and reference names
    assert set(load_controlnet_checkpoint(sd, cfg)) == set(w) and load_controlnet_checkpoint(w, cfg).keys() == w.keys()


def test_loader_reads_a_safetensors_file(tmp_path):
    from safetensors.torch import save_file
    cfg = tiny_sd3_controlnet(depth=2, heads=4)
    w = synth_mmdit_weights(cfg, seed=4321)
    path = str(tmp_path / "controlnet.safetensors")
    save_file(to_diffusers_sd3_controlnet(w, cfg), path)
    back = load_controlnet_checkpoint(path, cfg)
    assert all(torch.equal(back[k], w[k]) for k in w)


def test_loader_refusals():
    cfg = tiny_sd3_controlnet(depth=2, heads=4)
    h = cfg.hidden_size
    sd = to_diffusers_sd3_controlnet(synth_mmdit_weights(cfg, seed=4321), cfg)
    drop = lambda *keys: {k: v for k, v in sd.items() if k not in keys}
    with pytest.raises(CheckpointError, match="lacks 1 tensors"):
        sd3_controlnet_checkpoint_to_reference(drop("transformer_blocks.0.attn.to_q.weight"), cfg)
    with pytest.raises(CheckpointError, match="lacks 1 tensors"):
        sd3_controlnet_checkpoint_to_reference(drop("pos_embed_input.proj.bias"), cfg)
    with pytest.raises(CheckpointError, match="shape"):
        sd3_controlnet_checkpoint_to_reference(dict(sd, **{"controlnet_blocks.0.weight": torch.zeros(h, h + 8)}), cfg)
    with pytest.raises(CheckpointError, match="extra_conditioning_channels"):
        sd3_controlnet_checkpoint_to_reference(dict(sd, **{"pos_embed_input.proj.weight": torch.zeros(h, 17, 2, 2)}), cfg)
    with pytest.raises(CheckpointError, match="no joint blocks"):
        sd3_controlnet_checkpoint_to_reference({k: v for k, v in sd.items() if ".add_" not in k}, cfg)
    with pytest.raises(CheckpointError, match="2 blocks and 1 controlnet_blocks"):
        sd3_controlnet_checkpoint_to_reference(drop("controlnet_blocks.1.weight", "controlnet_blocks.1.bias"), cfg)
    with pytest.raises(CheckpointError, match="the configuration 3 of each"):
        sd3_controlnet_checkpoint_to_reference(sd, tiny_sd3_controlnet(depth=3, heads=4))
    with pytest.raises(CheckpointError, match="unknown SD3 ControlNet checkpoint key"):
        sd3_controlnet_checkpoint_to_reference(dict(sd, **{"transformer_blocks.0.attn2.to_q.weight": torch.zeros(h, h)}), cfg)
    with pytest.raises(CheckpointError, match="rows expected"):
        sd3_controlnet_checkpoint_to_reference(dict(sd, **{"transformer_blocks.1.norm1_context.linear.weight": torch.zeros(2 * h, h)}), cfg)
    with pytest.raises(CheckpointError, match="control-net configuration"):
        sd3_controlnet_checkpoint_to_reference(sd, tiny_sd3(depth=2, heads=4))


# ---- configuration and packing --------------------------------------------------------------------------------------------------------
def test_control_net_configs():
    assert SD3_CONTROLNET_6.control_net and SD3_CONTROLNET_6.depth_multimodal == 6
    assert (SD3_CONTROLNET_6.hidden_size, SD3_CONTROLNET_6.num_heads, SD3_CONTROLNET_6.head_dim) == (SD3_2b.hidden_size, 24, 64)
    cfg = tiny_sd3_controlnet()
    assert cfg.control_net and (cfg.depth_multimodal, cfg.num_heads, cfg.hidden_size) == (2, 4, 256)
    assert cfg.num_modulation_rows() == tiny_sd3().num_modulation_rows() - 2 and "final_layer" not in adaln_order(cfg)
    assert not SD3_2b.control_net and "final_layer" in adaln_order(tiny_sd3())
    for bad in (replace(tiny_flux(), control_net=True), replace(tiny_sd35m(), control_net=True), replace(fp8_config(tiny_flux()), control_net=True)):
        with pytest.raises(ValueError, match="SD3 family"):
            validate_control_net(bad)


def test_pack_mmdit_names_for_a_control_net():
    cfg = tiny_sd3_controlnet(depth=2, heads=4)
    h = cfg.hidden_size
    w = synth_mmdit_weights(cfg, seed=4321)
    assert not any(k.startswith("final_layer") for k in w) and set(w) - set(synth_mmdit_weights(tiny_sd3(depth=2, heads=4))) == {
        "pos_embed_input.proj.weight", "pos_embed_input.proj.bias", "controlnet_blocks.0.weight", "controlnet_blocks.0.bias",
        "controlnet_blocks.1.weight", "controlnet_blocks.1.bias"}
    packed = pack_mmdit(cfg, w, "cpu")
    assert tuple(packed["pos_embed_input.proj.weight"].shape) == (h, cfg.patch_dim) == tuple(packed["x_embedder.proj.weight"].shape)
    assert torch.equal(packed["pos_embed_input.proj.weight"], w["pos_embed_input.proj.weight"].reshape(h, -1))
    for i in range(2):
        assert torch.equal(packed[f"controlnet_blocks.{i}.weight"], w[f"controlnet_blocks.{i}.weight"]) and tuple(packed[f"controlnet_blocks.{i}.bias"].shape) == (h,)
    assert not any(k.startswith("final_layer") for k in packed) and tuple(packed["adaLN.weight"].shape) == (cfg.num_modulation_rows() * h, h)
    # a model's pack is what it was
    plain = pack_mmdit(tiny_sd3(depth=2, heads=4), synth_mmdit_weights(tiny_sd3(depth=2, heads=4)), "cpu")
    assert "final_layer.linear.weight" in plain and not any("controlnet" in k or "pos_embed_input" in k for k in plain)


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def parse(argv):
    return cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args(argv)


def test_cli_parsing():
    base = ["--prompt", "x", "--model-version", SD3]
    r = cli.resolve(parse(base))
    assert not any(k.startswith("controlnet") for k in r)  # (keys only when the flags are given)
    r = cli.resolve(parse(base + ["--controlnet", "cn.safetensors", "--controlnet-image-path", "edges.png"]))
    assert (r["controlnet_ckpt"], r["controlnet_image_path"]) == ("cn.safetensors", "edges.png") and "controlnet_scale" not in r and "controlnet_interval" not in r
    r = cli.resolve(parse(base + ["--controlnet", "cn.safetensors", "--controlnet-image-path", "edges.png", "--controlnet-scale", "0.7",
                                  "--controlnet-interval", "0", "0.67", "--sampler", "heun", "--guidance-interval", "0.2", "0.9"]))
    assert r["controlnet_scale"] == 0.7 and r["controlnet_interval"] == (0.0, 0.67) and r["sampler"] == "heun"
    for argv, msg in ((["--controlnet-image-path", "e.png"], "need --controlnet"), (["--controlnet-scale", "0.5"], "need --controlnet"),
                      (["--controlnet", "c"], "needs --controlnet-image-path"),
                      (["--controlnet", "c", "--controlnet-image-path", "e", "--block-cache", "0.1"], "--block-cache"),
                      (["--controlnet", "c", "--controlnet-image-path", "e", "--slg-scale", "2.5", "--skip-layers", "1"], "--slg-scale"),
                      (["--controlnet", "c", "--controlnet-image-path", "e", "--pag-scale", "3", "--pag-layers", "1"], "--pag-scale"),
                      (["--controlnet", "c", "--controlnet-image-path", "e", "--controlnet-interval", "0.8", "0.2"], "START <= STOP")):
        with pytest.raises(ValueError, match=msg):
            cli.resolve(parse(base + argv))
    with pytest.raises(ValueError, match="SD3 model version"):
        cli.resolve(parse(["--prompt", "x", "--controlnet", "c", "--controlnet-image-path", "e"]))  # (the default version is FLUX)
    with pytest.raises(ValueError, match="dual attention"):
        cli.resolve(parse(["--prompt", "x", "--model-version", "stabilityai/stable-diffusion-3.5-medium", "--controlnet", "c", "--controlnet-image-path", "e"]))
    with pytest.raises(SystemExit):
        parse(base + ["--controlnet-interval", "0.5"])


# ---- the pipeline's refusals ----------------------------------------------------------------------------------------------------------
def stub(cfg, flux=False):
    return SimpleNamespace(mmdit_config=cfg, _IS_FLUX=flux)


def test_constructor_refusals():
    check = DiffusionPipeline._check_controlnet_config
    with pytest.raises(ValueError, match="SD3 family"):
        check(stub(tiny_flux(), flux=True), None)
    with pytest.raises(ValueError, match="dual attention"):
        check(stub(SD3_5_MEDIUM), None)
    with pytest.raises(ValueError, match="fp8"):
        check(stub(replace(tiny_sd3(), weight_dtype="fp8_e4m3")), None)
    with pytest.raises(ValueError, match="control_net=True"):
        check(stub(tiny_sd3()), tiny_sd3())
    with pytest.raises(ValueError, match="does not fit the model"):
        check(stub(tiny_sd3(depth=2, heads=4)), tiny_sd3_controlnet(depth=2, heads=6))
    with pytest.raises(ValueError, match="does not fit the model"):
        check(stub(tiny_sd3(depth=2, heads=4)), tiny_sd3_controlnet(depth=3, heads=4))
    p = stub(SD3_2b)
    check(p, None)
    assert p.controlnet_config == SD3_CONTROLNET_6
    p = stub(replace(tiny_sd3(depth=3), activation_dtype="float16"))
    check(p, tiny_sd3_controlnet(depth=2))
    assert p.controlnet_config.activation_dtype == "float16" and p.controlnet_config.control_net


def test_call_refusals():
    image = np.zeros((64, 96, 3), dtype=np.uint8)
    without, with_cn = SimpleNamespace(controlnet=None), SimpleNamespace(controlnet=object())
    opts = lambda pipe, **kw: _controlnet_options(pipe, kw.get("image"), kw.get("scale", 1.0), kw.get("interval"), kw.get("n", 1), kw.get("hw", (64, 96)),
                                                  kw.get("block_cache"), kw.get("slg"), kw.get("pag"))
    assert opts(without) is None
    for kw in (dict(image=image), dict(scale=0.5), dict(interval=(0, 1))):
        with pytest.raises(ValueError, match="need a pipeline built with a ControlNet"):
            opts(without, **kw)
    with pytest.raises(ValueError, match="needs controlnet_image_path in every call"):
        opts(with_cn)
    with pytest.raises(ValueError, match="block_cache"):
        opts(with_cn, image=image, block_cache=0.1)
    with pytest.raises(ValueError, match="skip-layer or perturbed-attention"):
        opts(with_cn, image=image, slg={"scale": 2.5})
    with pytest.raises(ValueError, match="skip-layer or perturbed-attention"):
        opts(with_cn, image=image, pag={"scale": 3.0})
    with pytest.raises(ValueError, match="controlnet_scale must be finite"):
        opts(with_cn, image=image, scale=float("nan"))
    with pytest.raises(ValueError, match="controlnet_interval"):
        opts(with_cn, image=image, interval=(0.0, 0.5, 1.0))
    with pytest.raises(ValueError, match="it must have the output's size"):
        opts(with_cn, image=image, hw=(64, 64))
    with pytest.raises(ValueError, match="multiples of 16"):
        opts(with_cn, image=np.zeros((60, 96, 3), dtype=np.uint8), hw=(60, 96))
    with pytest.raises(ValueError, match="one per image"):
        opts(with_cn, image=[image, image, image], n=2)
    got = opts(with_cn, image=[image, image], n=2, scale=0.7, interval=(0, 0.67))
    assert tuple(got["pixels"].shape) == (2, 64, 96, 3) and got["scale"] == 0.7 and got["interval"] == (0.0, 0.67)
    assert tuple(opts(with_cn, image=image, n=2)["pixels"].shape) == (1, 64, 96, 3)


def test_multi_gpu_sharding_refuses_a_controlnet():
    from diffusionkit_amd.dist import generate_sharded
    with pytest.raises(ValueError, match="ControlNet"):
        generate_sharded(SimpleNamespace(controlnet=object()), "x", [1, 2], 0, 2)
    with pytest.raises(ValueError, match="ControlNet"):
        generate_sharded(SimpleNamespace(controlnet=None), "x", [1, 2], 0, 2, controlnet_image_path="e.png")
