"""CPU-side checks of the float16 VAE (the reference decodes Stable Diffusion 3 latents with an fp16 decoder, mlx/__init__.py:108-113,483-484):
the config field and helper, weight packing, the CLI flag, the C-ABI additions, the handle's dtype setter and the route of an fp16 conv-form
launch (dk_conv3x3_plan_f16: no kernel runs)."""
import ctypes as C
import re
from dataclasses import replace

import pytest
import torch

from diffusionkit_amd import _lib, cli
from diffusionkit_amd.config import MMDIT_CKPT, VAEDecoderConfig, VAEEncoderConfig, tiny_vae, tiny_vae_encoder

F16_VAE_SYMBOLS = ("dk_vae_set_dtype", "dk_conv3x3_f16", "dk_conv3x3_plan", "dk_conv3x3_plan_f16", "dk_conv3x3_ws_f16", "dk_conv3x3_ws_plan",
                   "dk_conv3x3_ws_plan_f16", "dk_conv3x3_gn_f16", "dk_groupnorm_f16",
                   "dk_groupnorm_table_f16", "dk_attention_d512_f16", "dk_softmax_rows_f16", "dk_transpose_f16", "dk_latent_sample_f16")


def test_default_is_bfloat16_and_the_helper_takes_both_halves():
    from diffusionkit_amd.config import float16_vae_config
    assert VAEDecoderConfig().dtype == "bfloat16" and VAEEncoderConfig().dtype == "bfloat16"
    assert tiny_vae().dtype == "bfloat16" and tiny_vae_encoder().dtype == "bfloat16"
    for cfg in (VAEDecoderConfig(), VAEEncoderConfig(), tiny_vae(), tiny_vae_encoder()):
        c = float16_vae_config(cfg)
        assert type(c) is type(cfg) and c.dtype == "float16" and replace(c, dtype="bfloat16") == cfg
        assert float16_vae_config(cfg, "bfloat16") == cfg
        with pytest.raises(ValueError, match="unknown VAE dtype"):
            float16_vae_config(cfg, "float32")
    with pytest.raises(ValueError):
        float16_vae_config(object())


@pytest.mark.parametrize("half", ["decoder", "encoder"])
def test_pack_vae_packs_in_the_config_dtype_and_rounds_once(half):
    from diffusionkit_amd.config import float16_vae_config
    from diffusionkit_amd.weights import pack_vae, synth_vae_encoder_weights, synth_vae_weights
    cfg = tiny_vae() if half == "decoder" else tiny_vae_encoder()
    w = {k: v.float() for k, v in (synth_vae_weights(cfg, seed=5) if half == "decoder" else synth_vae_encoder_weights(cfg, seed=5)).items()}
    w["conv_out.bias"][0] = 1.0 + 2.0 ** -10  # one fp16 ulp above 1: not a bf16 value
    w["conv_out.bias"][1] = 1.0 + 2.0 ** -12  # not an fp16 value either: rounds (once) to 1
    pbf, p16 = pack_vae(cfg, w, "cpu"), pack_vae(float16_vae_config(cfg), w, "cpu")
    assert set(pbf) == set(p16) and any(k.endswith(".conv2_sc.weight") for k in pbf)
    cin = cfg.in_channels
    for k, t in w.items():
        if k == "conv_in.weight":  # the channel pad to 64 stays, in both element types
            o = t.shape[0]
            src = torch.zeros(o, 3, 3, 64)
            src[..., :cin] = t
            src = src.reshape(o, -1)
            assert p16[k].shape == (o, 9 * 64) and torch.all(p16[k].reshape(o, 3, 3, 64)[..., cin:] == 0)
        else:
            src = t.reshape(t.shape[0], -1) if t.dim() == 4 else t
        assert p16[k].dtype == torch.float16 and torch.equal(p16[k], src.to(torch.float16)), k
        assert pbf[k].dtype == torch.bfloat16 and torch.equal(pbf[k], src.to(torch.bfloat16)), k  # the default: the tensors of before
        assert p16[k].is_contiguous() and p16[k].shape == pbf[k].shape
    assert float(p16["conv_out.bias"][0]) == 1.0 + 2.0 ** -10 and float(pbf["conv_out.bias"][0]) == 1.0
    assert float(p16["conv_out.bias"][1]) == 1.0
    for k in pbf:
        if k.endswith(".conv2_sc.weight"):
            stem = k[:-len(".conv2_sc.weight")]
            assert torch.equal(p16[k], torch.cat([p16[stem + ".conv2.weight"], p16[stem + ".conv_shortcut.weight"]], dim=1))
    # an fp16 checkpoint tensor reaches the engine bit for bit
    q16 = pack_vae(float16_vae_config(cfg), {k: v.to(torch.float16) for k, v in w.items()}, "cpu")
    assert all(torch.equal(q16[k], p16[k]) for k in p16)
    with pytest.raises(ValueError, match="unknown VAE dtype"):
        pack_vae(replace(cfg, dtype="float32"), w, "cpu")


def test_cli_flag_and_default():
    parser = cli.build_parser(tuple(MMDIT_CKPT))
    base = ["--prompt", "x", "--model-version", "argmaxinc/mlx-stable-diffusion-3-medium"]
    assert parser.parse_args(base).vae_dtype is None
    assert "vae_dtype" not in cli.resolve(parser.parse_args(base))  # a key only when the flag is given
    for v in ("float16", "bfloat16"):
        r = cli.resolve(parser.parse_args(base + ["--vae-dtype", v]))
        assert r["vae_dtype"] == v and "activation_dtype" not in r
    r = cli.resolve(parser.parse_args(base + ["--vae-dtype", "float16", "--activation-dtype", "float16"]))
    assert r["vae_dtype"] == "float16" and r["activation_dtype"] == "float16"
    # the VAE's own switch: every family takes it
    r = cli.resolve(parser.parse_args(["--prompt", "x", "--model-version", "argmaxinc/mlx-FLUX.1-schnell", "--vae-dtype", "float16"]))
    assert r["vae_dtype"] == "float16" and r["flux"]
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--vae-dtype", "float32"])


def test_pipeline_rejects_an_unknown_vae_dtype():
    from diffusionkit_amd.config import tiny_sd3
    from diffusionkit_amd.pipeline import DiffusionPipeline
    with pytest.raises(ValueError, match="unknown VAE dtype"):
        DiffusionPipeline(w16=True, a16=True, vae_dtype="float32", device="cpu", mmdit_config=tiny_sd3(), vae_config=tiny_vae())


def test_new_symbols_in_header_library_and_ctypes_table():
    lib = _lib.load()
    header = set(re.findall(r"\b(dk_[a-z0-9_]+)\s*\(", open(_lib.HEADER_PATH).read()))
    for s in F16_VAE_SYMBOLS:
        assert s in header and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.dk_abi_version() == 5  # purely additive


def _create(cfg):
    lib = _lib.load()
    c = _lib.dk_vae_config()
    c.in_channels, c.out_channels = cfg.in_channels, cfg.out_channels
    for i, ch in enumerate(cfg.block_out_channels):
        c.block_out_channels[i] = ch
    c.n_blocks, c.layers_per_block, c.resnet_groups, c.group_norm_eps = len(cfg.block_out_channels), cfg.layers_per_block, cfg.resnet_groups, cfg.group_norm_eps
    h = C.c_void_p()
    assert lib.dk_vae_create(C.byref(c), C.byref(h)) == 0, lib.dk_last_error()
    return h


def test_setter_refuses_unknown_codes_and_a_change_of_mind():
    lib = _lib.load()
    for cfg in (tiny_vae(), tiny_vae_encoder()):
        h = _create(cfg)
        for bad in (2, -1, 16):
            assert lib.dk_vae_set_dtype(h, bad) != 0 and b"0 bf16, 1 fp16" in lib.dk_last_error()
        assert lib.dk_vae_set_dtype(h, 1) == 0
        assert lib.dk_vae_set_dtype(h, 1) == 0  # naming the type already set: accepted
        assert lib.dk_vae_set_dtype(h, 0) != 0 and b"precede the first dk_vae_bind" in lib.dk_last_error()
        buf = torch.zeros(64)
        assert lib.dk_vae_bind(h, b"conv_in.bias", buf.data_ptr()) == 0
        assert lib.dk_vae_set_dtype(h, 1) == 0 and lib.dk_vae_set_dtype(h, 0) != 0
        lib.dk_vae_destroy(h)
        # a handle nobody set anything on is bf16: after a bind only 0 is accepted
        h = _create(cfg)
        assert lib.dk_vae_bind(h, b"conv_in.bias", buf.data_ptr()) == 0
        assert lib.dk_vae_set_dtype(h, 1) != 0 and b"precede the first dk_vae_bind" in lib.dk_last_error()
        assert lib.dk_vae_set_dtype(h, 0) == 0
        lib.dk_vae_destroy(h)
    assert lib.dk_vae_set_dtype(None, 1) != 0


def test_engines_refuse_host_tensors_and_unknown_dtypes():
    """the boundary check of the fp16 engines names what it expects (fp16 tensors on the device); no GPU needed to get that far"""
    from diffusionkit_amd.config import float16_vae_config
    from diffusionkit_amd.engine import VAEDecoderEngine, VAEEncoderEngine
    from diffusionkit_amd.weights import pack_vae, synth_vae_encoder_weights, synth_vae_weights
    cfg, ecfg = float16_vae_config(tiny_vae()), float16_vae_config(tiny_vae_encoder())
    with pytest.raises(_lib.DkHipError, match="GPU"):
        VAEDecoderEngine(cfg, pack_vae(cfg, synth_vae_weights(cfg), "cpu"))
    with pytest.raises(_lib.DkHipError, match="GPU"):
        VAEEncoderEngine(ecfg, pack_vae(ecfg, synth_vae_encoder_weights(ecfg), "cpu"))
    with pytest.raises(_lib.DkHipError, match="unknown VAE dtype"):
        VAEDecoderEngine(replace(tiny_vae(), dtype="float32"), {})


CONV_CASES = [(1, 16, 16, 64, 128, 0), (2, 6, 10, 64, 128, 0), (1, 16, 24, 64, 64, 1), (1, 16, 16, 128, 256, 0), (1, 8, 8, 128, 128, 2),
              (1, 224, 224, 64, 256, 0), (1, 128, 96, 128, 256, 0)]


def _plan_fields(p):
    return [getattr(p, f) for f, _ in p._fields_]


def test_f16_conv_plan_reports_the_conv_form_routes():
    """dk_conv3x3_plan_f16: an fp16 convolution takes the route of its bf16 twin -- the 128 x 128 kernel's conv form for the small stages, gemm256v3's
    (generation 3) where O % 256 == 0 and the tiles fill the CUs or when forced; never generation 4"""
    from diffusionkit_amd import ops
    F16, BF = torch.float16, torch.bfloat16
    for (B, H, W, Cc, O, ups) in CONV_CASES:
        a, b = ops.conv3x3_plan(B, H, W, Cc, O, ups, dtype=BF), ops.conv3x3_plan(B, H, W, Cc, O, ups, dtype=F16)
        assert _plan_fields(a) == _plan_fields(b), (B, H, W, Cc, O, ups)
        assert b.launches == 1 and b.kernel in (128, 3)
    assert ops.conv3x3_plan(1, 16, 16, 128, 256, dtype=F16).kernel == 128
    assert ops.conv3x3_plan(1, 224, 224, 64, 256, dtype=F16, res=True).kernel == 3  # 196 tiles: the automatic choice
    try:
        ops.tune("gemm", 9)
        p = ops.conv3x3_plan(1, 16, 16, 128, 256, dtype=F16)
        assert p.kernel == 3 and p.tile_rows in (224, 256)
        assert ops.conv3x3_plan(1, 16, 16, 64, 128, dtype=F16).kernel == 128  # O = 128: no 256-column form
        ops.tune("gemm", 10)  # "gemm256v4 where eligible": has no conv form and no fp16 form
        assert ops.conv3x3_plan(1, 224, 224, 64, 256, dtype=F16).kernel == 3
    finally:
        ops.tune("gemm", -1)
    with pytest.raises(_lib.DkHipError, match="bfloat16 or torch.float16"):
        ops.conv3x3_plan(1, 16, 16, 64, 128, dtype=torch.float32)
