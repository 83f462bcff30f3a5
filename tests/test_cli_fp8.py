"""``--fp8 quality|speed`` of diffusionkit_amd.cli: the switch in front of config.fp8_config (the fp8 path had no command-line form)."""
import numpy as np
import pytest

from diffusionkit_amd import cli
from diffusionkit_amd.config import FLUX_FP8_QUALITY_BLOCKS, MMDIT_CKPT, MODEL_CONFIG, fp8_config, tiny_flux, tiny_vae

FLUX = "argmaxinc/mlx-FLUX.1-schnell"


def parse(argv):
    return cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args(argv)


@pytest.mark.parametrize("policy", ["quality", "speed"])
def test_fp8_flag_selects_fp8_config(policy):
    a = parse(["--prompt", "x", "--fp8", policy, "--height", "896", "--width", "896"])
    assert a.fp8 == policy
    r = cli.resolve(a)
    cfg = r["mmdit_config"]
    assert cfg == fp8_config(MODEL_CONFIG[FLUX], policy)
    assert cfg.weight_dtype == "fp8_e4m3"
    assert cfg.fp8_bf16_double_blocks == (min(FLUX_FP8_QUALITY_BLOCKS, cfg.depth_multimodal) if policy == "quality" else 0)
    assert (r["height"], r["width"]) == (896, 896)  # 3136 image tokens: no multiple of 128, accepted by the fp8 engine


def test_without_the_flag_nothing_changes():
    a = parse(["--prompt", "a cat"])
    assert a.fp8 is None
    assert cli.resolve(a) == {"cfg": 0.0, "shift": 1.0, "height": 512, "width": 512, "flux": True, "low_memory_mode": True}


def test_fp8_flag_rejects_other_values_and_sd3():
    with pytest.raises(SystemExit):
        parse(["--prompt", "x", "--fp8", "fast"])
    with pytest.raises(SystemExit):
        parse(["--prompt", "x", "--fp8"])
    with pytest.raises(ValueError, match="head_dim 128"):
        cli.resolve(parse(["--prompt", "x", "--model-version", "argmaxinc/mlx-stable-diffusion-3-medium", "--fp8", "speed"]))


def test_fp8_flag_is_documented_in_help():
    assert "--fp8" in cli.build_parser(tuple(MMDIT_CKPT.keys())).format_help()


@pytest.mark.gpu
def test_cli_fp8_end_to_end_tiny_ragged_size(dev, tmp_path):
    """the whole command with --fp8 on a tiny FLUX-shaped config at 128 x 192 pixels: 96 image tokens, less than one MX scale block (text length 128);
    both policies run, and the fp8 image differs from the bf16 one (the flag reached the engine) while staying close to it"""
    over = dict(mmdit_config=tiny_flux(), vae_config=tiny_vae(), text_len=128)
    argv = ["--prompt", "a cat", "--steps", "2", "--seed", "7", "--height", "128", "--width", "192"]
    img_bf16, _ = cli.main(argv + ["-o", str(tmp_path / "b.png")], pipeline_overrides=over)
    ref = np.asarray(img_bf16).astype(np.float64)
    for policy in ("quality", "speed"):
        out = tmp_path / f"{policy}.png"
        img, log = cli.main(argv + ["--fp8", policy, "-o", str(out)], pipeline_overrides=over)
        assert out.exists() and img.size == (192, 128) and len(log["denoising"]["iter_time"]) == 2
        got = np.asarray(img).astype(np.float64)
        rmse = float(np.sqrt(np.mean((got - ref) ** 2)))
        print(f"[cli --fp8 {policy}] uint8 image against the bf16 run: rmse {rmse:.3f} of 255")
        if policy == "speed":
            assert not np.array_equal(got, ref), "--fp8 did not reach the engine"
        assert rmse < 255 * 10 ** (-25 / 20)  # 25 dB on the uint8 image: far below the 35 dB of the engine gates, far above a broken path
