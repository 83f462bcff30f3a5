"""The tiny latent decoder behind the public interface: ``generate_image(decoder="tiny")``, per-step previews that leave the loop's bits alone, the
refusals by name, and one CLI call that writes its preview files."""
import numpy as np
import pytest
import torch

from diffusionkit_amd import cli, dist
from diffusionkit_amd.config import tiny_flux, tiny_sd3, tiny_vae
from diffusionkit_amd.pipeline import DiffusionPipeline, FluxPipeline
from tests import _engine_state as es

pytestmark = pytest.mark.gpu
STEPS, SIZE = 3, (4, 6)


@pytest.fixture(scope="module", params=["flux", "sd3"])
def pipe(request, dev):
    cls, cfg, w = (FluxPipeline, tiny_flux(), 0.0) if request.param == "flux" else (DiffusionPipeline, tiny_sd3(), 4.0)
    p = cls(w16=True, a16=True, mmdit_config=cfg, vae_config=tiny_vae(), device=dev, text_len=16, tiny_decoder_ckpt="synthetic")
    p.test_cfg = w
    return p


def test_tiny_decode_and_previews(pipe):
    kw = dict(num_steps=STEPS, cfg_weight=pipe.test_cfg, latent_size=SIZE, seed=3)
    cond, pooled = pipe.encode_text("a cat", pipe.test_cfg, "")
    lat, _ = pipe.denoise_latents(cond, pooled, **kw)
    seen = []
    lat_pv, times = pipe.denoise_latents(cond, pooled, preview_every=1, preview_callback=lambda i, u8: seen.append((i, u8.clone())), **kw)
    es.assert_identical({"without previews": lat, "with previews": lat_pv}, "denoise_latents")
    assert [i for i, _ in seen] == list(range(STEPS)) and len(times) == STEPS
    assert all(u.dtype == torch.uint8 and tuple(u.shape) == (1, 8 * SIZE[0], 8 * SIZE[1], 3) for _, u in seen)
    assert not torch.equal(seen[0][1], seen[-1][1])  # (an estimate per step, not one image)
    img, log = pipe.generate_image("a cat", decoder="tiny", verbose=False, **kw)
    want = pipe.tiny_decoder.decode(lat)[1]
    assert img.size == (8 * SIZE[1], 8 * SIZE[0]) and log["decoding"]["decoder"] == "tiny"
    assert np.array_equal(np.asarray(img), want[0].cpu().numpy())
    vae_img, vae_log = pipe.generate_image("a cat", verbose=False, **kw)  # the default: the VAE's image, no new key
    assert np.array_equal(np.asarray(vae_img), pipe.decoder.decode(lat)[1][0].cpu().numpy()) and "decoder" not in vae_log["decoding"]


def test_refusals(pipe):
    kw = dict(num_steps=1, latent_size=SIZE, seed=3, verbose=False)
    px, mask = np.zeros((8 * SIZE[0], 8 * SIZE[1], 3), np.uint8), np.zeros((8 * SIZE[0], 8 * SIZE[1]), np.uint8)
    with pytest.raises(ValueError, match="composite"):
        pipe.generate_image("a", decoder="tiny", image_path=px, mask_path=mask, **kw)
    with pytest.raises(ValueError, match="both preview_every"):
        pipe.generate_image("a", preview_every=1, **kw)
    with pytest.raises(ValueError, match="edit"):
        pipe.generate_image("a", image_path=px, edit_source_text="b", preview_every=1, preview_callback=print, **kw)
    with pytest.raises(ValueError, match="unknown decoder"):
        pipe.generate_image("a", decoder="taesd", **kw)
    for extra in (dict(decoder="tiny"), dict(preview_every=1, preview_callback=print)):
        with pytest.raises(ValueError, match="multi-GPU sharding"):
            dist.generate_sharded(pipe, "a", [1, 2], 0, 1, **extra)
    keep, pipe.tiny_decoder = pipe.tiny_decoder, None
    try:
        for extra in (dict(decoder="tiny"), dict(preview_every=1, preview_callback=print)):
            with pytest.raises(ValueError, match="tiny_decoder_ckpt"):
                pipe.generate_image("a", **extra, **kw)
    finally:
        pipe.tiny_decoder = keep


def test_cli_writes_previews(tmp_path):
    over = dict(mmdit_config=tiny_flux(), vae_config=tiny_vae(), text_len=16)
    out, pv = tmp_path / "a.png", tmp_path / "pv"
    img, log = cli.main(["--prompt", "a cat", "--steps", "4", "--seed", "7", "--height", "32", "--width", "48", "-o", str(out), "--tiny-decoder",
                         "synthetic", "--decoder", "tiny", "--preview-dir", str(pv), "--preview-every", "2"], pipeline_overrides=over)
    assert out.exists() and img.size == (48, 32) and log["decoding"]["decoder"] == "tiny"
    assert sorted(f.name for f in pv.iterdir()) == ["step_001.png", "step_003.png"]
    assert __import__("PIL.Image").Image.open(pv / "step_003.png").size == (48, 32)
    for argv, text in ((["--decoder", "tiny"], "need --tiny-decoder"), (["--preview-every", "2"], "needs --preview-dir")):
        with pytest.raises(ValueError, match=text):
            cli.main(["--prompt", "a cat", *argv], pipeline_overrides=over)
