"""Tiny latent decoder, host side: the float64 reference against a nested-loop Block, the constants of tests/_tae.py re-measured, the synthetic
weights' range, the checkpoint loader's two key forms and its refusals.  No GPU."""
import pytest
import torch

from diffusionkit_amd import _lib, model_io
from diffusionkit_amd.config import TinyDecoderConfig
from diffusionkit_amd.weights import pack_tae, synth_tae_weights
from tests import _tae as T
from tests._numeric_range import BF, spacing
from tests._util import psnr, randn


def test_reference_block_equals_nested_loops():
    x, ws, bs = T.block_operands((1, 2, 3))
    h = x.double()
    for j in range(3):
        o = torch.zeros(1, 2, 3, 64, dtype=torch.float64)
        for y in range(2):
            for xx in range(3):
                for ky in range(3):
                    for kx in range(3):
                        sy, sx = y + ky - 1, xx + kx - 1
                        if 0 <= sy < 2 and 0 <= sx < 3:
                            o[0, y, xx] += ws[j][:, ky, kx].double() @ h[0, sy, sx]
        o = o + bs[j].double() + (x.double() if j == 2 else 0.0)
        h = T.rb(torch.relu(o))
    assert torch.equal(h, T.block(x, ws, bs, True))


def test_measured_constants():
    worst = 0.0
    for g in T.BLOCK_GRIDS:
        x, ws, bs = T.block_operands(g)
        r = (T.block(x, ws, bs, True, dt=torch.float32).double() - T.block(x, ws, bs, True)).abs() / T.block_unit(x, ws, bs)
        worst = max(worst, float(r.max()))
    print(f"block: worst |fp32 restatement - ref64| / unit = {worst:.3g}")
    assert worst <= T.C_BLOCK / 2 * 1.0001 and T.C_BLOCK <= 1e-2
    # the padding fault moves the border by more than ten gates on the all-positive case
    x, ws, bs = T.block_operands((1, 5, 7), positive=True)
    a, b = T.block(x, ws, bs, True), T.block(x, ws, bs, True, keep_out_of_image=True)
    gate = spacing(a.abs(), BF) + T.C_BLOCK * T.block_unit(x, ws, bs)
    d = (a - b).abs() / gate
    assert min(float(d[:, 0].min()), float(d[:, -1].min()), float(d[:, :, 0].min()), float(d[:, :, -1].min())) > 10.0
    w = {k: v.float() for k, v in synth_tae_weights().items()}
    low = 1e9
    for i in range(len(T.LATENTS)):
        lat = T.latent(i)
        exact, _ = T.decode(lat, w, False)
        assert float(((exact <= 0) | (exact >= 1)).double().mean()) < 0.5, "synthetic weights saturate the image"
        low = min(low, psnr(exact, T.decode(lat, w, True)[0]))
    print(f"decoder: PSNR of the rounding-point reference against the exact one >= {low:.1f} dB")
    assert low - 3.0 >= T.PSNR_MIN


def test_pack_and_abi():
    p = pack_tae(synth_tae_weights(), "cpu")
    assert p["1.weight"].shape == (64, 160) and torch.all(p["1.weight"][:, 144:] == 0)
    assert p["19.weight"].shape == (16, 576) and torch.all(p["19.weight"][3:] == 0) and p["19.bias"].shape == (16,)
    assert p["7.weight"].shape == (64, 576) and "7.bias" not in p and len(p) == 1 * 2 + 10 * 6 + 3 + 2
    lib = _lib.load()
    assert lib.dk_tae_workspace_bytes(1, 128, 128) == 3 * 1024 * 1024 * 64 * 2 and lib.dk_tae_workspace_bytes(0, 1, 1) == 0
    assert lib.dk_tune_set(b"tae_block", -1) == 0
    with pytest.raises(_lib.DkHipError):
        from diffusionkit_amd.engine import TinyDecoderEngine
        TinyDecoderEngine(p)  # CPU tensors: there is no CPU path


def _published(w):
    return {k: (v.permute(0, 3, 1, 2).contiguous() if v.dim() == 4 else v) for k, v in w.items()}


def test_loader_key_forms_and_refusals(tmp_path):
    from safetensors.torch import save_file
    w = synth_tae_weights(seed=7)
    pub = _published(w)
    save_file(pub, str(tmp_path / "taef1_decoder.safetensors"))
    save_file({"decoder.layers." + k: v for k, v in pub.items()}, str(tmp_path / "diffusers.safetensors"))
    for name in ("taef1_decoder.safetensors", "diffusers.safetensors"):
        got = model_io.taesd_checkpoint_to_reference(str(tmp_path / name))
        assert set(got) == set(TinyDecoderConfig().tensor_shapes()) and all(torch.equal(got[k], w[k]) for k in w)
    with pytest.raises(ValueError, match="4 latent channels, not 16"):
        model_io.taesd_checkpoint_to_reference({**pub, "1.weight": pub["1.weight"][:, :4].contiguous()})
    with pytest.raises(ValueError, match="encoder"):
        model_io.taesd_checkpoint_to_reference({**{"decoder.layers." + k: v for k, v in pub.items()}, "encoder.layers.0.weight": pub["1.weight"]})
    with pytest.raises(ValueError, match="missing"):
        model_io.taesd_checkpoint_to_reference({k: v for k, v in pub.items() if not k.startswith("18.")})
