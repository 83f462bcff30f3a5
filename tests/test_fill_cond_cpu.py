"""Channel-concatenated conditioning (FLUX.1 Fill / Canny / Depth) without a GPU: the layout statement against its index formula, the
concat-Linear against its split form, the configuration presets, the synthetic and checkpoint weights, the boundary (header, export table,
ctypes table, workspace rule, what the setter refuses), the CLI flags and the pipeline's refusals."""
import re

import numpy as np
import pytest
import torch

from diffusionkit_amd import _lib, cli
from diffusionkit_amd.config import FLUX_CONTROL_DEV, FLUX_DEV, FLUX_FILL_DEV, MMDIT_CKPT, tiny_flux, tiny_sd3
from diffusionkit_amd.weights import mmdit_weight_shapes, synth_mmdit_weights
from oracle.mmdit import OracleMMDiT, Prec
from tests import _fillcond as fc
from tests._util import BF, randn, rel_l2
from tests.test_abi_and_host import _mmdit_handle

NEW_NAMES = ("dk_mmdit_set_condition_width", "dk_mmdit_cache_condition", "dk_image_mask_out_f32", "dk_fill_condition_tokens")
SHAPE = (2, 8, 12, 20, 3)


# ---- the layout ------------------------------------------------------------------------------------------------------------------------
def test_reshape_statement_equals_the_index_formula():
    n, Hl, Wl, C = 2, 4, 6, 16
    z = randn(n, Hl, Wl, C, seed=1)
    mask = fc.make_mask(n, 8 * Hl, 8 * Wl, seed=2)
    vals = set(np.unique(mask.numpy()).tolist())
    assert {0, 255} <= vals and len(vals) > 10, "the mask must carry 0, 255 and in-between bytes"
    tok = fc.condition_tokens_reference(z, mask)
    assert tok.shape == (n, (Hl // 2) * (Wl // 2), 64 + 256) and tok.dtype == BF
    gw = Wl // 2
    want = torch.empty(tok.shape, dtype=torch.float32)
    for b in range(n):
        for i in range(Hl // 2):
            for j in range(gw):
                t = i * gw + j
                for c in range(C):
                    for ph in range(2):
                        for pw in range(2):
                            want[b, t, 4 * c + 2 * ph + pw] = z[b, 2 * i + ph, 2 * j + pw, c]
                for py in range(8):
                    for px in range(8):
                        for ph in range(2):
                            for pw in range(2):
                                col, v = fc.mask_column_formula(mask[b].numpy(), i, j, py, px, ph, pw)
                                want[b, t, col] = float(v)
    assert torch.equal(tok, want.to(BF))
    # one shared mask is broadcast; no mask: the latent columns alone (control)
    one = fc.condition_tokens_reference(z, mask[:1])
    assert torch.equal(one[0], tok[0]) and torch.equal(one[1, :, 64:], tok[0, :, 64:]) and torch.equal(one[1, :, :64], tok[1, :, :64])
    assert torch.equal(fc.condition_tokens_reference(z), tok[..., :64])
    # and the two wrong layouts of the effect test are wrong
    assert not torch.equal(fc.tokens_mask_phpwc(z, mask), tok) and torch.equal(fc.tokens_mask_phpwc(z, mask)[..., :64], tok[..., :64])
    assert torch.equal(fc.tokens_halves_swapped(z, mask)[..., :256], tok[..., 64:])


def test_latent_columns_are_the_oracle_patchify():
    """the (c, ph, pw) order is the base oracle's own ``patchify_via_reshape`` order: with zeroed condition columns the model is the base model"""
    cfg, base = tiny_flux(condition_features=320), tiny_flux()
    wf = {k: v.float() for k, v in fc.weights(320).items()}
    wf["x_embedder.proj.weight"] = wf["x_embedder.proj.weight"].clone()
    wf["x_embedder.proj.weight"][..., 64:] = 0
    w0 = dict(wf)
    w0["x_embedder.proj.weight"] = wf["x_embedder.proj.weight"][..., :64].contiguous()
    text, pooled, lat, z, mask = fc.case_inputs(cfg, "A1", 320)
    outs = []
    for m, kw in ((fc.FillCondMMDiT(cfg, wf, Prec()), {"cond": fc.condition_tokens_reference(z, mask).float()}), (OracleMMDiT(base, w0, Prec()), {})):
        m.cache_modulation_params(pooled, torch.tensor(fc.TIMESTEPS))
        outs.append(m(lat, text, fc.TIMESTEPS[1], **kw))
    assert torch.equal(outs[0], outs[1])


def test_concat_linear_equals_the_split_form():
    g = torch.Generator().manual_seed(0)
    t, c = torch.randn(3, 24, 64, generator=g, dtype=torch.float64), torch.randn(3, 24, 320, generator=g, dtype=torch.float64)
    w, b = torch.randn(256, 384, generator=g, dtype=torch.float64), torch.randn(256, generator=g, dtype=torch.float64)
    whole = torch.cat([t, c], -1) @ w.t() + b
    split = (t @ w[:, :64].t() + b) + c @ w[:, 64:].t()
    assert rel_l2(whole, split) < 1e-14


def test_emulating_oracle_rounds_the_condition_share():
    """fp32: the concat-Linear; emu: bf16(bf16(latent share + bias) + bf16(condition share))"""
    cfg = tiny_flux(condition_features=64)
    wf = {k: v.float() for k, v in fc.weights(64).items()}
    _, _, lat, z, _ = fc.case_inputs(cfg, "A1", 64)
    cond = fc.condition_tokens_reference(z).float()
    w = wf["x_embedder.proj.weight"].reshape(cfg.hidden_size, -1)
    b = wf["x_embedder.proj.bias"]
    t = fc.patchify(lat)
    m32, me = fc.FillCondMMDiT(cfg, wf, Prec()), fc.FillCondMMDiT(cfg, wf, Prec(BF))
    m32.cond = me.cond = cond
    assert torch.equal(m32._patch_embed(lat), torch.cat([t, cond], -1) @ w.t() + b)
    r = lambda x: x.to(BF).float()
    assert torch.equal(me._patch_embed(lat), r(r(t @ w[:, :64].t() + b) + r(cond @ w[:, 64:].t())))


# ---- configuration and weights ---------------------------------------------------------------------------------------------------------
def test_presets():
    from dataclasses import replace
    assert FLUX_DEV.condition_features == 0 and tiny_flux().condition_features == 0
    assert FLUX_FILL_DEV == replace(FLUX_DEV, condition_features=320) and FLUX_CONTROL_DEV == replace(FLUX_DEV, condition_features=64)
    assert tiny_flux(condition_features=320) == replace(tiny_flux(), condition_features=320)
    from diffusionkit_amd.config import validate_condition_features
    validate_condition_features(FLUX_FILL_DEV)
    for bad in (replace(tiny_flux(), condition_features=100), replace(tiny_flux(), condition_features=-64), replace(tiny_sd3(), condition_features=64)):
        with pytest.raises(ValueError, match="condition_features"):
            validate_condition_features(bad)


def test_synthetic_weights():
    base = synth_mmdit_weights(tiny_flux(), seed=1234)
    again = synth_mmdit_weights(tiny_flux(condition_features=0), seed=1234)
    assert list(base) == list(again) and all(torch.equal(base[k], again[k]) for k in base)  # (width 0: today's tensors)
    assert tuple(base["x_embedder.proj.weight"].shape) == (256, 1, 1, 64)
    for width in (64, 320):
        cfg = tiny_flux(condition_features=width)
        wide = synth_mmdit_weights(cfg, seed=1234)
        assert tuple(wide["x_embedder.proj.weight"].shape) == (256, 1, 1, 64 + width)
        assert mmdit_weight_shapes(cfg)["x_embedder.proj.weight"] == (256, 1, 1, 64 + width)
        assert {k: tuple(v.shape) for k, v in wide.items() if k != "x_embedder.proj.weight"} == \
               {k: tuple(v.shape) for k, v in base.items() if k != "x_embedder.proj.weight"}


def _flux_state_dict(cfg, width):
    """a BFL-layout FLUX state dict for ``cfg``'s geometry with an img_in of 64 + ``width`` columns (zeros: only keys and shapes are read)"""
    h, r, T, P = cfg.hidden_size, cfg.mlp_ratio, cfg.token_level_text_embed_dim, cfg.pooled_text_embed_dim
    D = cfg.head_dim
    sd = {}

    def lin(name, o, i):
        sd[name + ".weight"], sd[name + ".bias"] = torch.zeros(o, i, dtype=BF), torch.zeros(o, dtype=BF)

    lin("img_in", h, 64 + width)
    lin("txt_in", h, T)
    lin("time_in.in_layer", h, cfg.frequency_embed_dim)
    lin("time_in.out_layer", h, h)
    lin("vector_in.in_layer", h, P)
    lin("vector_in.out_layer", h, h)
    lin("final_layer.linear", 64, h)
    lin("final_layer.adaLN_modulation.1", 2 * h, h)
    for i in range(cfg.depth_multimodal):
        for s in ("img", "txt"):
            b = f"double_blocks.{i}.{s}"
            lin(f"{b}_mod.lin", 6 * h, h)
            lin(f"{b}_attn.qkv", 3 * h, h)
            lin(f"{b}_attn.proj", h, h)
            lin(f"{b}_mlp.0", r * h, h)
            lin(f"{b}_mlp.2", h, r * h)
            sd[f"{b}_attn.norm.query_norm.scale"] = torch.zeros(D, dtype=BF)
            sd[f"{b}_attn.norm.key_norm.scale"] = torch.zeros(D, dtype=BF)
    for i in range(cfg.depth_unified):
        b = f"single_blocks.{i}"
        lin(f"{b}.modulation.lin", 3 * h, h)
        lin(f"{b}.linear1", (3 + r) * h, h)
        lin(f"{b}.linear2", h, (1 + r) * h)
        sd[f"{b}.norm.query_norm.scale"] = torch.zeros(D, dtype=BF)
        sd[f"{b}.norm.key_norm.scale"] = torch.zeros(D, dtype=BF)
    return sd


def test_model_io_accepts_and_refuses_by_width():
    from diffusionkit_amd.model_io import CheckpointError, load_mmdit_checkpoint
    for width in (0, 64, 320):
        cfg = tiny_flux(condition_features=width)
        named = load_mmdit_checkpoint(_flux_state_dict(cfg, width), cfg)
        assert tuple(named["x_embedder.proj.weight"].shape) == (cfg.hidden_size, 1, 1, 64 + width)
    for have, want in ((320, 0), (0, 320), (64, 320)):
        with pytest.raises(CheckpointError) as e:
            load_mmdit_checkpoint(_flux_state_dict(tiny_flux(), have), tiny_flux(condition_features=want))
        msg = str(e.value)
        assert "img_in.weight" in msg and f"condition width of {have}" in msg and f"condition_features is {want}" in msg, msg


# ---- the boundary ------------------------------------------------------------------------------------------------------------------------
def test_new_names_in_header_export_table_and_ctypes_table():
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    declared = set(re.findall(r"\b(dk_[a-z0-9_]+)\s*\(", src))
    lib = _lib.load()
    for name in NEW_NAMES:
        assert name in declared, f"{name} is not declared in include/dk_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in _lib.SIGNATURES, f"{name} is missing from the ctypes table"
    assert lib.dk_abi_version() == 5  # (additive)


def test_workspace_grows_by_the_condition_share_only():
    """off: the bytes of a handle that never heard of the option; on: one [B, S_i, h] bf16 buffer more (256-byte carve granularity); off again:
    the first number"""
    lib = _lib.load()
    cfg = tiny_flux()
    h, fresh = _mmdit_handle(lib, cfg), _mmdit_handle(lib, cfg)
    try:
        base = lib.dk_mmdit_workspace_bytes(fresh, *SHAPE)
        assert lib.dk_mmdit_set_condition_width(h, 0) == 0
        assert lib.dk_mmdit_workspace_bytes(h, *SHAPE) == base
        for width in (64, 320):
            assert lib.dk_mmdit_set_condition_width(h, width) == 0, lib.dk_last_error()
            conde = SHAPE[0] * 24 * cfg.hidden_size * 2
            assert conde <= lib.dk_mmdit_workspace_bytes(h, *SHAPE) - base < conde + 256
        assert lib.dk_mmdit_set_condition_width(h, 0) == 0
        assert lib.dk_mmdit_workspace_bytes(h, *SHAPE) == base
    finally:
        lib.dk_mmdit_destroy(h)
        lib.dk_mmdit_destroy(fresh)


def test_setter_refuses_and_changes_nothing():
    lib = _lib.load()
    h = _mmdit_handle(lib, tiny_sd3())
    try:
        base = lib.dk_mmdit_workspace_bytes(h, 2, 8, 12, 20, 3)
        assert lib.dk_mmdit_set_condition_width(h, 64) != 0
        assert b"use_pos_embed" in lib.dk_last_error()
        assert lib.dk_mmdit_workspace_bytes(h, 2, 8, 12, 20, 3) == base
        assert lib.dk_mmdit_set_condition_width(h, 0) == 0  # (off is always accepted)
    finally:
        lib.dk_mmdit_destroy(h)
    h = _mmdit_handle(lib, tiny_flux())
    try:
        base = lib.dk_mmdit_workspace_bytes(h, *SHAPE)
        for bad in (-64, 1, 100, 63, 65):
            assert lib.dk_mmdit_set_condition_width(h, bad) != 0, bad
            assert b"multiple of 64" in lib.dk_last_error()
            assert lib.dk_mmdit_workspace_bytes(h, *SHAPE) == base, bad
        # a reference grid and a condition width exclude each other, whichever comes first; a refused call leaves the accepted state in place
        assert lib.dk_mmdit_set_reference_grid(h, 6, 10) == 0
        with_ref = lib.dk_mmdit_workspace_bytes(h, *SHAPE)
        assert lib.dk_mmdit_set_condition_width(h, 320) != 0 and b"reference grid" in lib.dk_last_error()
        assert lib.dk_mmdit_workspace_bytes(h, *SHAPE) == with_ref
        assert lib.dk_mmdit_set_reference_grid(h, 0, 0) == 0
        assert lib.dk_mmdit_set_condition_width(h, 320) == 0
        on = lib.dk_mmdit_workspace_bytes(h, *SHAPE)
        assert lib.dk_mmdit_set_reference_grid(h, 6, 10) != 0 and b"condition width" in lib.dk_last_error()
        assert lib.dk_mmdit_set_condition_width(h, 100) != 0
        assert lib.dk_mmdit_workspace_bytes(h, *SHAPE) == on
    finally:
        lib.dk_mmdit_destroy(h)


def test_entries_refuse_an_unprepared_engine():
    import ctypes
    lib = _lib.load()
    h = _mmdit_handle(lib, tiny_flux())
    try:
        assert lib.dk_mmdit_set_condition_width(h, 320) == 0
        assert lib.dk_mmdit_cache_condition(h, ctypes.c_void_p(256), 0, None) != 0
        assert b"prepare" in lib.dk_last_error()
    finally:
        lib.dk_mmdit_destroy(h)


def test_operator_entries_refuse_bad_arguments():
    import ctypes
    lib = _lib.load()
    p = ctypes.c_void_p(256)  # (never dereferenced: every call below is refused before its launch)
    assert lib.dk_image_mask_out_f32(p, p, p, 2, 3, 16, 16, None) != 0 and b"n_mask" in lib.dk_last_error()
    assert lib.dk_image_mask_out_f32(p, None, p, 2, 1, 16, 16, None) != 0
    assert lib.dk_fill_condition_tokens(p, p, p, 2, 3, 4, 4, 16, 2, None) != 0 and b"n_mask" in lib.dk_last_error()
    assert lib.dk_fill_condition_tokens(p, None, p, 1, 0, 3, 4, 16, 2, None) != 0 and b"patch size" in lib.dk_last_error()
    assert lib.dk_fill_condition_tokens(None, None, p, 1, 0, 4, 4, 16, 2, None) != 0


# ---- CLI and pipeline --------------------------------------------------------------------------------------------------------------------
def _args(*extra):
    return cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args(["--prompt", "a cat", *extra])


FLUX = next(v for v in MMDIT_CKPT if "FLUX" in v)
SD3 = next(v for v in MMDIT_CKPT if "FLUX" not in v)


def test_cli_flags():
    r = cli.resolve(_args("--model-version", FLUX))
    assert not {"condition", "condition_image_path", "condition_mask_path"} & set(r)  # (keys only when the flags are given)
    r = cli.resolve(_args("--model-version", FLUX, "--condition", "fill", "--condition-image-path", "a.png", "--condition-mask-path", "m.png"))
    assert (r["condition"], r["condition_image_path"], r["condition_mask_path"]) == ("fill", "a.png", "m.png")
    r = cli.resolve(_args("--model-version", FLUX, "--condition", "control", "--condition-image-path", "edges.png"))
    assert (r["condition"], r["condition_image_path"]) == ("control", "edges.png") and "condition_mask_path" not in r
    with pytest.raises(SystemExit):
        _args("--condition", "redux")
    for flags, match in (
            (("--model-version", SD3, "--condition", "fill", "--condition-image-path", "a.png", "--condition-mask-path", "m.png"), "FLUX"),
            (("--model-version", FLUX, "--condition-image-path", "a.png"), "condition='fill' or condition='control'"),
            (("--model-version", FLUX, "--condition", "fill"), "condition_image_path"),
            (("--model-version", FLUX, "--condition", "fill", "--condition-image-path", "a.png"), "condition_mask_path"),
            (("--model-version", FLUX, "--condition", "control", "--condition-image-path", "a.png", "--condition-mask-path", "m.png"), "no condition_mask_path"),
            (("--model-version", FLUX, "--condition", "control", "--condition-image-path", "a.png", "--reference-image-path", "r.png"), "reference_image_path")):
        with pytest.raises(ValueError, match=match):
            cli.resolve(_args(*flags))


def _bare(cls, condition=None):
    p = object.__new__(cls)  # (the checks under test run before anything else of the pipeline's state is read)
    p.condition = condition
    return p


def test_pipeline_refusals():
    from diffusionkit_amd.pipeline import DiffusionPipeline, FluxPipeline
    img, mask = np.zeros((64, 96, 3), dtype=np.uint8), np.zeros((64, 96), dtype=np.uint8)
    for method in ("denoise_latents", "generate_image"):
        call = lambda pipe, **kw: getattr(pipe, method)(None, None, latent_size=(8, 12), seed=0, **kw) if method == "denoise_latents" else \
            getattr(pipe, method)("a cat", latent_size=(8, 12), seed=0, **kw)
        with pytest.raises(ValueError, match="FLUX-family"):
            call(_bare(DiffusionPipeline), condition_image_path=img)
        with pytest.raises(ValueError, match="condition='fill' or condition='control'"):
            call(_bare(FluxPipeline), condition_image_path=img, condition_mask_path=mask)
        with pytest.raises(ValueError, match="needs condition_image_path in every call"):
            call(_bare(FluxPipeline, "fill"))
        with pytest.raises(ValueError, match="needs condition_mask_path"):
            call(_bare(FluxPipeline, "fill"), condition_image_path=img)
        with pytest.raises(ValueError, match="takes no condition_mask_path"):
            call(_bare(FluxPipeline, "control"), condition_image_path=img, condition_mask_path=mask)
        with pytest.raises(ValueError, match="cannot be combined"):
            call(_bare(FluxPipeline, "control"), condition_image_path=img, reference_image_path=img)
    # the constructor refuses the SD3 family and an unknown name before it loads anything
    with pytest.raises(ValueError, match="FLUX-family"):
        DiffusionPipeline(w16=True, a16=True, condition="fill")
    with pytest.raises(ValueError, match="unknown condition"):
        FluxPipeline(w16=True, a16=True, condition="redux")
    # sizes: the output's, never resized; a list holds one entry per seed
    dl = lambda pipe, **kw: pipe.denoise_latents(None, None, latent_size=(8, 12), seed=[0, 1], **kw)
    with pytest.raises(ValueError, match="not resized"):
        dl(_bare(FluxPipeline, "control"), condition_image_path=np.zeros((64, 64, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="not resized"):
        dl(_bare(FluxPipeline, "fill"), condition_image_path=img, condition_mask_path=np.zeros((32, 48), dtype=np.uint8))
    with pytest.raises(ValueError, match="one per image"):
        dl(_bare(FluxPipeline, "control"), condition_image_path=[img])


def test_read_condition_images():
    from PIL import Image
    from diffusionkit_amd.pipeline import read_condition_images
    img = np.arange(64 * 96 * 3, dtype=np.uint32).reshape(64, 96, 3).astype(np.uint8)
    mask = fc.make_mask(1, 64, 96)[0].numpy()
    px, m = read_condition_images(img, mask, (64, 96), 2)
    assert px.shape == (1, 64, 96, 3) and m.shape == (1, 64, 96) and np.array_equal(px[0], img) and np.array_equal(m[0], mask)  # (in-between bytes kept)
    px, m = read_condition_images([img, Image.fromarray(img)], [mask, Image.fromarray(mask)], (64, 96), 2)
    assert px.shape == (2, 64, 96, 3) and np.array_equal(px[1], img) and np.array_equal(m[1], mask)
    px, m = read_condition_images(Image.fromarray(img[:, :, 0]), None, (64, 96), 1)
    assert px.shape == (1, 64, 96, 3) and m is None


def test_dist_slices_the_list_form():
    from diffusionkit_amd import dist

    class Pipe:
        def generate_image(self, text, **kw):
            return kw

    seeds, images, masks = [10, 11, 12, 13, 14], list("abcde"), list("vwxyz")
    kw = dist.generate_sharded(Pipe(), "x", seeds, 1, 2, condition_image_path=images, condition_mask_path=masks, num_steps=2)
    assert kw == {"seed": [12, 13, 14], "condition_image_path": ["c", "d", "e"], "condition_mask_path": ["x", "y", "z"], "num_steps": 2}
    kw = dist.generate_sharded(Pipe(), "x", seeds, 0, 2, condition_image_path="one.png")
    assert kw == {"seed": [10, 11], "condition_image_path": "one.png"}  # (keys only when set; one image for all is passed through)


def test_pipeline_keywords_are_keyword_only():
    import inspect
    from diffusionkit_amd.pipeline import DiffusionPipeline
    for fn in (DiffusionPipeline.denoise_latents, DiffusionPipeline.generate_image):
        for name in ("condition_image_path", "condition_mask_path"):
            p = inspect.signature(fn).parameters[name]
            assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


def test_effect_inputs_discriminate():
    """the conditions the GPU effect test leans on, on the oracle alone, with the figures its docstring quotes: the condition moves the output by
    far more than 5 % of its norm, the bf16-emulating oracle reproduces that effect to <= 0.2, and both wrong layouts miss the bound"""
    name, width = "A1", 320
    r = fc.oracle_case(name, width)
    f, e = r["fp32"][fc.STEP], r["emu"][fc.STEP]
    d32, de = f["final"] - f["final0"], e["final"] - e["final0"]
    e_e = rel_l2(d32, de)
    assert float(d32.norm() / f["final"].norm()) >= 0.05 and e_e <= 0.2
    for fn in (fc.tokens_mask_phpwc, fc.tokens_halves_swapped):
        w = fc.oracle_case(name, width, tokens_fn=fn)["fp32"][fc.STEP]
        assert rel_l2(d32, w["final"] - w["final0"]) > 5 * (2.0 * e_e + 0.02), fn.__name__
