"""Reference-image conditioning without a GPU: the new names in the header, the library's export table and the ctypes table, the workspace
rule (off: today's bytes), what the setter refuses, the oracle's table helper, and the pipeline / CLI / sharding validation."""
import re

import numpy as np
import pytest
import torch

from diffusionkit_amd import _lib, cli, dist
from diffusionkit_amd.config import MMDIT_CKPT, tiny_flux, tiny_sd3
from oracle.mmdit import OracleMMDiT, Prec, rope_table
from tests import _refcond as rc
from tests._util import randn
from tests.test_abi_and_host import _mmdit_handle

NEW_NAMES = ("dk_mmdit_set_reference_grid", "dk_mmdit_cache_reference", "dk_rope_table_segments_f32")
SHAPE = (1, 8, 8, 16, 3)


# ---- the boundary ------------------------------------------------------------------------------------------------------------------
def test_new_names_in_header_export_table_and_ctypes_table():
    src = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    declared = set(re.findall(r"\b(dk_[a-z0-9_]+)\s*\(", src))
    lib = _lib.load()
    for name in NEW_NAMES:
        assert name in declared, f"{name} is not declared in include/dk_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in _lib.SIGNATURES, f"{name} is missing from the ctypes table"
    assert lib.dk_abi_version() == 5  # (additive)


# ---- the workspace and the setter ----------------------------------------------------------------------------------------------------
def test_workspace_grows_only_with_a_reference_grid():
    """off: the bytes of a handle that never heard of the option; on: at least the longer joint buffers more; off again: the first number"""
    lib = _lib.load()
    cfg = tiny_flux()
    h, fresh = _mmdit_handle(lib, cfg), _mmdit_handle(lib, cfg)
    try:
        base = lib.dk_mmdit_workspace_bytes(fresh, *SHAPE)
        assert lib.dk_mmdit_set_reference_grid(h, 0, 0) == 0
        assert lib.dk_mmdit_workspace_bytes(h, *SHAPE) == base
        assert lib.dk_mmdit_set_reference_grid(h, 6, 10) == 0, lib.dk_last_error()
        on = lib.dk_mmdit_workspace_bytes(h, *SHAPE)
        S_r, hid = 15, cfg.hidden_size
        # X, XN, ATT (h each), QKV (3h) and the embedded reference itself (h) gain S_r rows of 2-byte elements, at the least
        assert on - base >= S_r * hid * 2 * 7, (base, on)
        assert lib.dk_mmdit_set_reference_grid(h, 0, 0) == 0
        assert lib.dk_mmdit_workspace_bytes(h, *SHAPE) == base
    finally:
        lib.dk_mmdit_destroy(h)
        lib.dk_mmdit_destroy(fresh)


def test_setter_refuses_and_changes_nothing():
    lib = _lib.load()
    h = _mmdit_handle(lib, tiny_sd3())
    try:
        base = lib.dk_mmdit_workspace_bytes(h, 2, 8, 12, 20, 3)
        assert lib.dk_mmdit_set_reference_grid(h, 6, 10) != 0
        assert b"RoPE" in lib.dk_last_error()
        assert lib.dk_mmdit_workspace_bytes(h, 2, 8, 12, 20, 3) == base
        assert lib.dk_mmdit_set_reference_grid(h, 0, 0) == 0  # (off is always accepted)
    finally:
        lib.dk_mmdit_destroy(h)
    h = _mmdit_handle(lib, tiny_flux())
    try:
        base = lib.dk_mmdit_workspace_bytes(h, *SHAPE)
        for bad in ((5, 10), (6, 9), (0, 10), (6, 0), (-2, 4), (4, -2)):  # odd sides, one side zero, negative sides
            assert lib.dk_mmdit_set_reference_grid(h, *bad) != 0, bad
            assert b"patch size" in lib.dk_last_error()
            assert lib.dk_mmdit_workspace_bytes(h, *SHAPE) == base, bad
        # a refused call leaves an accepted grid in place
        assert lib.dk_mmdit_set_reference_grid(h, 6, 10) == 0
        on = lib.dk_mmdit_workspace_bytes(h, *SHAPE)
        assert lib.dk_mmdit_set_reference_grid(h, 5, 10) != 0
        assert lib.dk_mmdit_workspace_bytes(h, *SHAPE) == on
    finally:
        lib.dk_mmdit_destroy(h)


def test_entries_refuse_an_unprepared_engine():
    import ctypes
    lib = _lib.load()
    h = _mmdit_handle(lib, tiny_flux())
    try:
        assert lib.dk_mmdit_set_reference_grid(h, 6, 10) == 0
        assert lib.dk_mmdit_cache_reference(h, ctypes.c_void_p(256), 0, None) != 0
        assert b"prepare" in lib.dk_last_error()
    finally:
        lib.dk_mmdit_destroy(h)


# ---- the oracle of the layout --------------------------------------------------------------------------------------------------------
def test_extended_table_helper():
    cfg = tiny_flux()
    S_t, gh, gw, rh, rw = 20, 4, 6, 3, 5
    ext = rc.rope_table_ext(cfg, S_t, gh, gw, rh, rw)
    assert ext.shape[0] == S_t + gh * gw + rh * rw
    assert torch.equal(ext[:S_t + gh * gw], rope_table(cfg, S_t, gh, gw))
    assert torch.equal(rc.rope_table_ext(cfg, S_t, gh, gw), rope_table(cfg, S_t, gh, gw))
    own = rope_table(cfg, S_t, rh, rw)[S_t:]  # the image rows of a table built for the reference grid
    a0 = cfg.rope_axes_dim[0] // 2
    assert torch.equal(ext[S_t + gh * gw:, a0:], own[:, a0:])
    omega = 1.0 / (float(cfg.rope_theta) ** (torch.arange(0, cfg.rope_axes_dim[0], 2, dtype=torch.float32) / cfg.rope_axes_dim[0]))
    assert torch.equal(ext[S_t + gh * gw:, :a0, 0], torch.cos(omega)[None].expand(rh * rw, -1))
    assert torch.equal(ext[S_t + gh * gw:, :a0, 1], torch.sin(omega)[None].expand(rh * rw, -1))


def test_oracle_without_a_reference_is_the_base_oracle():
    cfg = tiny_flux()
    wf = {k: v.float() for k, v in rc.sharpened_weights(cfg).items()}
    text, pooled, lat, _ = rc.case_inputs(cfg, "A2")
    outs = []
    for cls in (OracleMMDiT, rc.RefCondMMDiT):
        m = cls(cfg, wf, Prec())
        m.cache_modulation_params(pooled, torch.tensor(rc.TIMESTEPS))
        outs.append(m(lat, text, rc.TIMESTEPS[1]))
    assert torch.equal(outs[0], outs[1])


def test_sharpened_inputs_discriminate():
    """the conditions the GPU tests lean on, on the oracle alone: the reference moves the output by >= 5 % of its norm, and the bf16-emulating
    oracle reproduces that effect to <= 0.2 -- far from the 1.0 of an ignored reference"""
    from tests._util import rel_l2
    r = rc.oracle_case("A1")
    f, e = r["fp32"][rc.STEP], r["emu"][rc.STEP]
    d32, de = f["final"] - f["final0"], e["final"] - e["final0"]
    assert float(d32.norm() / f["final"].norm()) >= 0.05
    assert rel_l2(d32, de) <= 0.2


# ---- pipeline, CLI, sharding ---------------------------------------------------------------------------------------------------------
def _bare(cls):
    return object.__new__(cls)  # (the checks under test run before anything of the pipeline's state is read)


def test_pipeline_validation():
    from diffusionkit_amd.pipeline import DiffusionPipeline, FluxPipeline, read_reference_u8
    good = np.zeros((48, 80, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="RoPE"):
        _bare(DiffusionPipeline).denoise_latents(None, None, seed=0, reference_image_path=good)
    for hw in ((48, 81), (40, 80), (8, 16)):
        with pytest.raises(ValueError, match="multiples of 16"):
            _bare(FluxPipeline).denoise_latents(None, None, seed=0, reference_image_path=np.zeros((*hw, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="one per image"):
        _bare(FluxPipeline).denoise_latents(None, None, seed=[0, 1], reference_image_path=[good])
    with pytest.raises(ValueError, match="one size"):
        _bare(FluxPipeline).denoise_latents(None, None, seed=[0, 1], reference_image_path=[good, np.zeros((32, 80, 3), dtype=np.uint8)])
    assert read_reference_u8(good).shape == (48, 80, 3)  # (never resized: read_image_u8 would cut this to 0 x 64)
    from PIL import Image
    assert read_reference_u8(Image.fromarray(good[:, :, 0])).shape == (48, 80, 3)


def test_pipeline_keyword_is_keyword_only():
    import inspect
    from diffusionkit_amd.pipeline import DiffusionPipeline
    for fn in (DiffusionPipeline.denoise_latents, DiffusionPipeline.generate_image):
        p = inspect.signature(fn).parameters["reference_image_path"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


def _args(*extra):
    return cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args(["--prompt", "a cat", *extra])


def test_cli_flag_reaches_resolve():
    assert "reference_image_path" not in cli.resolve(_args())  # (a key only when the flag is given)
    assert cli.resolve(_args("--reference-image-path", "ref.png"))["reference_image_path"] == "ref.png"
    sd3 = next(v for v in MMDIT_CKPT if "FLUX" not in v)
    with pytest.raises(ValueError, match="FLUX"):
        cli.resolve(_args("--model-version", sd3, "--reference-image-path", "ref.png"))


def test_dist_slices_the_list_form():
    refs = ["a", "b", "c", "d", "e"]
    seeds = [10, 11, 12, 13, 14]
    for world in (1, 2, 3):
        got = [dist.shard_per_image(refs, len(seeds), r, world) for r in range(world)]
        assert [len(g) for g in got] == [len(dist.shard_seeds(seeds, r, world)) for r in range(world)]
        assert sum(got, []) == refs
    assert dist.shard_per_image("one.png", 5, 1, 2) == "one.png" and dist.shard_per_image(None, 5, 1, 2) is None
    with pytest.raises(ValueError, match="one per seed"):
        dist.shard_per_image(refs[:2], 5, 0, 2)

    class Pipe:
        def generate_image(self, text, **kw):
            return kw

    kw = dist.generate_sharded(Pipe(), "x", seeds, 1, 2, reference_image_path=refs, num_steps=2)
    assert kw == {"seed": [12, 13, 14], "reference_image_path": ["c", "d", "e"], "num_steps": 2}
    assert dist.generate_sharded(Pipe(), "x", seeds, 0, 2) == {"seed": [10, 11]}  # (keys only when set)
    assert dist.generate_sharded(Pipe(), "x", [7], 0, 2) is None  # (rank 0 of 2 holds no seed of one)
