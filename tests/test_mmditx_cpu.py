"""MMDiT-X (Stable Diffusion 3.5 medium) without a GPU: the oracle of the dual-attention block against the pinned one, the configuration
and the engine's modulation table, the setter's refusals, the workspace, the synthetic weights, the checkpoint loader and the CLI."""
import ctypes
import hashlib
from dataclasses import replace

import pytest
import torch

from diffusionkit_amd import _lib, cli
from diffusionkit_amd.config import (FLUX_SCHNELL, MMDIT_CKPT, MODEL_CONFIG, SD3_2b, SD3_5_MEDIUM, SD3_8b, PositionalEncoding, float16_config,
                                     fp8_config, tiny_flux, tiny_sd3, tiny_sd35m, validate_dual_attention)
from diffusionkit_amd.model_io import CheckpointError, load_mmdit_checkpoint, sd3_checkpoint_to_reference
from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
from oracle.mmdit import OracleMMDiT, Prec
from tests._mmditx import MMDiTXOracle, to_stability_sd3, without_dual
from tests._util import randn

VERSION = "stabilityai/stable-diffusion-3.5-medium"


# ---- oracle ---------------------------------------------------------------------------------------------------------------------------
def _oracle_out(cls, cfg, w, B=2):
    text, pooled, lat = randn(B, 20, cfg.token_level_text_embed_dim, seed=3), randn(B, cfg.pooled_text_embed_dim, seed=4), randn(B, 8, 12, 16, seed=5)
    m = cls(cfg, w, Prec())
    m.cache_modulation_params(pooled, torch.tensor([752.0]))
    return m(lat, text, 752.0)


def test_oracle_equals_the_pinned_oracle_with_the_second_gate_closed():
    """gate_msa2 = 0 takes the second attention out of the sum: MMDiTXOracle must then be OracleMMDiT -- the restatement pinned against the
    reference -- on the same model without it, value for value; with the gate rows back the outputs differ."""
    cfg = tiny_sd35m()
    h = cfg.hidden_size
    w = {k: v.float() for k, v in synth_mmdit_weights(cfg).items()}
    closed = dict(w)
    for i in range(cfg.dual_attention_blocks):
        for leaf in ("weight", "bias"):
            k = f"multimodal_transformer_blocks.{i}.image_transformer_block.adaLN_modulation.layers.1.{leaf}"
            closed[k] = w[k].clone()
            closed[k][8 * h:9 * h] = 0
    cfg0, w0 = without_dual(closed, cfg)
    assert cfg0.dual_attention_blocks == 0 and not any("attn2" in k for k in w0)
    ref = _oracle_out(OracleMMDiT, cfg0, w0)
    got = _oracle_out(MMDiTXOracle, cfg, closed)
    assert bool((got == ref).all())
    assert not torch.equal(_oracle_out(MMDiTXOracle, cfg, w), ref)
    # (and without dual blocks the subclass is the base class)
    assert torch.equal(_oracle_out(MMDiTXOracle, cfg0, w0), ref)


# ---- configuration and the engine's tables --------------------------------------------------------------------------------------------
def make_handle(cfg, fp8=False):
    """a dk_mmdit handle for ``cfg`` as MMDiTEngine fills the descriptor, without weights or a GPU"""
    lib = _lib.load()
    c = _lib.dk_mmdit_config()
    c.num_heads, c.depth_multimodal, c.depth_unified = cfg.num_heads, cfg.depth_multimodal, cfg.depth_unified
    c.hidden_size, c.mlp_ratio, c.vae_latent_dim, c.patch_size = cfg.hidden_size, cfg.mlp_ratio, cfg.vae_latent_dim, cfg.patch_size
    c.use_qk_norm = int(cfg.use_qk_norm)
    c.use_rope = int(cfg.pos_embed_type == PositionalEncoding.PreSDPARope)
    for i, a in enumerate(cfg.rope_axes_dim or ()):
        c.rope_axes_dim[i] = a
    c.n_rope_axes, c.rope_theta = len(cfg.rope_axes_dim or ()), cfg.rope_theta
    c.use_pos_embed = int(cfg.pos_embed_type == PositionalEncoding.LearnedInputEmbedding)
    c.max_latent_resolution = cfg.max_latent_resolution
    c.pooled_text_embed_dim, c.token_level_text_embed_dim = cfg.pooled_text_embed_dim, cfg.token_level_text_embed_dim
    c.frequency_embed_dim, c.max_period, c.layer_norm_eps = cfg.frequency_embed_dim, cfg.max_period, cfg.layer_norm_eps
    c.fp8_linears = int(fp8)
    h = ctypes.c_void_p()
    _lib.check(lib.dk_mmdit_create(ctypes.byref(c), ctypes.byref(h)), "dk_mmdit_create")
    return lib, h


def last_error(lib):
    return lib.dk_last_error().decode()


def check_table(lib, h, cfg):
    assert lib.dk_mmdit_mod_rows(h) == cfg.num_modulation_rows()
    off = 0
    for i in range(cfg.depth_multimodal):
        assert lib.dk_mmdit_mod_offset(h, 0, i) == off
        off += 9 if i < cfg.dual_attention_blocks else 6
        assert lib.dk_mmdit_mod_offset(h, 1, i) == off
        off += 2 if (i == cfg.depth_multimodal - 1 and cfg.depth_unified < 1) else 6
    for i in range(cfg.depth_unified):
        assert lib.dk_mmdit_mod_offset(h, 2, i) == off
        off += 3
    assert lib.dk_mmdit_mod_offset(h, 3, 0) == off and off + 2 == cfg.num_modulation_rows()


@pytest.mark.parametrize("cfg", [tiny_sd35m(), SD3_5_MEDIUM, tiny_sd35m(dual=0), tiny_sd35m(dual=3)], ids=["tiny", "medium", "dual0", "dual_all"])
def test_modulation_table_counts_nine_rows_for_dual_image_modules(cfg):
    lib, h = make_handle(cfg)
    assert lib.dk_mmdit_set_dual_attention(h, cfg.dual_attention_blocks) == 0
    check_table(lib, h, cfg)
    lib.dk_mmdit_destroy(h)


def test_preset_and_config_rules():
    c = SD3_5_MEDIUM
    assert (c.depth_multimodal, c.num_heads, c.hidden_size, c.head_dim, c.use_qk_norm, c.max_latent_resolution, c.dual_attention_blocks) == (
        24, 24, 1536, 64, True, 384, 13)
    assert c.dtype == SD3_8b.dtype and c.pos_embed_type == PositionalEncoding.LearnedInputEmbedding
    assert c.num_modulation_rows() == 13 * 15 + 10 * 12 + 8 + 2
    assert c.param_count() - replace(c, dual_attention_blocks=0).param_count() == 13 * (4 + 3) * 1536 * 1536  # attn2 + three adaLN rows
    t = tiny_sd35m()
    assert (t.depth_multimodal, t.num_heads, t.dual_attention_blocks, t.head_dim) == (3, 4, 2, 64)
    assert float16_config(c).activation_dtype == "float16"
    with pytest.raises(ValueError, match="head_dim 128"):
        fp8_config(c)
    for bad in (replace(t, dual_attention_blocks=4), replace(t, dual_attention_blocks=-1), replace(tiny_flux(), dual_attention_blocks=1),
                replace(t, weight_dtype="fp8_e4m3")):
        with pytest.raises(ValueError, match="dual_attention_blocks"):
            validate_dual_attention(bad)
    assert MODEL_CONFIG[VERSION] is SD3_5_MEDIUM and list(MMDIT_CKPT)[-1] == VERSION


def test_without_dual_blocks_the_tables_are_todays():
    """n_dual = 0: the numbers of the parent commit (344 rows for FLUX: 19 * 12 + 38 * 3 + 2)"""
    for cfg, rows in ((SD3_2b, 23 * 12 + 8 + 2), (SD3_8b, 37 * 12 + 8 + 2), (FLUX_SCHNELL, 344)):
        assert cfg.dual_attention_blocks == 0 and cfg.num_modulation_rows() == rows
        lib, h = make_handle(cfg)
        check_table(lib, h, cfg)
        assert lib.dk_mmdit_set_dual_attention(h, 0) == 0  # (off is legal for every family)
        check_table(lib, h, cfg)
        lib.dk_mmdit_destroy(h)


# ---- the setter's refusals ------------------------------------------------------------------------------------------------------------
def bind_all(lib, h, packed):
    for name, t in packed.items():  # (host pointers: bound by name, never read before a launch)
        assert lib.dk_mmdit_bind(h, name.encode(), t.data_ptr()) == 0


def resolve_only(lib, h):
    """dk_mmdit_prepare up to its size check: the weights are resolved, nothing is launched"""
    rc = lib.dk_mmdit_prepare(h, 1, 8, 8, 16, 1, 4096, 0, None)
    return rc, last_error(lib)


def test_setter_refusals_leave_the_engine_as_it_was():
    assert _lib.load().dk_abi_version() == 5
    # FLUX geometry
    lib, h = make_handle(tiny_flux())
    rows = lib.dk_mmdit_mod_rows(h)
    assert lib.dk_mmdit_set_dual_attention(h, 1) != 0 and "depth_unified == 0" in last_error(lib)
    assert lib.dk_mmdit_mod_rows(h) == rows
    lib.dk_mmdit_destroy(h)
    # fp8 Linears (head_dim 128, no single blocks: only the fp8 rule can refuse it)
    lib, h = make_handle(replace(tiny_flux(depth_unified=0), pos_embed_type=PositionalEncoding.LearnedInputEmbedding, rope_axes_dim=None), fp8=True)
    rows = lib.dk_mmdit_mod_rows(h)
    assert lib.dk_mmdit_set_dual_attention(h, 1) != 0 and "fp8_linears == 0" in last_error(lib)
    assert lib.dk_mmdit_mod_rows(h) == rows
    lib.dk_mmdit_destroy(h)
    # out of range, then a legal value on the same handle
    cfg = tiny_sd35m()
    lib, h = make_handle(cfg)
    for n in (-1, cfg.depth_multimodal + 1):
        assert lib.dk_mmdit_set_dual_attention(h, n) != 0 and "[0, depth_multimodal]" in last_error(lib)
        assert lib.dk_mmdit_mod_rows(h) == replace(cfg, dual_attention_blocks=0).num_modulation_rows()
    assert lib.dk_mmdit_set_dual_attention(h, cfg.dual_attention_blocks) == 0
    check_table(lib, h, cfg)
    # after the weights are resolved
    packed = pack_mmdit(cfg, synth_mmdit_weights(cfg), "cpu")
    bind_all(lib, h, packed)
    rc, msg = resolve_only(lib, h)
    assert rc != 0 and "workspace too small" in msg
    assert lib.dk_mmdit_set_dual_attention(h, 1) != 0 and "before the weights are resolved" in last_error(lib)
    check_table(lib, h, cfg)
    assert lib.dk_mmdit_workspace_bytes(h, 2, 8, 12, 20, 3) > 0
    lib.dk_mmdit_destroy(h)


def test_attn2_weights_are_required_inside_the_range_and_refused_outside():
    cfg = tiny_sd35m()
    packed = pack_mmdit(cfg, synth_mmdit_weights(cfg), "cpu")
    b0, b1 = (f"multimodal_transformer_blocks.{i}.image_transformer_block" for i in (0, 1))
    h_ = cfg.hidden_size
    assert packed[b0 + ".attn2.qkv.weight"].shape == (3 * h_, h_) and packed[b0 + ".attn2.o_proj.weight"].shape == (h_, h_)
    assert bool((packed[b0 + ".attn2.qkv.bias"][h_:2 * h_] != 0).any())  # attn2's k bias is kept (the main attention's is zero: quirk Q9)
    assert bool((packed[b0 + ".attn.qkv.bias"][h_:2 * h_] == 0).all())
    assert packed[b0 + ".qk_norm2.k_norm.weight"].shape == (64,) and packed["adaLN.weight"].shape == (cfg.num_modulation_rows() * h_, h_)
    assert not any("attn2" in k or "qk_norm2" in k for k in packed if ".2.image_transformer_block" in k)
    # missing inside the range
    lib, h = make_handle(cfg)
    assert lib.dk_mmdit_set_dual_attention(h, 2) == 0
    bind_all(lib, h, {k: v for k, v in packed.items() if k != b1 + ".attn2.o_proj.weight"})
    rc, msg = resolve_only(lib, h)
    assert rc != 0 and "weight not bound" in msg and b1 + ".attn2.o_proj.weight" in msg
    lib.dk_mmdit_destroy(h)
    # bound outside the range: an engine that would ignore them refuses them
    lib, h = make_handle(cfg)
    assert lib.dk_mmdit_set_dual_attention(h, 1) == 0
    bind_all(lib, h, packed)
    rc, msg = resolve_only(lib, h)
    assert rc != 0 and "outside the dual attention range" in msg and b1 + ".attn2." in msg
    lib.dk_mmdit_destroy(h)


# ---- workspace ------------------------------------------------------------------------------------------------------------------------
def carve_bytes(lib, cfg, B, Hl, Wl, S_t, n_t):
    """mmdit_carve of the parent commit for bf16 Linears without cache / reference / condition: every take starts on 256 bytes; returns
    (dk_mmdit_workspace_bytes, end of the last take)"""
    h, r, p = cfg.hidden_size, cfg.mlp_ratio, cfg.patch_size
    S_i = (Hl // p) * (Wl // p)
    S = S_t + S_i
    BS = B * S
    rope = cfg.pos_embed_type == PositionalEncoding.PreSDPARope
    ldh, ldcat = lib.dk_weight_pitch(r * h), lib.dk_weight_pitch((1 + r) * h)
    hid, cat = BS * ldh * 2, (BS * ldcat * 2 if cfg.depth_unified > 0 else 0)
    g = 1 if cfg.guidance_embed else 0
    takes = [BS * h * 2, BS * h * 2, BS * 3 * h * 2, BS * h * 2, max(cat, hid), n_t * B * cfg.num_modulation_rows() * h * 2,
             0 if rope else S_i * h * 2, B * S_t * h * 2, n_t * cfg.frequency_embed_dim * 2, n_t * h * 2, n_t * h * 2, B * h * 2, B * h * 2,
             n_t * B * h * 2, g * cfg.frequency_embed_dim * 2, g * h * 2, g * h * 2, S * cfg.head_dim * 4 if rope else 0, n_t * 4,
             lib.dk_gemm_workspace_bytes(), lib.dk_attention_workspace_bytes() if cfg.head_dim == 128 else 0]
    off = 0
    for n in takes:
        off = (off + 255) // 256 * 256 + n
    return off + 256, off


@pytest.mark.parametrize("cfg,shape", [(tiny_sd3(), (2, 8, 12, 20, 3)), (tiny_flux(), (1, 16, 16, 256, 4)), (SD3_2b, (2, 128, 128, 154, 28)),
                                       (tiny_sd35m(dual=0), (2, 10, 14, 20, 3))], ids=["tiny_sd3", "tiny_flux", "sd3_2b", "sd35m_dual0"])
def test_workspace_without_dual_blocks_is_the_parents(cfg, shape):
    lib, h = make_handle(cfg)
    assert lib.dk_mmdit_set_dual_attention(h, 0) == 0
    assert lib.dk_mmdit_workspace_bytes(h, *shape) == carve_bytes(lib, cfg, *shape)[0]
    lib.dk_mmdit_destroy(h)


@pytest.mark.parametrize("cfg,shape", [(tiny_sd35m(), (2, 10, 14, 20, 3)), (SD3_5_MEDIUM, (2, 128, 128, 154, 28))], ids=["tiny", "medium"])
def test_workspace_with_dual_blocks_adds_three_buffers_behind_everything(cfg, shape):
    """XN2 + QKV2 + ATT2 = 5 B S_x h elements behind the parent's carve (whose modulation table holds the three extra rows per dual block)"""
    lib, h = make_handle(cfg)
    assert lib.dk_mmdit_set_dual_attention(h, cfg.dual_attention_blocks) == 0
    B, Hl, Wl = shape[:3]
    Mi, hs = B * (Hl // 2) * (Wl // 2), cfg.hidden_size
    total, end = carve_bytes(lib, cfg, *shape)
    got = lib.dk_mmdit_workspace_bytes(h, *shape)
    assert 5 * Mi * hs * 2 <= got - total <= 5 * Mi * hs * 2 + 3 * 256
    off = end
    for n in (Mi * hs * 2, Mi * 3 * hs * 2, Mi * hs * 2):
        off = (off + 255) // 256 * 256 + n
    assert got == off + 256
    lib.dk_mmdit_destroy(h)


# ---- synthetic weights ----------------------------------------------------------------------------------------------------------------
def _digest(w):
    d = hashlib.sha256()
    for k in w:
        d.update(k.encode())
        d.update(w[k].view(torch.int16).numpy().tobytes())
    return d.hexdigest()


def test_synthetic_weights_without_dual_blocks_are_todays():
    """names, order and bits of every tensor, pinned on the parent commit"""
    w = synth_mmdit_weights(tiny_sd3())
    assert len(w) == 63 and _digest(w) == "f58d45dad1c945c462506d1aaa08e25701570fd3f0ea24fe483b0a6fb2874e94"
    k = "multimodal_transformer_blocks.1.image_transformer_block.adaLN_modulation.layers.1.weight"
    assert hashlib.sha256(w[k].view(torch.int16).numpy().tobytes()).hexdigest()[:16] == "c22166d65f2629e3"
    assert float(w["x_embedder.proj.weight"].float().sum()) == -0.1329241394996643
    wf = synth_mmdit_weights(tiny_flux())
    assert len(wf) == 104 and _digest(wf) == "38e4cb8bd617d04985b268eea19c07425702ecd7a56623b3940a129133bea550"
    # the dual tensors come behind that stream: the same model without them is a prefix, bit for bit
    cfg = tiny_sd35m()
    wd = synth_mmdit_weights(cfg)
    cfg0, w0 = without_dual(wd, cfg)
    ref = synth_mmdit_weights(cfg0)
    assert list(ref) == list(w0) and all(torch.equal(ref[k], w0[k]) for k in ref)
    b0 = "multimodal_transformer_blocks.0.image_transformer_block"
    assert wd[b0 + ".adaLN_modulation.layers.1.weight"].shape == (9 * cfg.hidden_size, cfg.hidden_size)
    assert wd[b0 + ".attn2.k_proj.bias"].shape == (cfg.hidden_size,) and b0.replace(".0.", ".2.") + ".attn2.q_proj.weight" not in wd


# ---- checkpoint loader ----------------------------------------------------------------------------------------------------------------
def test_loader_round_trip_through_the_stability_layout():
    cfg = tiny_sd35m()
    w = synth_mmdit_weights(cfg)
    sd = to_stability_sd3(w, cfg)
    assert "model.diffusion_model.joint_blocks.1.x_block.attn2.qkv.weight" in sd and "model.diffusion_model.joint_blocks.2.x_block.attn2.qkv.weight" not in sd
    for back in (sd3_checkpoint_to_reference(sd, cfg), load_mmdit_checkpoint(sd, cfg)):
        assert set(back) == set(w)
        for k in w:
            assert torch.equal(back[k], w[k]), k
    assert "multimodal_transformer_blocks.0.image_transformer_block.attn2.k_proj.bias" in back  # kept, unlike attn.k_proj's (quirk Q9)
    assert "multimodal_transformer_blocks.0.image_transformer_block.attn.k_proj.bias" not in back


def test_loader_refuses_stray_and_missing_attn2_tensors():
    cfg = tiny_sd35m()
    sd = to_stability_sd3(synth_mmdit_weights(cfg), cfg)
    pre = "model.diffusion_model.joint_blocks."
    stray = dict(sd)
    stray[pre + "2.x_block.attn2.qkv.weight"] = sd[pre + "0.x_block.attn2.qkv.weight"]
    with pytest.raises(CheckpointError, match=r"joint_blocks\.2\.x_block\.attn2\.qkv\.weight"):
        sd3_checkpoint_to_reference(stray, cfg)
    stray = dict(sd)
    stray[pre + "0.context_block.attn2.proj.bias"] = sd[pre + "0.x_block.attn2.proj.bias"]
    with pytest.raises(CheckpointError, match=r"context_block\.attn2\.proj\.bias"):
        sd3_checkpoint_to_reference(stray, cfg)
    missing = {k: v for k, v in sd.items() if k != pre + "1.x_block.attn2.ln_k.weight"}
    with pytest.raises(CheckpointError, match=r"multimodal_transformer_blocks\.1\.image_transformer_block\.qk_norm2\.k_norm\.weight"):
        sd3_checkpoint_to_reference(missing, cfg)
    with pytest.raises(CheckpointError, match="attn2"):  # the checkpoint of a dual model under a configuration without dual blocks
        sd3_checkpoint_to_reference(sd, replace(cfg, dual_attention_blocks=0))


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------
def test_cli_knows_the_version():
    a = cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args(["--prompt", "x", "--model-version", VERSION, "--local-ckpt", "sd3.5_medium.safetensors"])
    r = cli.resolve(a)
    assert (r["flux"], r["shift"], r["height"], r["width"], r["cfg"]) == (False, 3.0, cli.HEIGHT[VERSION], cli.WIDTH[VERSION], 5.0)
    assert MODEL_CONFIG[a.model_version] is SD3_5_MEDIUM and cli.checkpoint_dict(a.local_ckpt, a.ckpt) == {"mmdit": "sd3.5_medium.safetensors"}
    with pytest.raises(ValueError, match="FLUX"):  # reference-image conditioning keeps refusing the SD3 family
        cli.resolve(cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args(["--prompt", "x", "--model-version", VERSION, "--reference-image-path", "r.png"]))
