"""CPU-side checks of the float16 activation mode of the SD3 family (the reference's dtype for Stable Diffusion 3, config.py:77-79): the config rule,
weight packing, the CLI flag, the pipeline's rejection of FLUX, the C-ABI additions, the fp16 GEMM routes (dk_gemm_plan_f16: no kernel runs) and the
weight blob of the data-parallel path."""
import ctypes as C
import os
import re
import socket
from dataclasses import replace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from diffusionkit_amd import _lib, cli
from diffusionkit_amd.config import MMDIT_CKPT, SD3_2b, SD3_8b, MMDiTConfig, tiny_flux, tiny_sd3

F16_SYMBOLS = ("dk_mmdit_set_activation_dtype", "dk_gemm_f16", "dk_gemm_plan_f16", "dk_gemm_fused_f16", "dk_attention_desc_f16", "dk_attention_plan_f16", "dk_ln_modulate_f16",
               "dk_qk_norm_rope_f16", "dk_timestep_embedding_f16", "dk_latent_to_tokens_f16", "dk_euler_cfg_step_f16")


def test_default_is_bfloat16_and_the_rule_names_the_family():
    from diffusionkit_amd.config import float16_config, fp8_config, validate_activation_dtype
    assert MMDiTConfig().activation_dtype == "bfloat16" and SD3_2b.activation_dtype == "bfloat16"
    for cfg in (tiny_sd3(), SD3_2b, SD3_8b):
        c = float16_config(cfg)
        assert c.activation_dtype == "float16" and replace(c, activation_dtype="bfloat16") == cfg
        validate_activation_dtype(c)
    validate_activation_dtype(tiny_flux())  # bfloat16: every family
    with pytest.raises(ValueError, match="head_dim == 64 and depth_unified == 0"):
        float16_config(tiny_flux())
    with pytest.raises(ValueError, match="fp8_e4m3"):
        # (a geometry fp8_config accepts has head_dim 128, which the first rule rejects: the fp8 rule is reached with head_dim 64)
        validate_activation_dtype(replace(tiny_sd3(), weight_dtype="fp8_e4m3", activation_dtype="float16"))
    with pytest.raises(ValueError):
        float16_config(fp8_config(tiny_flux(1, 1)))
    with pytest.raises(ValueError, match="unknown activation_dtype"):
        validate_activation_dtype(replace(tiny_sd3(), activation_dtype="float32"))


def test_pack_mmdit_emits_float16_and_rounds_once():
    from diffusionkit_amd.config import float16_config
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    cfg = tiny_sd3()
    w = synth_mmdit_weights(cfg, dtype=torch.float32)
    name = "multimodal_transformer_blocks.0.image_transformer_block.attn.o_proj.weight"
    w[name][0, 0] = 1.0 + 2.0 ** -10   # one fp16 ulp above 1: not a bf16 value
    w[name][0, 1] = 1.0 + 2.0 ** -12   # not an fp16 value either: rounds (once) to 1
    p16 = pack_mmdit(float16_config(cfg), w, "cpu")
    pbf = pack_mmdit(cfg, w, "cpu")
    assert set(p16) == set(pbf)
    for k in pbf:
        assert p16[k].dtype == torch.float16 and pbf[k].dtype == torch.bfloat16, k
        assert p16[k].shape == pbf[k].shape and p16[k].stride() == pbf[k].stride(), k  # same names, pitches and fusions
    base = name[:-len(".weight")]
    assert float(p16[base + ".weight"][0, 0]) == 1.0 + 2.0 ** -10 and float(pbf[base + ".weight"][0, 0]) == 1.0
    assert float(p16[base + ".weight"][0, 1]) == 1.0
    # an fp16 checkpoint tensor reaches the engine bit for bit (through the q | k | v fusion too)
    w16 = {k: v.to(torch.float16) for k, v in w.items()}
    q16 = pack_mmdit(float16_config(cfg), w16, "cpu")
    b0 = "multimodal_transformer_blocks.0.image_transformer_block"
    h = cfg.hidden_size
    assert torch.equal(q16[b0 + ".attn.qkv.weight"][h:2 * h], w16[b0 + ".attn.k_proj.weight"])
    assert torch.equal(q16[base + ".weight"], w16[name]) and all(torch.equal(q16[k], p16[k]) for k in p16)


def test_cli_flag_and_default():
    def parse(argv):
        return cli.build_parser(tuple(MMDIT_CKPT.keys())).parse_args(argv)
    sd3 = ["--prompt", "x", "--model-version", "argmaxinc/mlx-stable-diffusion-3-medium"]
    a = parse(sd3)
    assert a.activation_dtype == "bfloat16"
    assert cli.resolve(a) == {"cfg": 5.0, "shift": 3.0, "height": 512, "width": 512, "flux": False, "low_memory_mode": True}  # as before the flag existed
    r = cli.resolve(parse(sd3 + ["--activation-dtype", "float16"]))
    assert r["activation_dtype"] == "float16" and r["flux"] is False
    with pytest.raises(ValueError, match="head_dim == 64"):
        cli.resolve(parse(["--prompt", "x", "--activation-dtype", "float16"]))  # the default model version is FLUX
    with pytest.raises(SystemExit):
        parse(sd3 + ["--activation-dtype", "float32"])


def test_flux_pipeline_rejects_float16():
    from diffusionkit_amd.pipeline import DiffusionPipeline, FluxPipeline
    with pytest.raises(ValueError, match="SD3 family"):
        FluxPipeline(w16=True, a16=True, activation_dtype="float16", device="cpu", mmdit_config=tiny_flux(1, 1))
    with pytest.raises(ValueError, match="unknown activation_dtype"):
        DiffusionPipeline(w16=True, a16=True, activation_dtype="float32", device="cpu", mmdit_config=tiny_sd3())


def test_new_symbols_in_header_library_and_ctypes_table():
    lib = _lib.load()
    header = set(re.findall(r"\b(dk_[a-z0-9_]+)\s*\(", open(_lib.HEADER_PATH).read()))
    for s in F16_SYMBOLS:
        assert s in header and s in _lib.SIGNATURES and hasattr(lib, s), s
    assert lib.dk_abi_version() == 5  # purely additive


def test_setter_accepts_only_the_sd3_family_and_only_before_bind():
    from diffusionkit_amd.engine import MMDiTEngine
    from diffusionkit_amd.config import float16_config
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    lib = _lib.load()
    cfg = float16_config(tiny_sd3())
    packed = pack_mmdit(cfg, synth_mmdit_weights(cfg), "cpu")
    with pytest.raises(_lib.DkHipError, match="GPU"):  # (the boundary check: fp16 tensors are what it now expects, and they must be on the device)
        MMDiTEngine(cfg, packed)
    with pytest.raises(_lib.DkHipError, match="head_dim == 64"):
        MMDiTEngine(replace(tiny_flux(1, 1), activation_dtype="float16"), packed)

    def create(cfg):
        eng = MMDiTEngine.__new__(MMDiTEngine)  # the config marshalling of __init__, without tensors
        c = _lib.dk_mmdit_config()
        c.num_heads, c.depth_multimodal, c.depth_unified = cfg.num_heads, cfg.depth_multimodal, cfg.depth_unified
        c.hidden_size, c.mlp_ratio, c.vae_latent_dim, c.patch_size = cfg.hidden_size, cfg.mlp_ratio, cfg.vae_latent_dim, cfg.patch_size
        c.use_pos_embed, c.max_latent_resolution = 1, cfg.max_latent_resolution
        c.pooled_text_embed_dim, c.token_level_text_embed_dim = cfg.pooled_text_embed_dim, cfg.token_level_text_embed_dim
        c.frequency_embed_dim, c.max_period, c.layer_norm_eps = cfg.frequency_embed_dim, cfg.max_period, cfg.layer_norm_eps
        h = C.c_void_p()
        assert lib.dk_mmdit_create(C.byref(c), C.byref(h)) == 0, lib.dk_last_error()
        return h
    h = create(tiny_sd3())
    assert lib.dk_mmdit_set_activation_dtype(h, 1) == 0 and lib.dk_mmdit_set_activation_dtype(h, 0) == 0
    assert lib.dk_mmdit_set_activation_dtype(h, 2) != 0 and b"0 bf16, 1 fp16" in lib.dk_last_error()
    buf = torch.zeros(64)
    assert lib.dk_mmdit_bind(h, b"x", buf.data_ptr()) == 0
    assert lib.dk_mmdit_set_activation_dtype(h, 1) != 0 and b"precede the first dk_mmdit_bind" in lib.dk_last_error()
    lib.dk_mmdit_destroy(h)
    h = create(replace(tiny_sd3(heads=2), hidden_size_override=256))  # head_dim 128
    assert lib.dk_mmdit_set_activation_dtype(h, 1) != 0 and b"head_dim == 64, depth_unified == 0, fp8_linears == 0" in lib.dk_last_error()
    assert lib.dk_mmdit_set_activation_dtype(h, 0) == 0
    lib.dk_mmdit_destroy(h)


FAKE_WS = 0x10000


def _plan(fn, M, N, K, M2=0):
    lib = _lib.load()

    def desc(m):
        d = _lib.dk_gemm_desc()
        d.M, d.N, d.K, d.lda, d.ldc, d.ldr, d.alpha, d.epilogue = m, N, K, K, N, N, 1.0, 0
        d.workspace, d.workspace_bytes = FAKE_WS, lib.dk_gemm_workspace_bytes()
        return d
    p, a, b = _lib.dk_gemm_plan_t(), desc(M), desc(M2) if M2 else None
    assert getattr(lib, fn)(C.byref(a), C.byref(b) if b is not None else None, C.byref(p)) == 0, lib.dk_last_error()
    return [getattr(p, f) for f, _ in p._fields_], p


def test_f16_plan_never_names_generation_4_and_keeps_the_other_routes():
    """the SD3 sweep of tests/test_dispatch_plan.py (384 ... 1536 pixels x batch 1 ... 8; SD3-medium h = 1536 with 589 text rows per batch row,
    SD3.5-large h = 2432): fp16 launches stay on gemm256v3.hip / the 128 x 128 kernel -- also under the knobs that force the bf16-only kernel -- and
    every launch that bf16 already routes there is routed identically."""
    lib = _lib.load()
    n = same = gen4 = 0
    for h, txt in ((1536, 589), (2432, 589)):
        for res in (384, 512, 640, 768, 896, 1024, 1280, 1536):
            for batch in (1, 2, 4, 8):
                M_img, M_txt = 2 * batch * (res // 16) ** 2, 2 * batch * txt
                for N, K in ((3 * h, h), (h, h), (4 * h, h), (h, 4 * h)):
                    for args in ((M_img, N, K, M_txt), (M_img, N, K), (M_txt, N, K)):
                        fb, pb = _plan("dk_gemm_plan", *args)
                        ff, pf = _plan("dk_gemm_plan_f16", *args)
                        assert pf.kernel in (3, 128) and pf.launches >= 1, (h, res, batch, args, pf.kernel)
                        n += 1
                        gen4 += pb.kernel == 4
                        if pb.kernel in (3, 128):
                            assert ff == fb, (h, res, batch, args, ff, fb)
                            same += 1
    assert n == 2 * 8 * 4 * 4 * 3 and same > 0 and gen4 > 0  # (the sweep does contain launches bf16 sends to generation 4)
    try:  # the knobs that name the bf16-only kernel have no effect on fp16 launches
        base, _ = _plan("dk_gemm_plan_f16", 8192, 6144, 1536)
        for key, v in ((b"gemm", 10), (b"gemm_v4", 2)):
            assert lib.dk_tune_set(key, v) == 0
            assert _plan("dk_gemm_plan", 8192, 6144, 1536)[1].kernel == 4
            assert _plan("dk_gemm_plan_f16", 8192, 6144, 1536)[0] == base
            lib.dk_tune_set(key, -1)
    finally:
        lib.dk_tune_set(b"gemm", -1)
        lib.dk_tune_set(b"gemm_v4", -1)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from diffusionkit_amd import dist as dk
    from diffusionkit_amd.config import float16_config
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    r, _, _ = dk.init_distributed("gloo")
    cfg = float16_config(tiny_sd3(1))
    ref = pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=99), "cpu")
    got = dk.broadcast_weights(ref if r == 0 else None, "cpu", src=0, chunk_elems=100_003)
    ok = set(got) == set(ref) and all(got[k].dtype == torch.float16 and torch.equal(got[k], ref[k]) for k in ref)
    dist.barrier()
    q.put((r, ok))
    dist.destroy_process_group()


def test_weight_blob_keeps_float16_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
    assert res == {0: True, 1: True}
