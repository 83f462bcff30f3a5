"""FLUX IP-Adapter on the MI355X: the decoupled image-prompt attention kernel against float64 under the operator gate and its footprint, the engine
against ``tests/_ip_adapter.IPAdapterFluxOracle`` (tiny models, the production width, guarded and poisoned workspaces, the refusals), and the
pipeline's step loop against the oracle loop.

The gates are the project's own (tests/test_gpu_model.py: err(hip, fp32) <= 2 err(emu, fp32) + 2e-3 and PSNR > 35 dB) and the operator gate of
tests/_ip_adapter.py (twice the fp32 restatement's error plus one bf16 unit, proved on mutants in tests/test_ip_adapter_cpu.py); nothing here sets a
tolerance of its own.  Arithmetic parity on synthetic weights: no adapter checkpoint has been run."""
from dataclasses import replace

import pytest
import torch

from diffusionkit_amd.config import FLUX_SCHNELL, IPAdapterConfig, fp8_config, tiny_flux, tiny_flux_controlnet, tiny_ip_adapter, tiny_sd3
from diffusionkit_amd.weights import pack_ip_adapter, pack_mmdit, synth_ip_adapter_weights, synth_mmdit_weights
from oracle.mmdit import Prec, embed_dtype
from tests import _ip_adapter as IP
from tests._engine_state import FILL_NAN, GuardedWorkspace, lend
from tests._footprint import NAN, SENTINEL, assert_footprint, bits, guarded
from tests._ip_adapter import IP_SCALE, IPAdapterFluxOracle, synthetic_embeds
from tests._util import BF, psnr, randn, rel_l2
from tests.test_gpu_model import psnr_ok, yardstick_ok

pytestmark = pytest.mark.gpu

TS = [1000.0, 752.0, 500.0]
IPC = tiny_ip_adapter()


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 4, 7, 16])
@pytest.mark.parametrize("rows", IP.ROWS, ids=[f"B{b}_St{t}_Si{i}" for b, t, i in IP.ROWS])
@pytest.mark.parametrize("h", [256, 3072])
def test_ip_attention_against_float64(dev, h, rows, N):
    """h 256: two heads, half of every wave's lanes past the row end; 3072: 24 heads, six column chunks.  (1, 0, 5): no text rows and one partial
    workgroup; (2, 3, 5): the image rows of batch row 1 sit behind its text rows; (2, 8, 70): three workgroups per image, the last with 6 rows;
    (3, 5, 6): three images.  Per-image K / V: image b's rows see image b's keys only (the reference indexes them so)."""
    from diffusionkit_amd import ops
    B, S_t, S_i = rows
    qkv, qn, k, v = IP.kernel_case(h, B, S_t, S_i, N)
    got = ops.ip_attention(qkv.to(dev, BF), S_t, qn.to(dev, BF), k.to(dev, BF), v.to(dev, BF))
    assert tuple(got.shape) == (B * S_i, h) and got.dtype == BF
    ref = IP.ip_attention_ref(qkv, S_t, qn, k, v)
    rest = IP.ip_attention_ref(qkv, S_t, qn, k, v, torch.float32)
    r, r0 = IP.operator_ratio(got, rest, ref), IP.operator_ratio(rest, rest, ref)
    print(f"[ip adapter] kernel h {h} rows {rows} N {N}: worst (row, head) at {r:.3f} of the bound (restatement {r0:.3f})")
    assert r <= 1.0
    if B > 1 and N > 1:  # (the images' keys differ: a launch that gave every image the first one's would miss the gate)
        assert IP.operator_ratio(IP.ip_attention_ref(qkv, S_t, qn, k, v, torch.float32, mutant="image 1 reads image 0"), rest, ref) > 2.0


@pytest.mark.parametrize("case", [(256, (2, 3, 5), 4), (256, (2, 8, 70), 7), (3072, (2, 3, 5), 4), (256, (3, 5, 6), 16)], ids=str)
def test_ip_attention_equal_values(dev, case):
    """every key of an image carries the same value row (tests/_ip_adapter.equal_values_case): the definition's output is that row, the gate's bound
    is one bf16 unit alone -- the case on which tests/test_ip_adapter_cpu.py proves that the gate rejects an output rounded twice.  The kernel
    rounds once: it returns the row bit for bit"""
    from diffusionkit_amd import ops
    h, (B, S_t, S_i), N = case
    qkv, qn, k, v = IP.equal_values_case(h, B, S_t, S_i, N)
    got = ops.ip_attention(qkv.to(dev, BF), S_t, qn.to(dev, BF), k.to(dev, BF), v.to(dev, BF))
    ref, rest = IP.ip_attention_ref(qkv, S_t, qn, k, v), IP.ip_attention_ref(qkv, S_t, qn, k, v, torch.float32)
    r = IP.operator_ratio(got, rest, ref)
    print(f"[ip adapter] kernel, equal values, {case}: worst (row, head) at {r:.3f} of the bound")
    assert r <= 1.0
    assert same_bits(got, v[:, :1].expand(B, S_i, h).reshape(B * S_i, h).to(BF))


def test_ip_attention_pitched_keys_and_refusals(dev):
    """K and V as column slices of one [B, N, 2h] buffer (the engine's cache layout) give the bits of dense ones; N = 17, 0 and D = 64 are refused
    by name"""
    from diffusionkit_amd import ops
    from diffusionkit_amd._lib import DkHipError
    h, B, S_t, S_i, N = 256, 2, 3, 5, 4
    qkv, qn, k, v = (t.to(dev, BF) for t in IP.kernel_case(h, B, S_t, S_i, N))
    dense = ops.ip_attention(qkv, S_t, qn, k, v)
    both = torch.cat([k, v], dim=2).contiguous()
    assert same_bits(ops.ip_attention(qkv, S_t, qn, both[:, :, :h], both[:, :, h:]), dense)
    z = lambda n: torch.zeros(B, n, h, dtype=BF, device=dev)
    with pytest.raises(DkHipError, match=r"\[1, 16\]"):
        ops.ip_attention(qkv, S_t, qn, z(17), z(17))
    with pytest.raises(DkHipError, match=r"\[1, 16\]"):
        ops.ip_attention(qkv, S_t, qn, z(0), z(0))
    with pytest.raises(DkHipError, match="head_dim must be 128"):
        ops.ip_attention(qkv, S_t, qn[:64].contiguous(), k, v, head_dim=64)


def launch_ip(qkv, S_t, qn, k, v, out):
    """dk_ip_attention_bf16 on caller-owned buffers (ops.ip_attention allocates its output: no margins to check)"""
    from diffusionkit_amd import _lib
    from diffusionkit_amd.ops import _stream
    B, S, h3 = qkv.shape
    h = h3 // 3
    _lib.check(_lib.load().dk_ip_attention_bf16(qkv.data_ptr(), h3, S - S_t, S, S_t, qn.data_ptr(), k.data_ptr(), v.data_ptr(), h, B, k.shape[1], h, 128,
                                                128 ** -0.5, 1e-6, out.data_ptr(), _stream()), "dk_ip_attention_bf16")


def test_ip_attention_footprint(dev):
    """h 256, (2, 3, 5), N 4; QKV, K, V and the output between NaN margins at exact size.  A NaN in one K element of head 1, image 1 poisons exactly
    head 1's 128 columns of image 1's rows; a NaN in a text row's q, or in the k / v columns of QKV, reaches nothing; the margins stay."""
    h, B, S_t, S_i, N = 256, 2, 3, 5, 4
    qkv0, qn, k0, v0 = (t.to(dev, BF) for t in IP.kernel_case(h, B, S_t, S_i, N))
    runs = {}
    for name in ("clean", "key", "text q", "k columns", "v columns"):
        qkv, gq = guarded(qkv0, 2)
        k, gk = guarded(k0, 2)
        v, gv = guarded(v0, 2)
        out, go = guarded(torch.full((B * S_i, h), SENTINEL, dtype=BF, device=dev), 2, fill=SENTINEL)
        if name == "key":
            k[1, 2, 128 + 77] = NAN
        if name == "text q":
            qkv[1, S_t - 1, 5] = NAN
            qkv[0, 0, 200] = NAN
        if name == "k columns":
            qkv[:, :, h:2 * h] = NAN
        if name == "v columns":
            qkv[:, :, 2 * h:] = NAN
        launch_ip(qkv, S_t, qn, k, v, out)
        torch.cuda.synchronize()
        for g, what in ((gq, "qkv"), (gk, "k"), (gv, "v"), (go, "out")):
            g.check(f"{name}: {what}")
        runs[name] = out.clone()
    clean = runs["clean"]
    assert not bool((clean == SENTINEL).any()), "every output element is written"
    expect = torch.zeros(clean.shape, dtype=torch.bool)
    expect[S_i:, 128:] = True
    assert_footprint(clean, runs["key"], expect, "K NaN, head 1 of image 1")
    for name in ("text q", "k columns", "v columns"):
        assert_footprint(clean, runs[name], torch.zeros(clean.shape, dtype=torch.bool), f"{name} NaN")


# ---- the engine -------------------------------------------------------------------------------------------------------------------------
def build(cfg, dev, ipc=IPC, seed=1234, named=None):
    from diffusionkit_amd.engine import MMDiTEngine
    wm, wa = named or (synth_mmdit_weights(cfg, seed=seed), synth_ip_adapter_weights(cfg, ipc, seed=2468))
    return MMDiTEngine(cfg, {**pack_mmdit(cfg, wm, dev), **pack_ip_adapter(cfg, ipc, wa, dev)}, ip_adapter=ipc)


def inputs(cfg, B, Hl, Wl, S_t):
    return randn(B, S_t, cfg.token_level_text_embed_dim, seed=3), randn(B, cfg.pooled_text_embed_dim, seed=4), randn(B, Hl, Wl, 16, seed=5)


def prepared(cfg, dev, B, Hl, Wl, S_t, ipc=IPC, named=None):
    eng = build(cfg, dev, ipc, named=named)
    text, pooled, lat = inputs(cfg, B, Hl, Wl, S_t)
    eng.prepare(B, (Hl, Wl), S_t, len(TS))
    eng.cache_modulation_params(pooled.to(dev), TS)
    return eng, text.to(dev, BF), eng.patchify(lat.to(dev))


def tokens_for(eng, embeds, dev):
    from diffusionkit_amd.engine import ip_adapter_project
    return ip_adapter_project(eng.weights, eng.ip_adapter, embeds.to(dev))


_oracle_cache = {}


def oracle(cfg, B, Hl, Wl, S_t, ipc=IPC, step=1, named=None, embed_prec=False):
    """the final layer's output of the fp32 and the bf16-emulating IPAdapterFluxOracle under per-image synthetic embeddings, and of the fp32 one
    without the adapter; computed once per case"""
    key = (cfg, B, Hl, Wl, S_t, ipc, step)
    if key not in _oracle_cache:
        wm, wa = named or (synth_mmdit_weights(cfg, seed=1234), synth_ip_adapter_weights(cfg, ipc, seed=2468))
        wm, wa = ({k: v.float() for k, v in w.items()} for w in (wm, wa))
        text, pooled, lat = inputs(cfg, B, Hl, Wl, S_t)
        ip = (wa, ipc, synthetic_embeds(B, ipc.embed_dim), IP_SCALE)
        res = {}
        for name, P, a in (("fp32", Prec(), ip), ("emu", Prec(BF), ip), ("plain", Prec(), None)):
            kw = dict(embed_prec=Prec(embed_dtype(cfg))) if embed_prec and P.act is None else {}
            m = IPAdapterFluxOracle(cfg, wm, P, **kw)
            m.ip = a
            m.cache_modulation_params(pooled, torch.tensor(TS))
            streams = {}
            m(lat, text, TS[step], taps=streams)
            res[name] = streams["final"]
        _oracle_cache[key] = res
    return _oracle_cache[key]


ENGINE = {"3+2": (tiny_flux(3, 2), 2, 8, 12, 20), "3+0": (tiny_flux(3, 0), 2, 8, 12, 20), "3+2_35tok": (tiny_flux(3, 2), 2, 10, 14, 20),
          "3+0_35tok": (tiny_flux(3, 0), 2, 10, 14, 20)}


@pytest.mark.parametrize("name", list(ENGINE))
def test_engine_with_adapter(dev, name):
    """(3, 2): the adds in front of double blocks 1 and 2 and of single block 0; (3, 0): the last one in the final layer's LayerNorm launch.  35
    image tokens: an odd count on every tile and a partial last workgroup of the new kernel per image.  Scale 0, set-then-cleared and zero V give
    the plain forward's bits; a re-cache replaces the tokens; a shared embedding gives the bits of per-image copies of it."""
    cfg, B, Hl, Wl, S_t = ENGINE[name]
    eng, text, tok = prepared(cfg, dev, B, Hl, Wl, S_t)
    emb = synthetic_embeds(B, IPC.embed_dim)
    plain = eng.forward_tokens(tok, text, 1).clone()
    eng.cache_ip_tokens(tokens_for(eng, emb, dev), per_image=True)
    assert same_bits(eng.forward_tokens(tok, text, 1), plain), "cached, scale still 0"
    eng.set_ip_scale(IP_SCALE)
    out = eng.forward_tokens(tok, text, 1).clone()
    res = oracle(cfg, B, Hl, Wl, S_t)
    moved = rel_l2(res["plain"], res["fp32"])
    e_h, e_e = yardstick_ok(out.float(), res["emu"], res["fp32"], name)
    p_h, p_e = psnr_ok(out.float(), res["emu"], res["fp32"], name)
    print(f"[ip adapter] engine {name}: hip-vs-fp32 {e_h:.3e} (emulation {e_e:.3e}), PSNR {p_h:.1f} dB (emulation {p_e:.1f}); the adapter moves "
          f"the output by {moved:.3e}")
    assert moved >= 10 * (2 * e_e + 2e-3), f"the adapter moves the fp32 oracle's output by {moved:.3e} only: a pass would show nothing"
    assert rel_l2(plain.float(), out.float()) >= 10 * (2 * e_e + 2e-3)
    # scale 0, and set then cleared: the plain forward's bits
    eng.set_ip_scale(0.0)
    assert same_bits(eng.forward_tokens(tok, text, 1), plain)
    eng.set_ip_scale(IP_SCALE)
    eng.set_ip_scale(0.0)
    assert eng.ip_scale == 0.0 and same_bits(eng.forward_tokens(tok, text, 1), plain)
    # a shared embedding against per-image copies of it, and a re-cache
    eng.set_ip_scale(IP_SCALE)
    eng.cache_ip_tokens(tokens_for(eng, emb[:1].repeat(B, 1), dev), per_image=True)
    copied = eng.forward_tokens(tok, text, 1).clone()
    eng.cache_ip_tokens(tokens_for(eng, emb[:1], dev), per_image=False)
    shared = eng.forward_tokens(tok, text, 1).clone()
    assert same_bits(shared, copied) and not same_bits(shared, out)
    eng.cache_ip_tokens(tokens_for(eng, emb, dev), per_image=True)
    assert same_bits(eng.forward_tokens(tok, text, 1), out)


def test_engine_zero_values_give_the_plain_bits(dev):
    """to_v_ip zeroed (weights and biases): every ip_i is zero, x + s * 0 = x -- the whole adapter path runs and changes no bit"""
    cfg, B, Hl, Wl, S_t = ENGINE["3+2"]
    wm, wa = synth_mmdit_weights(cfg, seed=1234), synth_ip_adapter_weights(cfg, IPC, seed=2468)
    wa = {k: (torch.zeros_like(v) if ".to_v_ip." in k else v) for k, v in wa.items()}
    eng, text, tok = prepared(cfg, dev, B, Hl, Wl, S_t, named=(wm, wa))
    plain = eng.forward_tokens(tok, text, 1).clone()
    eng.cache_ip_tokens(tokens_for(eng, synthetic_embeds(B, IPC.embed_dim), dev), per_image=True)
    eng.set_ip_scale(IP_SCALE)
    assert same_bits(eng.forward_tokens(tok, text, 1), plain)


def test_engine_production_width(dev):
    """FLUX.1's width (h 3072, 24 heads of 128, RoPE axes 16 + 56 + 56), main (1, 1), batch 1, latent 4 x 8, S_t 8, the published adapter's N = 4
    tokens of 4096 features: the new kernel on six column chunks, the add at NCH = 6 in single block 0"""
    cfg = replace(FLUX_SCHNELL, depth_multimodal=1, depth_unified=1, token_level_text_embed_dim=256, pooled_text_embed_dim=64)
    ipc = IPAdapterConfig(embed_dim=64)
    assert cfg.hidden_size == 3072 and cfg.num_heads == 24 and (ipc.ip_adapter_tokens, ipc.ip_adapter_dim) == (4, 4096)
    named = (synth_mmdit_weights(cfg, seed=1234), synth_ip_adapter_weights(cfg, ipc, seed=2468))
    eng, text, tok = prepared(cfg, dev, 1, 4, 8, 8, ipc=ipc, named=named)
    eng.cache_ip_tokens(tokens_for(eng, synthetic_embeds(1, ipc.embed_dim), dev), per_image=True)
    eng.set_ip_scale(IP_SCALE)
    out = eng.forward_tokens(tok, text, 1)
    res = oracle(cfg, 1, 4, 8, 8, ipc=ipc, named=named, embed_prec=True)
    e_h, e_e = yardstick_ok(out.float(), res["emu"], res["fp32"], "adapter at width")
    p_h, p_e = psnr_ok(out.float(), res["emu"], res["fp32"], "adapter at width")
    print(f"[ip adapter] at width: hip-vs-fp32 {e_h:.3e} (emulation {e_e:.3e}), PSNR {p_h:.1f} dB (emulation {p_e:.1f})")


def test_workspace_unchanged_without_the_adapter_and_guarded_with_it(dev):
    """without ip_adapter= the workspace size is the plain engine's; with it the engine runs on a NaN-filled interior of exactly the declared size
    and gives the plain run's bits, writes nothing outside, and then a smaller problem in the same (stale) allocation"""
    from diffusionkit_amd.engine import MMDiTEngine
    cfg = tiny_flux(3, 2)
    shapes = [(2, 8, 12, 20), (1, 6, 8, 12)]
    bare = MMDiTEngine(cfg, pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1234), dev))
    eng = build(cfg, dev)
    size = lambda e, s: int(e.lib.dk_mmdit_workspace_bytes(e._h, *s, len(TS)))
    h, nd, N = cfg.hidden_size, cfg.depth_multimodal, IPC.ip_adapter_tokens
    for B, Hl, Wl, S_t in shapes:
        extra = size(eng, (B, Hl, Wl, S_t)) - size(bare, (B, Hl, Wl, S_t))
        want = nd * B * N * 2 * h * 2 + B * (Hl // 2) * (Wl // 2) * h * 2
        assert want <= extra < want + 512, "the K / V cache and one ip buffer, each on a 256-byte boundary"
    nbytes = [size(eng, s) for s in shapes]
    ws = GuardedWorkspace(max(nbytes), dev)
    for k, (B, Hl, Wl, S_t) in enumerate(shapes):
        ref_eng, text, tok = prepared(cfg, dev, B, Hl, Wl, S_t)
        emb = synthetic_embeds(B, IPC.embed_dim)
        ref_eng.cache_ip_tokens(tokens_for(ref_eng, emb, dev), per_image=True)
        ref_eng.set_ip_scale(IP_SCALE)
        ref = ref_eng.forward_tokens(tok, text, 1).clone()
        if k == 0:
            ws.fill(FILL_NAN)
        lend(eng, ws, nbytes[k])
        eng._shape = None
        eng.prepare(B, (Hl, Wl), S_t, len(TS))
        assert eng._ws.numel() == nbytes[k]
        eng.cache_modulation_params(inputs(cfg, B, Hl, Wl, S_t)[1].to(dev), TS)
        eng.cache_ip_tokens(tokens_for(eng, emb, dev), per_image=True)
        eng.set_ip_scale(IP_SCALE)
        out = eng.forward_tokens(tok, text, 1)
        torch.cuda.synchronize()
        assert same_bits(out, ref), f"shape {k}: the guarded run differs from the plain one"
        ws.check(nbytes[k], f"shape {k}: engine with the adapter", fill=FILL_NAN if k == 0 else None)


def test_engine_refusals(dev):
    from diffusionkit_amd import ops
    from diffusionkit_amd._lib import DkHipError
    from diffusionkit_amd.engine import MMDiTEngine
    cfg, B, Hl, Wl, S_t = ENGINE["3+2"]
    eng, text, tok = prepared(cfg, dev, B, Hl, Wl, S_t)
    S_i, h = tok.shape[1], cfg.hidden_size
    emb = synthetic_embeds(B, IPC.embed_dim)
    eng.set_ip_scale(IP_SCALE)
    with pytest.raises(DkHipError, match="needs dk_mmdit_cache_ip_tokens"):
        eng.forward_tokens(tok, text, 1)
    with pytest.raises(DkHipError, match="image-prompt tokens shape"):
        eng.cache_ip_tokens(torch.zeros(B, IPC.ip_adapter_tokens + 1, IPC.ip_adapter_dim, dtype=BF, device=dev), per_image=True)
    eng.cache_ip_tokens(tokens_for(eng, emb, dev), per_image=True)
    ok = eng.forward_tokens(tok, text, 1).clone()
    # the tuning states that leave no raw image queries in QKV, each named by its knob
    try:
        ops.tune("attn_fuse_q", 0)
        with pytest.raises(DkHipError, match="attn_fuse_q"):
            eng.forward_tokens(tok, text, 1)
    finally:
        ops.tune("attn_fuse_q", 1)
    try:
        ops.tune("gemm_fuse_q", 1)
        with pytest.raises(DkHipError, match="gemm_fuse_q"):
            eng.forward_tokens(tok, text, 1)
    finally:
        ops.tune("gemm_fuse_q", -1)
    assert same_bits(eng.forward_tokens(tok, text, 1), ok)
    # "gemm_fuse_q" 1 with the keys' fused tail off finishes nothing: the queries stay raw, the forward runs and meets the oracle
    try:
        ops.tune("gemm_fuse_k", 0)
        ops.tune("gemm_fuse_q", 1)
        res = oracle(cfg, B, Hl, Wl, S_t)
        yardstick_ok(eng.forward_tokens(tok, text, 1).float(), res["emu"], res["fp32"], "gemm_fuse_k 0, gemm_fuse_q 1")
    finally:
        ops.tune("gemm_fuse_q", -1)
        ops.tune("gemm_fuse_k", 1)
    # the entries other than forward, while the adapter is active
    x = torch.zeros(B, S_t + S_i, h, dtype=BF, device=dev)
    with pytest.raises(DkHipError, match="IP-Adapter is active"):
        eng.run_blocks(x, 1, 0)
    with pytest.raises(DkHipError, match="dk_mmdit_forward_head cannot run while the IP-Adapter is active"):
        eng.forward_head(tok, text, 1)
    with pytest.raises(DkHipError, match="dk_mmdit_forward_tail cannot run while the IP-Adapter is active"):
        eng.forward_tail(1, False)
    eng.set_ip_scale(0.0)
    eng.run_blocks(x, 1, 0)
    # what cannot be set beside the adapter
    with pytest.raises(DkHipError, match="IP-Adapter"):
        eng.set_flux_control_taps(torch.zeros(5, B, S_i, h, dtype=BF, device=dev), 3)
    with pytest.raises(DkHipError, match="IP-Adapter"):
        eng.enable_block_cache(True)
    with pytest.raises(DkHipError, match="IP-Adapter"):
        eng.prepare(B, (Hl, Wl), S_t, len(TS), reference_size=(Hl, Wl))
    flat = build(tiny_flux(3, 0), dev)  # (the forks are the SD3 family's by depth_unified == 0: a FLUX model without single blocks reaches the rule)
    with pytest.raises(DkHipError, match="IP-Adapter"):
        flat.set_skip_layers([1], 1)
    with pytest.raises(DkHipError, match="IP-Adapter"):
        flat.set_perturbed_attention([1], 1)
    # engines that cannot take one
    packed = lambda c: {**pack_mmdit(c, synth_mmdit_weights(c, seed=1234), dev)}
    sd3 = tiny_sd3()
    with pytest.raises(DkHipError, match="FLUX family"):
        MMDiTEngine(sd3, packed(sd3), ip_adapter=IPC)
    f8 = fp8_config(cfg, "speed")
    with pytest.raises(DkHipError, match="fp8"):
        MMDiTEngine(f8, packed(f8), ip_adapter=IPC)
    cond = tiny_flux(3, 2, condition_features=64)
    with pytest.raises(DkHipError, match="condition width"):
        MMDiTEngine(cond, packed(cond), ip_adapter=IPC)
    cn = tiny_flux_controlnet(2, 1)
    with pytest.raises(DkHipError, match="ControlNet"):
        MMDiTEngine(cn, packed(cn), ip_adapter=IPC)
    with pytest.raises(DkHipError, match=r"\[1, 16\]"):
        MMDiTEngine(cfg, packed(cfg), ip_adapter=replace(IPC, ip_adapter_tokens=17))
    with pytest.raises(DkHipError, match="stacked"):
        MMDiTEngine(cfg, packed(cfg), ip_adapter=IPC)
    # the C entries themselves (the host validates first: these are reached through the library)
    lib = eng.lib
    bare = MMDiTEngine(cfg, packed(cfg))
    assert lib.dk_mmdit_set_ip_scale(bare._h, 0.5) != 0 and b"needs an IP-Adapter" in lib.dk_last_error()
    bare.prepare(B, (Hl, Wl), S_t, len(TS))
    assert lib.dk_mmdit_set_ip_adapter(bare._h, 4, 256) != 0 and b"before the weights are resolved" in lib.dk_last_error()
    fresh = MMDiTEngine(sd3, packed(sd3))
    assert lib.dk_mmdit_set_ip_adapter(fresh._h, 4, 256) != 0 and b"SD3 geometry is refused" in lib.dk_last_error()
    fresh = MMDiTEngine(cfg, packed(cfg))
    assert lib.dk_mmdit_set_ip_adapter(fresh._h, 17, 256) != 0 and b"between 1 and 16" in lib.dk_last_error()
    assert lib.dk_mmdit_set_ip_adapter(fresh._h, 4, 256) == 0
    with pytest.raises(DkHipError, match="weight not bound: ip_adapter.0.to_k_ip.weight"):
        fresh.prepare(B, (Hl, Wl), S_t, len(TS))


# ---- step loop and pipeline -----------------------------------------------------------------------------------------------------------
STEPS, HL_P, WL_P, SCALE_P = 3, 8, 16, 0.8
PIPE_MAIN = tiny_flux(3, 2)
_PIPES = {}


def pipe_for(dev, adapter=True, ckpt=None):
    """one tiny FLUX pipeline with the adapter (from this project's tensor names, or from ``ckpt``) and one without, for the whole module"""
    from diffusionkit_amd.config import tiny_vae, tiny_vae_encoder
    from diffusionkit_amd.pipeline import FluxPipeline
    key = (adapter, ckpt)
    if key not in _PIPES:
        kw = dict(ip_adapter_ckpt=ckpt or synth_ip_adapter_weights(PIPE_MAIN, IPC, seed=2468), ip_adapter_config=IPC) if adapter else {}
        _PIPES[key] = FluxPipeline(w16=True, a16=True, mmdit_config=PIPE_MAIN, vae_config=tiny_vae(), vae_encoder_config=tiny_vae_encoder(), device=dev,
                                   text_len=16, **kw)
    return _PIPES[key]


def pipe_inputs():
    return randn(1, 16, PIPE_MAIN.token_level_text_embed_dim, seed=7), randn(1, PIPE_MAIN.pooled_text_embed_dim, seed=8)


def sampled(pipe, dev, seed=0, **kw):
    text, pooled = pipe_inputs()
    n = len(seed) if isinstance(seed, list) else 1
    lat, iter_time = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=STEPS, cfg_weight=0.0, latent_size=(HL_P, WL_P), seed=seed, **kw)
    assert lat.shape == (n, HL_P, WL_P, 16) and lat.dtype == torch.float32
    return lat


def loop_references(embed, seed=0, sampler="euler"):
    """the oracle with the adapter as the model of the restated step loop (tests/test_samplers_cpu.py's ``plan_loop``), on the fp32 and the
    bf16-emulating oracle, after process_out; ``embed``: [1, E]"""
    from oracle import pipeline as op
    from tests.test_samplers_cpu import plan_loop, start_state
    text, pooled = pipe_inputs()
    wm = {k: v.float() for k, v in synth_mmdit_weights(PIPE_MAIN, seed=1234).items()}
    wa = {k: v.float() for k, v in synth_ip_adapter_weights(PIPE_MAIN, IPC, seed=2468).items()}
    sigmas = op.get_sigmas(1.0, True, STEPS)
    res = {}
    for name, P in (("fp32", Prec()), ("emu", Prec(BF))):
        m = IPAdapterFluxOracle(PIPE_MAIN, wm, P)
        m.ip = (wa, IPC, embed, SCALE_P)
        x0, _ = start_state(sigmas, seed, HL_P, WL_P)
        res[name] = op.process_out(plan_loop(m, sampler, x0, sigmas, text, pooled, 0.0, Prec(BF)), "flux")
    return res


def parity(lat, res, what):
    e_h, e_e = yardstick_ok(lat, res["emu"], res["fp32"], what)
    p_h, p_e = psnr(res["fp32"], lat), psnr(res["fp32"], res["emu"])
    print(f"[ip adapter] {what}: hip-vs-fp32 {e_h:.3e} (emulation {e_e:.3e}), PSNR hip {p_h:.1f} dB / emu {p_e:.1f} dB")
    assert p_h > 35.0, f"{what}: PSNR {p_h:.1f} dB"


def test_pipeline_from_an_xlabs_layout_file(dev, tmp_path):
    """3 Euler steps, tiny VAE, the adapter loaded from a file in XLabs-AI's layout: the final latent against the oracle loop, the bits of the same
    weights handed over by name, and -- with scale 0 -- the bits of a pipeline without an adapter"""
    import os
    from safetensors.torch import save_file
    path = os.path.join(tmp_path, "ip_adapter.safetensors")
    save_file(IP.to_xlabs_ip_adapter(synth_ip_adapter_weights(PIPE_MAIN, IPC, seed=2468), PIPE_MAIN), path)
    pipe, emb = pipe_for(dev, ckpt=path), synthetic_embeds(2, IPC.embed_dim)
    assert pipe.mmdit.ip_adapter is IPC
    lat = sampled(pipe, dev, ip_adapter_image_embeds=emb[0].numpy(), ip_adapter_scale=SCALE_P)
    assert pipe.last_ip_adapter == {"scale": SCALE_P, "tokens": IPC.ip_adapter_tokens, "images": 1} and pipe.mmdit.ip_scale == 0.0
    parity(lat, loop_references(emb[:1]), "pipeline, euler")
    named = pipe_for(dev)
    assert same_bits(lat, sampled(named, dev, ip_adapter_image_embeds=emb[:1], ip_adapter_scale=SCALE_P))
    plain = sampled(pipe_for(dev, adapter=False), dev)
    assert not same_bits(lat, plain) and rel_l2(plain, lat) > 0.05
    assert same_bits(sampled(named, dev, ip_adapter_image_embeds=emb[:1], ip_adapter_scale=0.0), plain)


def test_pipeline_heun(dev):
    """--sampler heun: two model evaluations per step but the last, every one with the adapter"""
    pipe, emb = pipe_for(dev), synthetic_embeds(2, IPC.embed_dim)
    lat = sampled(pipe, dev, sampler="heun", ip_adapter_image_embeds=emb[:1], ip_adapter_scale=SCALE_P)
    assert pipe.last_sampler["model_evals"] == 5
    parity(lat, loop_references(emb[:1], sampler="heun"), "heun")


def test_pipeline_two_seeds_two_embeddings(dev):
    """seed = [2, 3] with one embedding each: every image against its own oracle loop; swapped embeddings change the bits"""
    pipe, emb = pipe_for(dev), synthetic_embeds(2, IPC.embed_dim)
    both = sampled(pipe, dev, seed=[2, 3], ip_adapter_image_embeds=[emb[0], emb[1]], ip_adapter_scale=SCALE_P)
    assert pipe.last_ip_adapter["images"] == 2
    for i, s in enumerate((2, 3)):
        parity(both[i:i + 1], loop_references(emb[i:i + 1], seed=s), f"seed {s} with its embedding")
    swapped = sampled(pipe, dev, seed=[2, 3], ip_adapter_image_embeds=emb.flip(0), ip_adapter_scale=SCALE_P)
    assert not same_bits(both, swapped)


def test_pipeline_img2img_inpainting(dev):
    """img2img from an encoded image with a half mask: scale 0 gives the bits of the same call on a pipeline without the adapter, a nonzero scale
    moves the repainted half and leaves the kept half what the blend makes it"""
    from tests.test_gpu_inpaint import HALF, RGB
    with_ip, without = pipe_for(dev), pipe_for(dev, adapter=False)
    text, pooled = pipe_inputs()
    call = lambda p, **c: p.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=4, cfg_weight=0.0, latent_size=(HL_P, WL_P), seed=2,
                                            image_path=RGB, denoise=0.75, mask_path=HALF, **c)[0]
    emb = synthetic_embeds(1, IPC.embed_dim)
    plain = call(without)
    off = call(with_ip, ip_adapter_image_embeds=emb, ip_adapter_scale=0.0)
    on = call(with_ip, ip_adapter_image_embeds=emb, ip_adapter_scale=SCALE_P)
    assert bool(torch.isfinite(on).all()) and same_bits(off, plain)
    assert same_bits(on[:, :, :WL_P // 2], plain[:, :, :WL_P // 2]), "the kept half of the latent"
    assert rel_l2(plain[:, :, WL_P // 2:], on[:, :, WL_P // 2:]) > 0.05, "the repainted half"


def test_pipeline_refusals_on_the_device(dev):
    from diffusionkit_amd.config import tiny_vae
    from diffusionkit_amd.pipeline import DiffusionPipeline, FluxPipeline
    pipe, emb = pipe_for(dev), synthetic_embeds(1, IPC.embed_dim)
    text, pooled = pipe_inputs()
    run = lambda p, **kw: p.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=2, latent_size=(HL_P, WL_P), seed=0, **kw)
    with pytest.raises(ValueError, match="needs ip_adapter_image_embeds in every call"):
        run(pipe)
    with pytest.raises(ValueError, match="need a pipeline built with an IP-Adapter"):
        run(pipe_for(dev, adapter=False), ip_adapter_image_embeds=emb)
    with pytest.raises(ValueError, match="cfg_weight > 0"):
        run(pipe, ip_adapter_image_embeds=emb, cfg_weight=3.0)
    with pytest.raises(ValueError, match="block_cache"):
        run(pipe, ip_adapter_image_embeds=emb, block_cache=0.1)
    with pytest.raises(ValueError, match="reference_image_path"):
        run(pipe, ip_adapter_image_embeds=emb, reference_image_path=torch.zeros(64, 128, 3, dtype=torch.uint8).numpy())
    kw = dict(w16=True, a16=True, vae_config=tiny_vae(), device=dev, text_len=16, ip_adapter_ckpt=synth_ip_adapter_weights(PIPE_MAIN, IPC, seed=2468),
              ip_adapter_config=IPC)
    with pytest.raises(ValueError, match="FLUX family's"):
        DiffusionPipeline(mmdit_config=tiny_sd3(), **kw)
    with pytest.raises(ValueError, match="fp8"):
        FluxPipeline(mmdit_config=fp8_config(PIPE_MAIN, "speed"), **kw)
    with pytest.raises(ValueError, match="condition="):
        FluxPipeline(mmdit_config=PIPE_MAIN, condition="control", **kw)
    with pytest.raises(ValueError, match="controlnet_ckpt"):
        FluxPipeline(mmdit_config=PIPE_MAIN, controlnet_ckpt={"x": 1}, controlnet_config=tiny_flux_controlnet(2, 1), **kw)
