"""attention5.hip's tile loop WITHOUT the running row maximum (dk_attention_desc.score_bound; dk_attn5_fwd_kernel<true, true>) on the MI355X: against
the oracle, the fp64 softmax and the tracked body (dk_tune_set("attn_track", 1)) of the same launch -- whole blocks, bounded spikes, the key-split
jobs + merge, and inside the engine, where the bound comes from the QKNorm weights.

The untracked body is built for the fused query load only; the operator tests pass an identity RoPE table (cos 1, sin 0: the queries stay bit for bit
what they are), so the oracle sees the same q, k, v as the kernel."""
import math
from dataclasses import replace

import pytest
import torch

from oracle import mmdit as om
from oracle.mmdit import Prec
from tests._util import BF, bf16r, max_abs, randn, rel_l2

pytestmark = pytest.mark.gpu

D = 128
B_ADMITTED = 32.0 / math.log2(math.e)  # 2 B log2(e) <= 64 (attention.hip)


def measured_bound(qkv, H):
    """max |scale q.k| over every batch row and head, on the CPU, times the 2 % the engine's bound carries for the roundings"""
    h, worst = H * D, 0.0
    for b in range(qkv.shape[0]):
        for i in range(H):
            q, k = qkv[b, :, i * D:(i + 1) * D].double(), qkv[b, :, h + i * D:h + (i + 1) * D].double()
            worst = max(worst, float((q @ k.t()).abs().max()) / math.sqrt(D))
    return worst * 1.02


def run(qkv, H, dev, bound, track, split=-1):
    """one launch of kernel 10 with the fused (identity) query load under the knobs; returns the output and the plan of that launch"""
    from diffusionkit_amd import _lib, ops
    Bn, S, _ = qkv.shape
    h = H * D
    rope = torch.zeros(S, D // 2, 2, device=dev)
    rope[..., 0] = 1.0
    x = qkv.to(dev, BF).contiguous()
    desc = dict(q=x, k=x[:, :, h:], v=x[:, :, 2 * h:], out=x, B=Bn, H=H, S=S, D=D, ld=3 * h, ldo=h, scale=1.0 / math.sqrt(D), q_rope=rope, score_bound=bound)
    try:
        ops.tune("attn", 10)
        ops.tune("attn_track", track)
        ops.tune("attn_split", split)
        plan = ops.attention_plan(workspace_bytes=_lib.load().dk_attention_workspace_bytes(), **desc)
        y = ops.attention(x, H, D, score_bound=bound, qn=(None, None, 0, rope))
        torch.cuda.synchronize()
    finally:
        ops.tune("attn", -1)
        ops.tune("attn_track", -1)
        ops.tune("attn_split", -1)
    assert plan.kernel == 10 and plan.qfuse == 1
    return y, plan


def rows_the_tracked_body_moves(qkv, H):
    """rows whose exponent offset the TRACKED body moves behind the first tile (a later tile's maximum exceeds it by more than the threshold 4):
    the rows on which the two bodies can differ at all -- on every other row both keep the first tile's maximum and are bit-identical"""
    h, S, n = H * D, qkv.shape[1], 0
    for b in range(qkv.shape[0]):
        for i in range(H):
            s = qkv[b, :, i * D:(i + 1) * D].double() @ qkv[b, :, h + i * D:h + (i + 1) * D].double().t() / math.sqrt(D)
            tm = s.reshape(S, S // 64, 64).max(-1).values
            mc, moved = tm[:, 0].clone(), torch.zeros(S, dtype=torch.bool)
            for t in range(1, S // 64):
                m = tm[:, t] - mc > 4.0
                mc, moved = torch.where(m, tm[:, t], mc), moved | m
            n += int(moved.sum())
    return n


@pytest.mark.parametrize("B,H,S", [(1, 2, 768), (2, 3, 1024)])
def test_untracked_body_against_the_oracle_and_the_tracked_body(dev, B, H, S):
    """768 keys = 12 tiles (one pass of the four-tile loop + the eight peeled tiles), 1024 = two passes; test_attention5_one_wave_per_simd's inputs with
    q and k scaled by sqrt(2) each (scores x 2: maxima of 10 - 11, so that the tracked body does move the offset of some rows -- with the plain inputs
    it moves none, and the two bodies are bit-identical) and v by 1 / 4 (outputs below 1, as in that test: its 4e-3 between two kernel bodies is one bf16
    ulp of an output below 1).  That test's tolerances for the same two comparisons: oracle 6e-3 / 0.03, the other body 4e-3.  The bound handed over
    is the measured one."""
    h = H * D
    qkv = randn(B, S, 3 * h, seed=33)
    qkv[..., :2 * h] = bf16r(qkv[..., :2 * h] * math.sqrt(2.0))
    qkv[..., 2 * h:] = bf16r(qkv[..., 2 * h:] * 0.25)
    bound = measured_bound(qkv, H)
    moved = rows_the_tracked_body_moves(qkv, H)
    print(f"[untracked] B {B} H {H} S {S}: max |scale q.k| * 1.02 = {bound:.3f}; the tracked body moves the offset of {moved} rows")
    assert bound <= 22.0 and moved >= 16
    outs = {}
    for track in (1, 0):
        outs[track], plan = run(qkv, H, dev, bound, track)
        assert plan.untracked == 1 - track
    q, k, v = (qkv[..., i * h:(i + 1) * h].reshape(B, S, H, D).transpose(1, 2) for i in range(3))
    ref = om.sdpa(q, k, v, 1.0 / math.sqrt(D), Prec()).transpose(1, 2).reshape(B, S, h)
    worst = max_abs(outs[1].float(), outs[0].float())
    print(f"[untracked] vs oracle rel-L2 {rel_l2(ref, outs[0].float()):.3e} (tracked {rel_l2(ref, outs[1].float()):.3e}), max {max_abs(ref, outs[0].float()):.3e}, "
          f"max |out| {float(ref.abs().max()):.3f}; tracked vs untracked worst |diff| {worst:.3e}, bit-identical {torch.equal(outs[0], outs[1])}")
    assert float(ref.abs().max()) < 1.0
    assert rel_l2(ref, outs[0].float()) < 6e-3
    assert max_abs(ref, outs[0].float()) < 0.03
    assert worst < 4e-3
    assert not torch.equal(outs[0], outs[1])  # (the knob does select another body)


def test_untracked_body_with_bounded_spikes(dev):
    """test_attention5_spiked_key_forces_rescale's case inside the admitted range: keys 700 and 1023 aligned with queries 7 and 300, the factor chosen so
    that their scores are 20 -- far above the rows' first-tile maxima (~1), where the offset stays; fp64 reference, that test's tolerance"""
    S = 1024
    qkv = randn(1, S, 3 * D, seed=31, scale=0.5)
    for key, qrow in ((700, 7), (1023, 300)):
        f = 20.0 * math.sqrt(D) / float(qkv[0, qrow, :D].double().pow(2).sum())
        qkv[0, key, D:2 * D] = bf16r(qkv[0, qrow, :D] * f)
    bound = measured_bound(qkv, 1)
    print(f"[untracked] spikes: max |scale q.k| * 1.02 = {bound:.3f}")
    assert 19.0 < bound <= 22.0
    q, k, v = (qkv[..., i * D:(i + 1) * D].double() for i in range(3))
    p = torch.softmax(q[0] @ k[0].t() / math.sqrt(D), dim=-1)
    ref = (p @ v[0])[None]
    assert float(p[7, 700]) > 0.9 and float(p[300, 1023]) > 0.9
    y, plan = run(qkv, 1, dev, bound, 0)
    assert plan.untracked == 1
    print(f"[untracked] spikes: rel-L2 vs fp64 {rel_l2(ref, y.float()):.3e}")
    assert torch.isfinite(y.float()).all()
    assert rel_l2(ref, y.float()) < 6e-3


def test_untracked_key_split_jobs_and_merge(dev):
    """attn_split 2 at S = 3072: every block's two key ranges run the untracked body from the first tile of THEIR range and leave that offset; the merge
    weights the partials by it (a bounded spike in the second range: the ranges end at offsets ~19 apart).  Against the unsplit untracked launch and the
    oracle, with test_attention5_key_split_of_the_last_round's tolerances."""
    B, H, S = 1, 2, 3072
    h = H * D
    qkv = randn(B, S, 3 * h, seed=34, scale=0.7)
    f = 20.0 * math.sqrt(D) / float(qkv[0, 77, :D].double().pow(2).sum())
    qkv[0, 3000, h:h + D] = bf16r(qkv[0, 77, :D] * f)  # key 3000 aligned with query 77 of head 0
    bound = measured_bound(qkv, H)
    assert 19.0 < bound <= 22.0
    outs = {}
    for split in (0, 2):
        outs[split], plan = run(qkv, H, dev, bound, 0, split=split)
        assert plan.untracked == 1 and plan.split == max(split, 1) and plan.merge == (split > 1)
    q, k, v = (qkv[..., i * h:(i + 1) * h].reshape(B, S, H, D).transpose(1, 2) for i in range(3))
    ref = om.sdpa(q, k, v, 1.0 / math.sqrt(D), Prec()).transpose(1, 2).reshape(B, S, h)
    print(f"[untracked] key split: rel-L2 vs oracle {rel_l2(ref, outs[2].float()):.3e} (unsplit {rel_l2(ref, outs[0].float()):.3e}), "
          f"split vs unsplit {max_abs(outs[0].float(), outs[2].float()):.3e}")
    assert rel_l2(ref, outs[2].float()) < 6e-3 and rel_l2(ref, outs[0].float()) < 6e-3
    assert not torch.equal(outs[0], outs[2])  # (the switch does select the split launch: the partials are rounded to bf16)
    assert max_abs(outs[0].float(), outs[2].float()) < 0.02 * float(ref.abs().max()) + 4e-3


def test_engine_passes_the_bound_of_its_norm_weights(dev):
    """FLUX width, depth 1 + 1, latent 96 x 96 (S = 256 + 2304 = 2560: kernel 10, fused query load): the engine reads its QKNorm weights once and
    hands every joint attention launch max|w_q| max|w_k| sqrt(D) 1.02 -- dk_mmdit_score_bound reports it, the plan of that launch names the untracked body, and
    dk_tune_set("attn_track", 1) runs the tracked one.  Both forwards agree within the width tests' tolerance for a switched path
    (test_fused_key_norm_matches_separate_pass)."""
    from diffusionkit_amd import _lib, ops
    from diffusionkit_amd.config import FLUX_SCHNELL
    from diffusionkit_amd.engine import MMDiTEngine
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    cfg = replace(FLUX_SCHNELL, depth_multimodal=1, depth_unified=1)
    named = synth_mmdit_weights(cfg, seed=1234)
    eng = MMDiTEngine(cfg, pack_mmdit(cfg, named, dev))
    side, S_t = 96, 256
    S = S_t + (side // 2) ** 2
    assert S == 2560
    text = randn(1, S_t, cfg.token_level_text_embed_dim, seed=3)
    pooled = randn(1, cfg.pooled_text_embed_dim, seed=4)
    lat = randn(1, side, side, 16, seed=5)
    eng.prepare(1, (side, side), S_t, 2)
    eng.cache_modulation_params(pooled.to(dev), [1000.0, 752.0])
    tok = eng.patchify(lat.to(dev))
    # the bound the engine arrived at, per launch, against the weights, and the plan of that launch
    wmax = lambda stem, which: float(named[f"{stem}.qk_norm.{which}_norm.weight"].to(BF).float().abs().max())
    dbl = [f"multimodal_transformer_blocks.0.{s}_transformer_block" for s in ("image", "text")]
    sgl = ["unified_transformer_blocks.0.transformer_block"]
    h = cfg.num_heads * D
    for stems, split, kind in ((dbl, S_t, 0), (sgl, 0, 2)):
        want = max(wmax(s, "q") for s in stems) * max(wmax(s, "k") for s in stems) * math.sqrt(D) * 1.02
        bound = eng.score_bound(kind, 0)
        print(f"[untracked] engine: block kind {kind}: bound {bound:.4f} (from the weights: {want:.4f})")
        assert abs(bound - want) <= 1e-5 * want and 0.0 < bound <= B_ADMITTED
        p = ops.attention_plan(workspace_bytes=_lib.load().dk_attention_workspace_bytes(), q=1 << 28, k=(1 << 28) + 2 * h, v=(1 << 28) + 4 * h, out=1 << 29,
                               B=1, H=cfg.num_heads, S=S, D=D, ld=3 * h, ldo=h, scale=1.0 / math.sqrt(D), qn_a=1 << 30, qn_b=(1 << 30) + 256, qn_split=split,
                               qn_eps=1e-6, q_rope=1 << 31, score_bound=bound)
        assert (p.kernel, p.qfuse, p.untracked) == (10, 1, 1), (stems, bound)
    assert eng.score_bound(0, 1) == 0.0 and eng.score_bound(1, 0) == 0.0  # (no such block / no such kind)
    outs = {}
    try:
        for track in (-1, 1):
            ops.tune("attn_track", track)
            outs[track] = eng.forward_tokens(tok, text.to(dev, BF), 1).float().cpu()
    finally:
        ops.tune("attn_track", -1)
    auto, ref = outs[-1], outs[1]
    d = (auto - ref).abs()
    print(f"[untracked] engine: automatic vs tracked rel-L2 {rel_l2(ref, auto):.3e}, worst |diff| {float(d.max()):.3e} of max |out| {float(ref.abs().max()):.3f}")
    assert torch.isfinite(auto).all()
    assert rel_l2(ref, auto) < 8e-3
    assert float(d.max()) <= 0.05 * float(ref.abs().max())
    # (bit-identical is the expected outcome here: QK-normed random activations give scores of N(0, 1), no row's maximum moves by the threshold, and on
    #  such rows the two bodies compute the same bits -- test_untracked_body_against_the_oracle_and_the_tracked_body is where they differ)
