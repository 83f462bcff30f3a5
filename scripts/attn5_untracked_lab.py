"""attention5's two generated bodies against each other, per launch: the tracked tile loop (dk_tune_set("attn_track", 1): the running row maximum
and the deferred rescale) and the untracked one (a score bound from the caller, one exponent offset per row), through ops.attention with the fused
query load (an identity RoPE table: the queries stay what they are) -- the only instantiation the untracked body is built for.

Shapes: FLUX.1-schnell's 24 heads x 4352 tokens (408 workgroups: two rounds of 256 CUs), and two ONE-round launches of 256 workgroups with 32 and 64
key tiles, whose difference gives the time per tile and the cost per workgroup (profiles/NOTES_r05.md section 7).  The bodies alternate: three
rounds to warm up (the clock settles over the first hundred launches), then ROUNDS (5) rounds of twenty launches each; prints every round, then
mean, min and max per body."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from diffusionkit_amd import ops

dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(0)
BF, D = torch.bfloat16, 128
ROUNDS, WARM, N = int(os.environ.get("ROUNDS", "5")), 3, 20
shapes = [("FLUX schnell 24 x 4352", 1, 24, 4352), ("one round, 32 tiles (32 x 2048)", 1, 32, 2048), ("one round, 64 tiles (16 x 4096)", 1, 16, 4096)]
res = {}
for name, B, H, S in shapes:
    qkv = torch.randn(B, S, 3 * H * D, device=dev, generator=g).to(BF)
    h = H * D
    q, k = (qkv[0, :, i * h:i * h + D].float() for i in range(2))
    bound = float((q @ k.t()).abs().max()) / D ** 0.5 * 1.5  # head 0's largest score with a margin for the other heads; far below the 22.18 the route admits
    rope = torch.zeros(S, D // 2, 2, device=dev)
    rope[..., 0] = 1.0
    qn = (None, None, 0, rope)
    plan = dict(q=1 << 28, k=(1 << 28) + 2 * h, v=(1 << 28) + 4 * h, out=1 << 29, B=B, H=H, S=S, D=D, ld=3 * h, ldo=h, scale=D ** -0.5, q_rope=1 << 30, score_bound=bound)
    times, outs = {0: [], 1: []}, {}
    for rnd in range(WARM + ROUNDS):  # (the first WARM rounds are not counted)
        for track in (1, 0):
            ops.tune("attn_track", track)
            if rnd == 0:
                assert ops.attention_plan(workspace_bytes=0, **plan).untracked == 1 - track
            outs[track] = ops.attention(qkv, H, D, score_bound=bound, qn=qn)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(N):
                ops.attention(qkv, H, D, score_bound=bound, qn=qn)
            e1.record()
            torch.cuda.synchronize()
            if rnd >= WARM:
                times[track].append(e0.elapsed_time(e1) * 1000.0 / N)  # us per launch
    ops.tune("attn_track", -1)
    d = float((outs[0].float() - outs[1].float()).abs().max())
    fl = 4.0 * B * H * S * S * D
    for track in (1, 0):
        t = times[track]
        res[(name, track)] = sum(t) / len(t)
        print(f"{name}: {'tracked  ' if track else 'untracked'} us per launch {' '.join(f'{x:7.1f}' for x in t)} | mean {sum(t) / len(t):7.1f} min {min(t):7.1f} max {max(t):7.1f}"
              f" | {fl / (sum(t) / len(t)) / 1e6:6.0f} TF", flush=True)
    t1, t0 = times[1], times[0]
    gain, spread = sum(t1) / len(t1) - sum(t0) / len(t0), max(t1) - min(t1)
    print(f"{name}: bound {bound:.2f}; tracked - untracked {gain:6.1f} us ({100 * gain / (sum(t1) / len(t1)):.1f} %), spread of the tracked runs {spread:.1f} us -> "
          f"{'a gain' if gain > 2 * spread else 'NOT a gain by the 2 x spread rule'}; |tracked - untracked| max {d:.2e}, bit-identical: {torch.equal(outs[0], outs[1])}", flush=True)
for track in (1, 0):
    a, b = res[(shapes[1][0], track)], res[(shapes[2][0], track)]
    print(f"{'tracked  ' if track else 'untracked'}: {(b - a) / 32:.3f} us per tile, {a - 32 * (b - a) / 32:.1f} us per workgroup (one round of 256 workgroups, 64 against 32 key tiles)", flush=True)
