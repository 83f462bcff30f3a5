"""What the FLUX IP-Adapter costs (synthetic weights, times only), batch 1, N = 4 tokens of 4096 features, 512^2 and 1024^2, in one process:

  (a) one model evaluation of the FLUX.1-dev preset (dk_mmdit_forward with the context hoisted), plain;
  (b) the same with the adapter at scale 1: 19 launches of dk_ip_attention_bf16 more, and 19 LayerNorm launches that add its output;
  (k) the new launch alone (dk_ip_attention_bf16 called through ctypes on a QKV buffer of the evaluation's shape and a preallocated output, 200
      back-to-back calls between two events), beside the time its bytes -- q read, ip written -- take at the chip's streaming rate;
  (c) ``cache_ip_tokens``, once per call.

The rows alternate inside every repeat.

    python scripts/ip_adapter_time.py --commit HASH [--out profiles/ip_adapter.md]
    python scripts/ip_adapter_time.py --plain-only [--tree OTHER_TREE]     # (a) alone, one JSON line: for alternating two builds in one visit
    python scripts/ip_adapter_time.py --kernel-only                        # (k) alone, its table on stdout: no model is built

One process, no retries: a failure ends the run.  No checkpoint has been run: the weights and operands are random."""
import argparse
import json
import os
import sys

import numpy as np

S_T = 512
WARM, EVALS, REPEATS = 2, 4, 5
SIDES = (64, 128)  # latent cells: 512^2 and 1024^2 pixels
STREAM_TBS = 6.3   # the HBM rate a streaming copy reaches on this chip (profiles/flux_controlnet.md uses the same figure)


def measure(args):
    import torch
    from diffusionkit_amd.config import FLUX_DEV as cfg
    from diffusionkit_amd.engine import MMDiTEngine
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    BF = torch.bfloat16

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def rounds(fns, evals):
        for fn in fns.values():
            timed(fn, WARM)
        t = {name: [] for name in fns}
        for _ in range(REPEATS):  # (alternating: drift of the box lands on every row alike)
            for name, fn in fns.items():
                t[name].append(timed(fn, evals))
        return {k: float(np.median(v)) for k, v in t.items()}, {k: (min(v), max(v)) for k, v in t.items()}

    h, N_TOK = cfg.hidden_size, 4

    def kernel_row(side):
        """(k): the table row of the launch alone at latent side ``side``"""
        from diffusionkit_amd import _lib
        lib = _lib.load()
        S_i = (side // cfg.patch_size) ** 2
        qkv = torch.randn(1, S_T + S_i, 3 * h, generator=g).to(dev, BF)
        qn = torch.ones(cfg.head_dim, dtype=BF, device=dev)
        kv = torch.randn(1, N_TOK, 2 * h, generator=g).to(dev, BF)
        out = torch.empty(S_i, h, dtype=BF, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        args = (qkv.data_ptr(), 3 * h, S_i, S_T + S_i, S_T, qn.data_ptr(), kv.data_ptr(), kv.data_ptr() + 2 * h, 2 * h, 1, N_TOK, h, cfg.head_dim,
                cfg.head_dim ** -0.5, 1e-6, out.data_ptr(), stream)

        def kernel():
            _lib.check(lib.dk_ip_attention_bf16(*args), "dk_ip_attention_bf16")

        kmed, kspan = rounds({"k": kernel}, 200)
        nbytes = 2 * S_i * h * 2
        at = nbytes / (STREAM_TBS * 1e12) * 1e6
        return (f"| {side * 8}^2 | {S_i} | {1e3 * kmed['k']:.1f} ({1e3 * kspan['k'][0]:.1f} - {1e3 * kspan['k'][1]:.1f}) | {nbytes / 1e6:.1f} | {at:.1f} | "
                f"{1e3 * kmed['k'] / at:.2f} |")

    second = ["", "## The new launch alone", "",
              f"(k) `dk_ip_attention_bf16` through ctypes on a [1, {S_T} + S_i, 3 h] QKV buffer and a preallocated output, h = {h}, 200 back-to-back calls between two "
              f"events; *bytes*: the q columns of the image rows read and the output written, 2 S_i h 2 bytes (K and V, {2 * N_TOK * h * 2 / 1024:.0f} KiB, stay in cache); "
              f"*at {STREAM_TBS} TB/s*: those bytes at the rate a streaming copy reaches on this chip.", "",
              f"| image | S_i | (k) us (min - max) | bytes MB | at {STREAM_TBS} TB/s us | (k) / that |", "|---|---|---|---|---|---|"]
    if args.kernel_only:
        print("\n".join(second + [kernel_row(side) for side in SIDES]))
        return

    packed = pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1234, device=dev), dev, consume=True)
    text = torch.randn(1, S_T, cfg.token_level_text_embed_dim, generator=g).to(dev, BF)
    pooled = torch.randn(1, cfg.pooled_text_embed_dim, generator=g).to(dev, BF)

    def prepared(eng, side):
        eng.prepare(1, (side, side), S_T, 1)
        eng.cache_modulation_params(pooled, [1000.0])
        eng.cache_context(text)

    if args.plain_only:
        main = MMDiTEngine(cfg, packed)
        res = {}
        for side in SIDES:
            prepared(main, side)
            tok = main.patchify(torch.randn(1, side, side, 16, generator=g).to(dev))
            out = torch.empty_like(tok)
            med, span = rounds({"plain": lambda: main.forward_tokens(tok, None, 0, tokens_out=out)}, EVALS)
            res[f"{side * 8}^2"] = {"ms": round(med["plain"], 4), "min": round(span["plain"][0], 4), "max": round(span["plain"][1], 4)}
        print(json.dumps({"tree": args.label, "plain_evaluation": res}))
        return

    from diffusionkit_amd.config import FLUX_IP_ADAPTER as ipc
    from diffusionkit_amd.engine import ip_adapter_project
    from diffusionkit_amd.weights import pack_ip_adapter, synth_ip_adapter_weights
    packed.update(pack_ip_adapter(cfg, ipc, synth_ip_adapter_weights(cfg, ipc, seed=2468, device=dev), dev))
    main = MMDiTEngine(cfg, packed, ip_adapter=ipc)
    nd, N = cfg.depth_multimodal, ipc.ip_adapter_tokens
    tokens = ip_adapter_project(main.weights, ipc, torch.randn(1, ipc.embed_dim, generator=g))
    lines = ["# FLUX IP-Adapter: what the decoupled attention launch and the adapter cost", "",
             f"Commit {args.commit}; {torch.cuda.get_device_name(0)}; synthetic weights and operands, bf16, batch 1, text length {S_T}, N = {N} tokens of "
             f"{ipc.ip_adapter_dim} features; medians of {REPEATS} repeats of {EVALS} evaluations,",
             "the rows of a table alternating inside every repeat, HIP events around back-to-back calls in one process (`scripts/ip_adapter_time.py`).",
             "Nothing here is gated.  No checkpoint has been run.", "",
             "## One model evaluation, FLUX.1-dev preset", "",
             f"(a) `dk_mmdit_forward`, context hoisted, adapter set with scale 0 (the plain launches); (b) the same at scale 1: {nd} `dk_ip_attention_bf16` launches more and "
             f"{nd} LayerNorm launches with the add; (c) `dk_mmdit_cache_ip_tokens`, once per call.", "",
             "| image | (a) plain ms (min - max) | (b) with the adapter ms (min - max) | (b) - (a) ms | per double block us | (b) / (a) | (c) cache ms |",
             "|---|---|---|---|---|---|---|"]
    for side in SIDES:
        prepared(main, side)
        tok = main.patchify(torch.randn(1, side, side, 16, generator=g).to(dev))
        out = torch.empty_like(tok)
        main.cache_ip_tokens(tokens, per_image=False)

        def plain():
            main.set_ip_scale(0.0)
            main.forward_tokens(tok, None, 0, tokens_out=out)

        def adapted():
            main.set_ip_scale(1.0)
            main.forward_tokens(tok, None, 0, tokens_out=out)

        def cache():
            main.cache_ip_tokens(tokens, per_image=False)

        med, span = rounds({"a": plain, "b": adapted, "c": cache}, EVALS)
        main.set_ip_scale(0.0)
        cell = lambda k: f"{med[k]:.2f} ({span[k][0]:.2f} - {span[k][1]:.2f})"  # noqa: E731
        extra = med["b"] - med["a"]
        lines.append(f"| {side * 8}^2 | {cell('a')} | {cell('b')} | {extra:.3f} | {1e3 * extra / nd:.1f} | {med['b'] / med['a']:.4f} | {med['c']:.3f} |")
        second.append(kernel_row(side))
    text_out = "\n".join(lines + second) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text_out)


if __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(here, "profiles", "ip_adapter.md"))
    ap.add_argument("--commit", default="unknown", help="stamp of the tree that runs (the caller knows it; a copy without .git does not)")
    ap.add_argument("--plain-only", action="store_true", help="(a) alone, printed as one JSON line")
    ap.add_argument("--kernel-only", action="store_true", help="(k) alone, its table printed")
    ap.add_argument("--tree", default=here, help="the tree whose diffusionkit_amd package is measured (default: this script's)")
    ap.add_argument("--label", default="this", help="with --plain-only: the name of the tree in the JSON line")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    measure(a)
