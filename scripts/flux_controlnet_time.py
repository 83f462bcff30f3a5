"""What a FLUX ControlNet costs (synthetic weights, times only): one model evaluation of the FLUX.1-dev preset (dk_mmdit_forward with the context
hoisted) at batch 1, 512^2 and 1024^2, in one process:

  (a) the plain evaluation;
  (b) the main forward with the 15 precomputed taps of a (5, 10) ControlNet (``MMDiTEngine.set_flux_control_taps``): 18 double blocks, all 38 single
      blocks and the final layer -- 57 LayerNorm launches -- add a tap;
  (c) ``control_forward`` of the (5, 10) ControlNet (``config.flux_controlnet_config(5, 10)``);
  (d) the two together, as a controlled step runs them.

Beside them: (b) - (a) per tapped launch against the bytes the fused add moves (one tap row read, one image row written back), and (c) against
5 double-block and 10 single-block times of the main model (``run_blocks`` over all blocks of a kind, divided) plus fifteen h x h GEMMs timed
alone.  The rows of a table alternate inside every repeat.

    python scripts/flux_controlnet_time.py --commit HASH [--out profiles/flux_controlnet.md]
    python scripts/flux_controlnet_time.py --plain-only [--tree OTHER_TREE]     # (a) alone, one JSON line: for alternating two builds in one visit

One process, no retries: a failure ends the run.  No checkpoint has been run: the weights and operands are random."""
import argparse
import json
import os
import sys

import numpy as np

S_T = 512
WARM, EVALS, REPEATS = 2, 4, 5
SIDES = (64, 128)  # latent cells: 512^2 and 1024^2 pixels
N_DOUBLE, N_SINGLE = 5, 10


def measure(args):
    import torch
    from diffusionkit_amd import ops
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

    main = MMDiTEngine(cfg, pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1234, device=dev), dev, consume=True))
    text = torch.randn(1, S_T, cfg.token_level_text_embed_dim, generator=g).to(dev, BF)
    pooled = torch.randn(1, cfg.pooled_text_embed_dim, generator=g).to(dev, BF)

    def prepared(eng, side):
        eng.prepare(1, (side, side), S_T, 1)
        eng.cache_modulation_params(pooled, [1000.0])
        eng.cache_context(text)

    if args.plain_only:
        res = {}
        for side in SIDES:
            prepared(main, side)
            tok = main.patchify(torch.randn(1, side, side, 16, generator=g).to(dev))
            out = torch.empty_like(tok)
            med, span = rounds({"plain": lambda: main.forward_tokens(tok, None, 0, tokens_out=out)}, EVALS)
            res[f"{side * 8}^2"] = {"ms": round(med["plain"], 4), "min": round(span["plain"][0], 4), "max": round(span["plain"][1], 4)}
        print(json.dumps({"tree": args.label, "plain_evaluation": res}))
        return

    from diffusionkit_amd.config import flux_controlnet_config
    ccfg = flux_controlnet_config(N_DOUBLE, N_SINGLE, cfg)
    cn = MMDiTEngine(ccfg, pack_mmdit(ccfg, synth_mmdit_weights(ccfg, seed=4321, device=dev), dev, consume=True))
    h, nd, ns = cfg.hidden_size, cfg.depth_multimodal, cfg.depth_unified
    n_taps = N_DOUBLE + N_SINGLE
    launches = (nd - 1) + ns + 1  # block g + 1's LayerNorm behind double g < nd - 1; every single block's; the final layer's
    lines = ["# FLUX ControlNet: what the taps and the ControlNet's forward cost", "",
             f"Commit {args.commit}; {torch.cuda.get_device_name(0)}; synthetic weights and operands, bf16, batch 1, text length {S_T}; medians of "
             f"{REPEATS} repeats of {EVALS} evaluations,",
             "the rows of a table alternating inside every repeat, HIP events around back-to-back evaluations in one process (`scripts/flux_controlnet_time.py`).",
             "Nothing here is gated.  No checkpoint has been run.", "",
             f"## One model evaluation, FLUX.1-dev preset, ({N_DOUBLE}, {N_SINGLE}) ControlNet", "",
             f"(a) `dk_mmdit_forward`, context hoisted; (b) the same with {n_taps} taps set; (c) `dk_mmdit_control_forward` of the ControlNet; (d) (c) then (b), one stream.", "",
             "| image | (a) plain ms (min - max) | (b) with taps ms (min - max) | (c) ControlNet ms (min - max) | (d) both ms (min - max) | (d) - (a) ms | (d) / (a) |",
             "|---|---|---|---|---|---|---|"]
    second = ["", "## The fused add and the ControlNet against their predictions", "",
              f"*per launch*: ((b) - (a)) / {launches}, the {launches} LayerNorm launches that add a tap ({nd - 1} double blocks, {ns} single blocks, the final layer); "
              "*bytes*: one tap row read and one image row written back per image row (the row itself is read anyway);",
              "*at 6.3 TB/s*: those bytes at the HBM rate a streaming copy reaches on this chip.  *predicted (c)*: "
              f"{N_DOUBLE} double-block and {N_SINGLE} single-block times of the main model (`run_blocks` over the {nd} / {ns} blocks of a kind, divided; its two "
              f"copies of the stream included) plus the {n_taps} h x h tap GEMMs timed alone.", "",
              f"| image | (b) - (a) ms | per launch us | bytes per launch MB | at 6.3 TB/s us | spread of (a) ms | double block ms | single block ms | {n_taps} tap GEMMs ms | "
              "predicted (c) ms | (c) / predicted |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
    for side in SIDES:
        for eng in (main, cn):
            prepared(eng, side)
        lat = torch.randn(1, side, side, 16, generator=g).to(dev)
        cn.cache_control_image(torch.randn(1, side, side, 16, generator=g).to(dev), per_image=False)
        tok = main.patchify(lat)
        out = torch.empty_like(tok)
        taps = (torch.randn(*cn.taps_shape(), generator=g) * 0.1).to(dev, BF)
        S_i = tok.shape[1]
        x = torch.randn(S_i, h, generator=g).to(dev, BF)
        stream = torch.randn(1, S_T + S_i, h, generator=g).to(dev, BF)
        w, b = cn.weights["controlnet_blocks.0.weight"], cn.weights["controlnet_blocks.0.bias"]
        y = torch.empty_like(x)

        def plain():
            main.set_flux_control_taps(None)
            main.forward_tokens(tok, None, 0, tokens_out=out)

        def tapped():
            main.set_flux_control_taps(taps, N_DOUBLE, 1.0)
            main.forward_tokens(tok, None, 0, tokens_out=out)

        def control():
            cn.control_forward(tok, None, 0, taps_out=taps)

        def both():
            control()
            tapped()

        def gemms():
            for _ in range(n_taps):
                ops.linear(x, w, b, out=y)

        def doubles():
            main.set_flux_control_taps(None)
            main.run_blocks(stream, 0, 0, nd)

        def singles():
            main.set_flux_control_taps(None)
            main.run_blocks(stream, 0, nd, ns)

        med, span = rounds({"a": plain, "b": tapped, "c": control, "d": both, "g": gemms, "dbl": doubles, "sgl": singles}, EVALS)
        main.set_flux_control_taps(None)
        cell = lambda k: f"{med[k]:.2f} ({span[k][0]:.2f} - {span[k][1]:.2f})"  # noqa: E731
        lines.append(f"| {side * 8}^2 | {cell('a')} | {cell('b')} | {cell('c')} | {cell('d')} | {med['d'] - med['a']:.2f} | {med['d'] / med['a']:.3f} |")
        extra = med["b"] - med["a"]
        nbytes = 2 * S_i * h * 2  # (tap read + row write-back) x S_i rows x h x 2 bytes
        dbl, sgl = med["dbl"] / nd, med["sgl"] / ns
        pred = N_DOUBLE * dbl + N_SINGLE * sgl + med["g"]
        second.append(f"| {side * 8}^2 | {extra:.3f} | {1e3 * extra / launches:.1f} | {nbytes / 1e6:.1f} | {nbytes / 6.3e12 * 1e6:.1f} | "
                      f"{span['a'][1] - span['a'][0]:.3f} | {dbl:.3f} | {sgl:.3f} | {med['g']:.3f} | {pred:.2f} | {med['c'] / pred:.2f} |")
    text_out = "\n".join(lines + second) + "\n"
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text_out)


if __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(here, "profiles", "flux_controlnet.md"))
    ap.add_argument("--commit", default="unknown", help="stamp of the tree that runs (the caller knows it; a copy without .git does not)")
    ap.add_argument("--plain-only", action="store_true", help="(a) alone, printed as one JSON line")
    ap.add_argument("--tree", default=here, help="the tree whose diffusionkit_amd package is measured (default: this script's)")
    ap.add_argument("--label", default="this", help="with --plain-only: the name of the tree in the JSON line")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    measure(a)
