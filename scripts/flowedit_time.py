"""FlowEdit's costs on one box (profiles/flowedit.md's body).  (1) The step launch (dk_flowedit_step) at the latent of a 1024 x 1024 image, 128 x 128 x
16, in the FLUX layout (patch order (c, ph, pw), no CFG: 2 batch rows) and the SD3 layout ((ph, pw, c), CFG: 4 batch rows), against the stochastic
samplers' launch (dk_noisy_cfg_step) at the same latent with that family's usual rows (1 and 2), alternating; and the bytes each moves, from the shapes,
at the chip's measured streaming rate.  (2) One model evaluation of the edit phase (2 rows FLUX.1-schnell, 4 rows SD3-medium) against the plain
evaluation (1 and 2 rows) on synthetic weights, alternating.  HIP events over back-to-back launches in one process, each window after a warm-up of its
own.  ``python scripts/flowedit_time.py [--commit ID] [--no-model] [out.md [out.json]]``."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionkit_amd import ops  # noqa: E402

argv = sys.argv[1:]
commit, LAUNCHES, ROUNDS, MODEL = "not given", 20000, 5, True
if argv[:1] == ["--commit"]:
    commit, argv = argv[1], argv[2:]
if argv[:1] == ["--no-model"]:
    MODEL, argv = False, argv[1:]
assert torch.cuda.is_available(), "this script measures on the GPU: there is no CPU path"
dev = torch.device("cuda", 0)
res = {"commit": commit, "device": torch.cuda.get_device_name(0)}
Hl, Wl, C, p = 128, 128, 16, 2
S_I, F = (Hl // p) * (Wl // p), p * p * C
STREAM_TBS = 6.29  # MI355X, measured float4 copy (8.0 TB/s spec)
BF = torch.bfloat16


def window_us(fn, n, warm=200):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / n, 3)


def flowedit_bytes(rows, zs):
    """per launch: z read and written, x_src read, zt (and zs) written in fp32; ``rows`` batch rows of model_out read and of tokens written, 16 bit"""
    n = Hl * Wl * C
    return n * 4 * (4 + int(zs)) + 2 * rows * n * 2


def noisy_bytes(rows):
    """x read and written in fp32; ``rows`` batch rows of model_out read and of tokens written"""
    n = Hl * Wl * C
    return n * 4 * 2 + 2 * rows * n * 2


# ---- 1. the step launch -------------------------------------------------------------------------------------------------------------------------------
res["step"] = {}
for name, order, cfg_on, dt in (("flux", 1, False, BF), ("sd3", 0, True, BF), ("sd3-f16", 0, True, torch.float16)):
    rows_e, rows_n = (4, 2) if cfg_on else (2, 1)
    z, x_src, zt = (torch.randn(1, Hl, Wl, C, device=dev) for _ in range(3))
    out_e = torch.randn(rows_e, S_I, F, device=dev).to(dt)
    tok_e = torch.empty_like(out_e)
    x = torch.randn(1, Hl, Wl, C, device=dev)
    out_n = torch.randn(rows_n, S_I, F, device=dev).to(dt)
    tok_n = torch.empty_like(out_n)
    seeds = ops.seed_tensor([7], dev)
    launches = {
        "flowedit": lambda: ops.flowedit_step(z, x_src, out_e, tok_e, zt, 1, cfg_on, p, order, c=-1e-3, sigma_in=0.5, seeds=seeds, draw=1, w_src=3.5, w_tar=13.5),
        "noisy": lambda: ops.noisy_cfg_step(x, out_n, tok_n, 1, cfg_on, p, order, 0.75, 0.5, 5.0 if cfg_on else 0.0, None, (0.75, -0.3125, 0.0, 0.0, 0.0),
                                            False, False, cn=0.4330127, seeds=seeds, draw=1)}
    times = {k: [] for k in launches}
    for _ in range(ROUNDS):  # (alternating)
        for k, fn in launches.items():
            z.normal_(), x.normal_()  # (the window starts from unit-scale values whatever the last one left)
            times[k].append(window_us(fn, LAUNCHES))
    res["step"][name] = {"us": times, "rows": {"flowedit": rows_e, "noisy": rows_n},
                         "bytes": {"flowedit": flowedit_bytes(rows_e, False), "noisy": noisy_bytes(rows_n)}}
    print(name, times, flush=True)

# ---- 2. one model evaluation, edit rows against plain rows -----------------------------------------------------------------------------------------------
res["eval"] = {}
if MODEL:
    from diffusionkit_amd.config import FLUX_SCHNELL, SD3_2b
    from diffusionkit_amd.engine import MMDiTEngine
    from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
    for name, cfg, s_t, plain, edit in (("sd3-medium-1024", SD3_2b, 589, 2, 4), ("flux-schnell-1024", FLUX_SCHNELL, 256, 1, 2)):
        eng = MMDiTEngine(cfg, pack_mmdit(cfg, synth_mmdit_weights(cfg, seed=1234, device=dev), dev, consume=True))
        g = torch.Generator().manual_seed(1)
        text = torch.randn(edit, s_t, cfg.token_level_text_embed_dim, generator=g).to(dev, BF)
        pooled = torch.randn(edit, cfg.pooled_text_embed_dim, generator=g).to(dev, BF)
        times = {plain: [], edit: []}
        for _ in range(3):  # (alternating)
            for B in (plain, edit):
                eng.prepare(B, (Hl, Wl), s_t, 1)
                eng.cache_modulation_params(pooled[:B], [500.0])
                eng.cache_context(text[:B].contiguous())
                tok = torch.randn(B, S_I, F, device=dev).to(BF)
                out = torch.empty_like(tok)
                times[B].append(round(window_us(lambda: eng.forward_tokens(tok, None, 0, tokens_out=out), 10, warm=3) / 1e3, 3))
        res["eval"][name] = {"ms": {str(k): v for k, v in times.items()}, "plain_rows": plain, "edit_rows": edit}
        print(name, times, flush=True)
        del eng
        torch.cuda.empty_cache()

med = lambda v: float(np.median(v))  # noqa: E731
cell = lambda v: f"{med(v):.2f} ({min(v):.2f} - {max(v):.2f})"  # noqa: E731
lines = [f"Measured on {res['device']}, commit {commit}; {ROUNDS} alternating rounds of {LAUNCHES} back-to-back launches per variant (HIP events), latent "
         f"{Hl} x {Wl} x {C}, one image.  Bytes are counted from the shapes; the floor is bytes / {STREAM_TBS} TB/s, the chip's measured streaming rate.", "",
         "| Layout | dk_flowedit_step, us (median; min - max) | rows | bytes | floor, us | dk_noisy_cfg_step, us | rows | bytes | floor, us |",
         "|---|---|---|---|---|---|---|---|---|"]
for name, r in res["step"].items():
    b, rows, t = r["bytes"], r["rows"], r["us"]
    lines.append(f"| {name} | {cell(t['flowedit'])} | {rows['flowedit']} | {b['flowedit']} | {b['flowedit'] / STREAM_TBS / 1e6:.2f} | {cell(t['noisy'])} | "
                 f"{rows['noisy']} | {b['noisy']} | {b['noisy'] / STREAM_TBS / 1e6:.2f} |")
if res["eval"]:
    lines += ["", "One model evaluation (forward_tokens, synthetic weights, bf16), 3 alternating rounds of 10 back-to-back evaluations:", "",
              "| Model | plain rows | ms (median; min - max) | edit rows | ms | ratio |", "|---|---|---|---|---|---|"]
    for name, r in res["eval"].items():
        a, b = r["ms"][str(r["plain_rows"])], r["ms"][str(r["edit_rows"])]
        lines.append(f"| {name} | {r['plain_rows']} | {cell(a)} | {r['edit_rows']} | {cell(b)} | {med(b) / med(a):.2f} |")
print("\n".join(lines))
if argv:
    open(argv[0], "w").write("\n".join(lines) + "\n")
if len(argv) > 1:
    json.dump(res, open(argv[1], "w"), indent=1)
