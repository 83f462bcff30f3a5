"""The noisy row launch (dk_noisy_cfg_step, the stochastic samplers' update) against two baselines on one box, alternating, at the 128 x 128 x 16
latent with n_img 1 and 4: the plain row launch of the same build (dk_lms_cfg_step: unchanged code), and the unfused alternative -- ops.philox_normal,
a torch add_ of cn times its output, then the plain launch.  HIP events over back-to-back launches in one process, each window after a warm-up of its
own.  Also measured here: the generator's largest deviation from the float64 definition at N = 2^20; and, without the GPU, the analytic table of
tests/_stochastic.py.  ``python scripts/stochastic_step_time.py [--commit ID] [out.md [out.json]]`` writes profiles/stochastic_samplers.md's body."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffusionkit_amd import ops  # noqa: E402
from diffusionkit_amd.sampler import philox_normal_reference  # noqa: E402
from tests._stochastic import variance_ratio  # noqa: E402

argv = sys.argv[1:]
commit, LAUNCHES, ROUNDS = "not given", 20000, 5
if argv[:1] == ["--commit"]:
    commit, argv = argv[1], argv[2:]
if argv[:1] == ["--launches"]:  # (a short run for a kernel trace: rocprofv3 --kernel-trace --stats -- python scripts/stochastic_step_time.py --launches 2000)
    LAUNCHES, ROUNDS, argv = int(argv[1]), 1, argv[2:]
assert torch.cuda.is_available(), "this script measures on the GPU: there is no CPU path"
dev = torch.device("cuda", 0)
res = {"commit": commit, "device": torch.cuda.get_device_name(0)}
Hl, Wl, C, p = 128, 128, 16, 2
ROW = (0.75, -0.3125, 0.0, 0.0, 0.0)  # euler_a(1) from sigma 0.75 to 0.5 on a linear schedule
CN, DRAW = 0.4330127, 1


def kernel_us(fn, n):
    for _ in range(200):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / n, 3)


res["step_us_back_to_back"] = {}
for n_img in (1, 4):
    for cfg_on in (False, True):
        x = torch.randn(n_img, Hl, Wl, C, device=dev)
        out = torch.randn(n_img * (2 if cfg_on else 1), (Hl // p) * (Wl // p), p * p * C, device=dev).to(torch.bfloat16)
        tok = torch.empty_like(out)
        seeds = ops.seed_tensor(range(7, 7 + n_img), dev)
        head = (x, out, tok, n_img, cfg_on, p, 1, 0.75, 0.5, 5.0 if cfg_on else 0.0, None, ROW, False, False)

        def unfused():
            x.add_(ops.philox_normal(seeds, Hl * Wl * C, DRAW).view_as(x), alpha=CN)
            ops.lms_cfg_step(*head)
        launches = {"noisy": lambda: ops.noisy_cfg_step(*head, cn=CN, seeds=seeds, draw=DRAW), "plain": lambda: ops.lms_cfg_step(*head),
                    "unfused": unfused}
        times = {k: [] for k in launches}
        for _ in range(ROUNDS):  # (alternating)
            for k, fn in launches.items():
                x.normal_()  # (the window starts from unit-scale values whatever the last one left)
                times[k].append(kernel_us(fn, LAUNCHES))
        res["step_us_back_to_back"][f"n_img={n_img},cfg={'on' if cfg_on else 'off'}"] = times
        print(n_img, cfg_on, times, flush=True)

# ---- the generator's deviation ----------------------------------------------------------------------------------------------------------------------------
N, SEED = 1 << 20, (1 << 40) + 7
one = ops.seed_tensor([SEED], dev)
z = ops.philox_normal(one, N, 0).double().cpu().numpy()[0]
ref = philox_normal_reference(SEED, 0, N)
err = np.abs(z - ref)
res["generator"] = {"n": N, "seed": SEED, "max_abs_deviation": float(err.max()), "at_z": float(ref[int(err.argmax())]), "largest_abs_z": float(np.abs(ref).max()),
                    "philox_normal_us_128x128x16": kernel_us(lambda: ops.philox_normal(one, Hl * Wl * C, 0), LAUNCHES)}

# ---- the analytic table (host arithmetic) -----------------------------------------------------------------------------------------------------------------
res["analytic_var_ratio"] = {str(s): {"euler": variance_ratio("euler", s), "euler_a(1)": variance_ratio("euler_a", s, 1.0), "sde": variance_ratio("sde", s)}
                             for s in (8, 16, 32)}

med = lambda v: float(np.median(v))  # noqa: E731
lines = [f"Measured on {res['device']}, commit {commit}; {ROUNDS} alternating rounds of {LAUNCHES} back-to-back launches per variant (HIP events), "
         f"latent {Hl} x {Wl} x {C}, bf16 tokens, row (cx, cd, cn) = ({ROW[0]}, {ROW[1]}, {CN}).", "",
         "| n_img | CFG | noisy launch, us (median; min - max) | plain launch, us | unfused (philox_normal + add_ + plain), us | noisy - plain, us |", "|---|---|---|---|---|---|"]
for key, t in res["step_us_back_to_back"].items():
    n_img, cfg = (kv.split("=")[1] for kv in key.split(","))
    cell = lambda v: f"{med(v):.2f} ({min(v):.2f} - {max(v):.2f})"  # noqa: E731
    lines.append(f"| {n_img} | {cfg} | {cell(t['noisy'])} | {cell(t['plain'])} | {cell(t['unfused'])} | {med(t['noisy']) - med(t['plain']):+.2f} |")
g = res["generator"]
lines += ["", f"Generator (commit {commit}): largest |ops.philox_normal - philox_normal_reference| over N = 2^20 normals of seed 2^40 + 7, draw 0: "
          f"{g['max_abs_deviation']:.3e} (at z = {g['at_z']:.4f}; largest |z| of the sample {g['largest_abs_z']:.3f}).  ops.philox_normal alone at "
          f"{Hl} x {Wl} x {C}: {g['philox_normal_us_128x128x16']:.2f} us per call, back to back, its output allocation included.", "",
          f"Analytic problem (commit {commit}; host arithmetic, float64): var(x_final) / s^2, data N(0, 0.7^2), exact denoiser, linear schedule, 65536 elements.", "",
          "| Steps | euler | euler_a(1) | sde |", "|---|---|---|---|"]
lines += [f"| {s} | {r['euler']:.3f} | {r['euler_a(1)']:.3f} | {r['sde']:.3f} |" for s, r in res["analytic_var_ratio"].items()]
print("\n".join(lines))
if argv:
    open(argv[0], "w").write("\n".join(lines) + "\n")
if len(argv) > 1:
    json.dump(res, open(argv[1], "w"), indent=1)
