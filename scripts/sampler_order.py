"""Convergence order of the step plans (diffusionkit_amd.sampler.step_plan) on a problem with a closed-form answer, without a model or a GPU.

The data is N(0, s2), s2 = 0.25: the optimal denoiser is den = x (1 - sigma) s2 / ((1 - sigma)^2 s2 + sigma^2), and the exact flow keeps
x(sigma) proportional to sqrt((1 - sigma)^2 s2 + sigma^2).  From x = 1 at the first sigma of the schedule, the rows of each plan are run in float64
and the absolute error of the final state is printed per schedule, sampler and step count, as the table of profiles/samplers.md.

    python scripts/sampler_order.py

This says what the coefficient tables do on an analytic problem; it says nothing about image quality on a trained checkpoint.
"""
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from diffusionkit_amd.sampler import SAMPLERS, FluxSampler, ModelSamplingDiscreteFlow, get_sigmas, step_plan  # noqa: E402

S2 = 0.25


def denoiser(x, sigma):
    return x * (1.0 - sigma) * S2 / ((1.0 - sigma) ** 2 * S2 + sigma ** 2)


def exact(sigma0, sigma1, x0=1.0):
    v = lambda s: math.sqrt((1.0 - s) ** 2 * S2 + s ** 2)  # noqa: E731
    return x0 * v(sigma1) / v(sigma0)


def run_plan(rows, x=1.0):
    """the rows in float64: d = (x - den) / sigma, x' = cx x + cd d + ch H, H' = hx x + hd d; a row that reads H before one wrote it fails"""
    hist = None
    for r in rows:
        d = (x - denoiser(x, r.sigma)) / r.sigma
        h_new = r.hx * x + r.hd * d if r.writes_h else hist
        x = r.cx * x + r.cd * d + (r.ch * hist if r.reads_h else 0.0)
        hist = h_new
    return x


def final_error(name, sigmas):
    return abs(run_plan(step_plan(name, sigmas)) - exact(float(sigmas[0]), float(sigmas[-1])))


SCHEDULES = (("FLUX, shift 1", FluxSampler(shift=1.0)), ("SD3, shift 3", ModelSamplingDiscreteFlow(shift=3.0)))
STEPS = (8, 16, 32, 64)


def main():
    print("| schedule | sampler | evaluations at 16 steps | " + " | ".join(f"{n} steps" for n in STEPS) + " | error ratio per halving |")
    print("|---|---|---|" + "---|" * (len(STEPS) + 1))
    for label, smp in SCHEDULES:
        for name in SAMPLERS:
            errs = [final_error(name, get_sigmas(smp, n)) for n in STEPS]
            ratios = " / ".join(f"{a / b:.3g}" for a, b in zip(errs, errs[1:]))
            print(f"| {label} | {name} | {len(step_plan(name, get_sigmas(smp, 16)))} | " + " | ".join(f"{e:.1e}" for e in errs) + f" | {ratios} |")


if __name__ == "__main__":
    main()
