"""Helpers of the stochastic-sampler tests (tests/test_stochastic_cpu.py, tests/test_gpu_stochastic.py): the noise of an image as the float64
reference defines it, the loop of a stochastic plan restated on the oracle, the analytic Gaussian problem, and sample moments.  Plain numpy / torch."""
import numpy as np
import torch

from diffusionkit_amd.sampler import philox_normal_reference, step_plan
from oracle import pipeline as op
from tests.test_samplers_cpu import blend

N_MOMENTS = 1 << 20  # draws per moment / correlation estimate: the bounds below are five standard errors at this N
MOMENT_SEEDS = (0, 1, (1 << 40) + 7)


def xi_of(seeds, draw, shape):
    """float64 [len(seeds), *shape]: image j's normals of draw ``draw``, element r of the flattened ``shape`` from ``philox_normal_reference``"""
    n = int(np.prod(shape))
    return np.stack([philox_normal_reference(s, draw, n).reshape(shape) for s in seeds])


def reference_loop(model, name, x, sigmas, conditioning, pooled, cfg_weight, act, seeds, t_act=None, eta=None, first_draw=0, inpaint=None):
    """tests/test_samplers_cpu.py's ``plan_loop`` for the plans with a noise term: d = (x - den) / sigma, x' = cx x + cd d + cn xi with xi the float64
    reference's normals of (seeds[img], the row's draw) rounded to float32, then the blend at the row's sigma_next.  x: [len(seeds), h, w, c]."""
    timesteps = (t_act or act).r(sigmas * 1000.0)
    model.cache_modulation_params(pooled, timesteps)
    for r in step_plan(name, sigmas.numpy(), eta, first_draw=first_draw):
        den = op.cfg_denoise(model, x, float(timesteps[r.index]), r.sigma, conditioning, cfg_weight, act)
        d = (x - den) / r.sigma
        x = r.cx * x + r.cd * d
        if r.cn != 0.0:
            x = x + r.cn * torch.from_numpy(xi_of(seeds, r.draw, tuple(x.shape[1:]))).to(torch.float32)
        if inpaint is not None:
            noise, x_orig, m = inpaint
            x = blend(x, r.sigma_next, noise, x_orig, m.to(torch.float32)[None, :, :, None])
    return x


# ---- the analytic problem: data N(0, S^2), the exact denoiser, a linear schedule 1 -> 0 ------------------------------------------------------------
S_DATA = 0.7
N_ANALYTIC = 65536


def exact_denoiser(x, sigma):
    return x * (1.0 - sigma) * S_DATA ** 2 / ((1.0 - sigma) ** 2 * S_DATA ** 2 + sigma ** 2)


def variance_ratio(name, steps, eta=None, seed=11):
    """var(x_final) / S^2 in float64 from x ~ N(0, 1) at sigma = 1 (the reference's draw 1000 of ``seed``: outside every schedule index used here),
    through the rows of ``step_plan(name, linspace(1, 0, steps + 1))`` with the plan's own noise"""
    sigmas = np.linspace(1.0, 0.0, steps + 1).astype(np.float32)
    x = philox_normal_reference(seed, 1000, N_ANALYTIC)
    for r in step_plan(name, sigmas, eta):
        d = (x - exact_denoiser(x, r.sigma)) / r.sigma
        x = r.cx * x + r.cd * d + (r.cn * philox_normal_reference(seed, r.draw, N_ANALYTIC) if r.cn != 0.0 else 0.0)
    return float(x.var() / S_DATA ** 2)


# ---- sample statistics --------------------------------------------------------------------------------------------------------------------------------
def moments(z):
    """(|mean|, |var - 1|, |E z^3|, |E z^4 - 3|) of a float64 sample"""
    return abs(z.mean()), abs(z.var() - 1.0), abs((z ** 3).mean()), abs((z ** 4).mean() - 3.0)


def moment_bounds(n):
    """five standard errors of the four statistics of ``moments`` for n independent standard normals: 5 / sqrt(n) times sqrt(1, 2, 15, 96)"""
    return tuple(5.0 * np.sqrt(v / n) for v in (1.0, 2.0, 15.0, 96.0))


def corr(a, b):
    return abs(float(np.mean(a * b)))
