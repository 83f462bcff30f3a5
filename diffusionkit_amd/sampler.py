"""Flow-matching sigma schedules (host-side scalars, float32 like the reference).

reference: python/src/diffusionkit/mlx/sampler.py:10-42 (ModelSamplingDiscreteFlow),
:45-77 (FluxSampler); schedule assembly python/src/diffusionkit/mlx/__init__.py:559-571.

Everything here is O(num_steps) scalar work done once per image; it is evaluated in
numpy float32 so that the values agree with the reference's MLX float32 arrays.
"""
from __future__ import annotations

import math

import numpy as np

_F = np.float32


class _FlowSamplerBase:
    #: first table index (reference sampler.py:16 uses arange(1, 1001); FluxSampler :51 arange(0, 1001))
    _TABLE_START = 1

    def __init__(self, shift: float = 1.0):
        self.shift = shift
        timesteps = 1000
        ts = self.sigma(np.arange(self._TABLE_START, timesteps + 1, 1))
        self.sigmas = ts

    @property
    def sigma_min(self):
        return self.sigmas[0]

    @property
    def sigma_max(self):
        return self.sigmas[-1]

    def timestep(self, sigma):
        return np.asarray(sigma, dtype=_F) * _F(1000)

    def sigma(self, timestep):
        timestep = np.asarray(timestep).astype(_F) / _F(1000.0)
        if self.shift == 1.0:
            return timestep
        s = _F(self.shift)
        return s * timestep / (_F(1) + (s - _F(1)) * timestep)

    def calculate_denoised(self, sigma, model_output, model_input):
        # x0 = x - v * sigma (reference sampler.py:37-39 / :72-74)
        return model_input - model_output * sigma

    def noise_scaling(self, sigma, noise, latent_image, max_denoise=False):
        return sigma * noise + (1.0 - sigma) * latent_image


class ModelSamplingDiscreteFlow(_FlowSamplerBase):
    """SD3 schedule helper (reference sampler.py:10-42)."""
    _TABLE_START = 1


class FluxSampler(_FlowSamplerBase):
    """FLUX schedule helper (reference sampler.py:45-77)."""
    _TABLE_START = 0


def _linspace_f32(start: float, stop: float, num: int) -> np.ndarray:
    # MLX linspace: arange(num) * ((stop-start)/(num-1)) + start, in float32.
    if num == 1:
        return np.asarray([start], dtype=_F)
    step = _F((stop - start) / (num - 1))
    return (np.arange(num, dtype=_F) * step + _F(start)).astype(_F)


def get_sigmas(sampler, num_steps: int) -> np.ndarray:
    """reference mlx/__init__.py:559-571 (incl. quirk Q13: for SD3 the shift is applied
    to endpoints that already went through ``sigma()``)."""
    start = float(sampler.timestep(sampler.sigma_max))
    end = float(sampler.timestep(sampler.sigma_min))
    is_flux = isinstance(sampler, FluxSampler)
    n = num_steps + 1 if is_flux else num_steps
    timesteps = _linspace_f32(start, end, n)
    sigs = [float(sampler.sigma(t)) for t in timesteps]
    if not is_flux:
        sigs += [0.0]
    return np.asarray(sigs, dtype=_F)


def max_denoise(sampler, sigmas) -> bool:
    """reference mlx/__init__.py:576-579"""
    max_sigma = float(sampler.sigma_max)
    sigma = float(sigmas[0])
    return math.isclose(max_sigma, sigma, rel_tol=1e-05) or sigma > max_sigma


# ---- first-block cache: which steps compute and which reuse (host policy; no reference counterpart) -------------------------
def block_cache_rel(probe) -> float:
    """``probe``: (num, den) per batch row as ``MMDiTEngine.forward_head`` returns them, on the host -> the relative change of block 0's
    effect on the image rows, the maximum over the batch rows of num / den.  den == 0 (no computed step to compare with) gives inf."""
    rel = 0.0
    for num, den in probe:
        num, den = float(num), float(den)
        r = num / den if den > 0.0 else math.inf
        rel = r if (r > rel or r != r) else rel  # (a NaN row is kept: it compares False with every threshold, the step computes)
    return rel


class BlockCachePolicy:
    """Skip a step iff ``rel < threshold``; the first and the last step always compute, and after ``max_consecutive_skips`` skipped
    steps in a row (None: no cap) the next one computes.  threshold 0 never skips, inf skips every step in between (``rel`` = inf,
    the answer before any computed step, is never below a threshold).  ``decide`` is called once per step, in order."""

    def __init__(self, threshold: float, max_consecutive_skips=None):
        threshold = float(threshold)
        if not threshold >= 0.0:
            raise ValueError(f"block cache threshold must be a float >= 0, got {threshold}")
        if max_consecutive_skips is not None and int(max_consecutive_skips) < 0:
            raise ValueError("max_consecutive_skips must be None or >= 0")
        self.threshold = threshold
        self.max_consecutive_skips = None if max_consecutive_skips is None else int(max_consecutive_skips)
        self._run = 0

    def decide(self, step: int, n_steps: int, rel: float) -> bool:
        """True: reuse the cached blocks in this step."""
        if step == 0:
            self._run = 0
        capped = self.max_consecutive_skips is not None and self._run >= self.max_consecutive_skips
        skip = 0 < step < n_steps - 1 and not capped and rel < self.threshold
        self._run = self._run + 1 if skip else 0
        return skip


class FixedSchedule:
    """The same interface with the decisions written down: skip exactly the steps in ``skip`` (never the first or the last one),
    whatever ``rel`` says -- for runs that must take the same decisions regardless of rounding."""

    threshold = None

    def __init__(self, skip):
        self.skip = frozenset(int(s) for s in skip)

    def decide(self, step: int, n_steps: int, rel: float) -> bool:
        return 0 < step < n_steps - 1 and step in self.skip
