"""Flow-matching sigma schedules (host-side scalars, float32 like the reference).

reference: python/src/diffusionkit/mlx/sampler.py:10-42 (ModelSamplingDiscreteFlow),
:45-77 (FluxSampler); schedule assembly python/src/diffusionkit/mlx/__init__.py:559-571.

Everything here is O(num_steps) scalar work done once per image; it is evaluated in
numpy float32 so that the values agree with the reference's MLX float32 arrays.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple

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


# ---- step plans: the update of every model evaluation as a coefficient row (host; no reference counterpart) --------------------------------
SAMPLERS = ("euler", "heun", "ab2")
#: the samplers whose rows carry a noise term (cn xi, drawn inside the step launch: "stochastic samplers" below); every name ``step_plan`` takes
STOCHASTIC_SAMPLERS = ("euler_a", "sde")
ALL_SAMPLERS = SAMPLERS + STOCHASTIC_SAMPLERS


def check_sampler(name) -> str:
    """None -> "euler"; an unknown name raises a ValueError that lists the valid ones"""
    if name is None:
        return "euler"
    if name not in ALL_SAMPLERS:
        raise ValueError(f"unknown sampler {name!r}: valid samplers are {', '.join(ALL_SAMPLERS)}")
    return name


def check_sampler_eta(name, eta) -> float:
    """``sampler_eta`` of a checked sampler name -> the eta of ``euler_a`` (None: 1.0); with any other sampler a value raises, and so does one outside
    [0, 1] or NaN"""
    if eta is None:
        return 1.0
    if name != "euler_a":
        raise ValueError(f"sampler_eta belongs to sampler 'euler_a' alone, not to {name!r}")
    eta = float(eta)
    if not 0.0 <= eta <= 1.0:
        raise ValueError(f"sampler_eta must lie in [0, 1], got {eta}")
    return eta


class StepRow(NamedTuple):
    """One model evaluation and the update behind it (dk_lms_cfg_step):  d = (x - den) / sigma,  x' = cx x + cd d + ch H,  H' = hx x + hd d.
    ``index``: which entry of the schedule the model is evaluated at (also the row of the cached modulation table); ``sigma`` = sigmas[index];
    ``sigma_next``: the sigma x' lives at (the masked blend re-noises the known region to it); ``reads_h`` / ``writes_h``: whether the row takes
    the history buffer / leaves one for a later row; ``ends_step``: x' is the state at the next entry of the schedule.
    Stochastic samplers: x' takes one more term, cn xi, xi the image's own standard normals of draw ``draw`` (``philox_normal_reference``); cn == 0
    (every row of the deterministic samplers, where ``draw`` stays -1): no term, the launch as it was."""
    index: int
    sigma: float
    sigma_next: float
    cx: float
    cd: float
    ch: float
    hx: float
    hd: float
    reads_h: bool
    writes_h: bool
    ends_step: bool
    cn: float = 0.0
    draw: int = -1


def _row(index, sigma, sigma_next, cd, ch=0.0, reads_h=False, writes_h=False, ends_step=True) -> StepRow:
    # (every method here keeps cx = 1 and H' = d; the coefficients are rounded to the kernel's float32 once, here)
    f = lambda v: float(_F(v))  # noqa: E731
    return StepRow(int(index), f(sigma), f(sigma_next), 1.0, f(cd), f(ch) if reads_h else 0.0, 0.0, 1.0 if writes_h else 0.0, bool(reads_h),
                   bool(writes_h), bool(ends_step))


def _noisy_row(index, sigma, sigma_next, cx, cd, cn, draw) -> StepRow:
    # (a first-order row with its own cx and a noise term; rounded to the kernel's float32 once, like ``_row``)
    f = lambda v: float(_F(v))  # noqa: E731
    return StepRow(int(index), f(sigma), f(sigma_next), f(cx), f(cd), 0.0, 0.0, 0.0, False, False, True, f(cn), int(draw))


def euler_a_coefficients(sigma, sigma_next, eta):
    """(sigma_down, cx, cd, cn) of one ancestral step of a rectified flow, in float64 (k-diffusion's sample_euler_ancestral_RF):
    sigma_down = sigma' (1 + (sigma' / sigma - 1) eta), a = (1 - sigma') / (1 - sigma_down), cx = a, cd = a (sigma_down - sigma),
    cn = sqrt(sigma'^2 - sigma_down^2 a^2).  sigma_down == 1 (sigma' = 1: a schedule that does not leave pure noise) is refused."""
    sigma, sigma_next, eta = float(sigma), float(sigma_next), float(eta)
    down = sigma_next * (1.0 + (sigma_next / sigma - 1.0) * eta)
    if down == 1.0:
        raise ValueError(f"euler_a: the step {sigma} -> {sigma_next} has sigma_down = 1: the schedule must leave sigma = 1 after its first entry")
    a = (1.0 - sigma_next) / (1.0 - down)
    return down, a, a * (down - sigma), math.sqrt(max(sigma_next * sigma_next - down * down * a * a, 0.0))


def step_plan(name, sigmas, eta=None, first_draw: int = 0) -> List[StepRow]:
    """The ordered rows that take x from sigmas[0] to sigmas[-1], computed in float64 from the float32 schedule, with h = sigmas[i+1] - sigmas[i]:
    euler  one row (1, h, 0) per step -- h is exact in float64, so its rounding is the float32 difference dk_euler_cfg_step takes;
    heun   the trapezoid rule: the predictor (1, h, 0) at sigmas[i] leaves H = d, the corrector at sigmas[i+1], evaluated on the predicted
           state, is (1, h/2, -h/2): x + (h/2)(d1 + d2).  The model is never evaluated at sigma = 0: a step that ends there is its Euler row;
    ab2    variable-step Adams-Bashforth 2: the first row is Euler and leaves H = d; later ones are (1, h(1 + w), -h w), w = h / (2 h_prev),
           H = d; a step that ends at sigma = 0 is its Euler row here too.
    A row writes H only if the next row reads it.  A schedule cut by ``denoise`` starts at its first remaining entry, first-order.
    The stochastic samplers, first order, one evaluation per step.  A row with a noise term has draw = ``first_draw`` + its index: the whole schedule
    has draw == index, and a schedule cut by ``denoise`` keeps the draws of the entries it keeps when the caller passes the number of entries cut
    as ``first_draw`` (the index itself counts from the entries given here: it is also the row of the modulation table).  A row without one -- a step
    that ends at sigma = 0, every row under eta = 0 -- is the Euler row, draw = -1 like the deterministic samplers' rows.
    euler_a  ``euler_a_coefficients`` with ``eta`` in [0, 1] (None: 1); eta = 0 gives euler's rows exactly;
    sde      diffusers' FlowMatchEulerDiscreteScheduler(stochastic_sampling=True): x' = (1 - sigma') den + sigma' xi, i.e. (cx, cd, cn) =
             (1 - sigma', -(1 - sigma') sigma, sigma').  Every step re-draws all of the noise; at a finite number of steps this does not preserve the
             marginals of a mean-predicting denoiser (tests/test_stochastic_cpu.py tabulates it).  It is here as the published definition, nothing more."""
    name = check_sampler(name)
    eta = check_sampler_eta(name, eta)
    s = [float(v) for v in np.asarray(sigmas, dtype=_F)]
    n = len(s) - 1
    rows: List[StepRow] = []
    for i in range(n):
        h = s[i + 1] - s[i]
        last = s[i + 1] == 0.0
        if name == "euler" or last and name in ("heun", "euler_a", "sde") or name == "euler_a" and eta == 0.0:
            rows.append(_row(i, s[i], s[i + 1], h))  # (sde at sigma' = 0: (1, -sigma, 0), which is this row)
        elif name == "euler_a":
            _, cx, cd, cn = euler_a_coefficients(s[i], s[i + 1], eta)
            rows.append(_noisy_row(i, s[i], s[i + 1], cx, cd, cn, int(first_draw) + i))
        elif name == "sde":
            rows.append(_noisy_row(i, s[i], s[i + 1], 1.0 - s[i + 1], -(1.0 - s[i + 1]) * s[i], s[i + 1], int(first_draw) + i))
        elif name == "heun":
            rows.append(_row(i, s[i], s[i + 1], h, writes_h=True, ends_step=False))
            rows.append(_row(i + 1, s[i + 1], s[i + 1], h / 2, -h / 2, reads_h=True))
        else:
            feeds = i + 1 < n and s[i + 2] != 0.0  # (the next row reads H)
            if i == 0 or last:
                rows.append(_row(i, s[i], s[i + 1], h, writes_h=feeds))
            else:
                w = h / (2.0 * (s[i] - s[i - 1]))
                rows.append(_row(i, s[i], s[i + 1], h * (1.0 + w), -h * w, reads_h=True, writes_h=feeds))
    return rows


# ---- the noise of the stochastic samplers: Philox4x32-10 and Box-Muller, the definition the device function restates (no reference counterpart) -------
_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11; Random123's known answers hold): ``counter`` = four and ``key`` = two 32-bit words, each an int or an array
    of uint64 holding values below 2^32 (arrays broadcast) -> the four output words, of the same kind.  One round:
    c' = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key takes its Weyl increments between rounds."""
    arr = any(isinstance(v, np.ndarray) for v in tuple(counter) + tuple(key))
    cast = (lambda v: np.asarray(v, dtype=np.uint64)) if arr else int
    c0, c1, c2, c3 = (cast(v) for v in counter)
    k0, k1 = (cast(v) for v in key)
    m0, m1, w0, w1, lo = (cast(v) for v in (_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1, _M32))
    sh = cast(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # (below 2^64: exact in uint64)
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & lo, (p0 >> sh) ^ c3 ^ k1, p0 & lo
        k0, k1 = (k0 + w0) & lo, (k1 + w1) & lo
    return c0, c1, c2, c3


def philox_normal_reference(seed, draw, n, stream=0, quad_offset=0) -> np.ndarray:
    """The ``n`` (a multiple of 4) standard normals of one image, float64: quad q = quad_offset + r // 4 of element r is the Philox block of the counter
    (q & 0xffffffff, q >> 32, draw, stream) under the key (seed & 0xffffffff, seed >> 32), 0 <= seed < 2^64; a block (o0, o1, o2, o3) gives four
    normals by Box-Muller on 24-bit uniforms, u = ((o_a >> 8) + 1) 2^-24 in (0, 1], theta = 2 pi (o_b >> 8) 2^-24, z_a = sqrt(-2 ln u) cos theta,
    z_b = sqrt(-2 ln u) sin theta, with the pairs (o0, o1) -> z0, z1 and (o2, o3) -> z2, z3; element r takes z[r % 4].  ``stream`` 0: step noise."""
    seed, draw, n, stream, quad_offset = int(seed), int(draw), int(n), int(stream), int(quad_offset)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"the seed must lie in [0, 2^64), got {seed}")
    if n % 4 != 0 or n < 0:
        raise ValueError(f"n must be a multiple of 4, got {n}")
    q = np.arange(n // 4, dtype=np.uint64) + np.uint64(quad_offset)
    o = philox4x32_10((q & np.uint64(_M32), q >> np.uint64(32), np.uint64(draw & _M32), np.uint64(stream & _M32)), (seed & _M32, seed >> 32))
    z = np.empty((n // 4, 4), dtype=np.float64)
    for a in (0, 2):
        u = ((o[a] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        theta = 2.0 * math.pi * ((o[a + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24)
        rad = np.sqrt(-2.0 * np.log(u))
        z[:, a], z[:, a + 1] = rad * np.cos(theta), rad * np.sin(theta)
    return z.reshape(-1)


def stochastic_reference(x, den, row, xi):
    """One row in float64 numpy: d = (x - den) / sigma, x' = cx x + cd d + cn xi (``row`` a first-order StepRow; ``xi`` shaped like x, ignored where
    cn == 0)"""
    x, den = np.asarray(x, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = row.cx * x + row.cd * ((x - den) / row.sigma)
    return out + row.cn * np.asarray(xi, dtype=np.float64) if row.cn != 0.0 else out


# ---- FlowEdit: text-guided editing of an existing image (Kulikov et al. 2024; no reference counterpart) --------------------------------------
FLOWEDIT_STREAM = 1  # the Philox stream tag of the edit's draws: a stochastic sampler in the tail (tag 0) never repeats one
# (T, n_max, n_min, source, target) per family: the paper's settings as recalled, NOT verified against the paper or the authors' code.  source /
# target: the CFG weights (SD3) or the distilled-guidance values (FLUX.1-dev)
FLOWEDIT_DEFAULTS = {"sd3": (50, 33, 0, 3.5, 13.5), "flux": (28, 24, 0, 1.5, 5.5)}


class FlowEditRow(NamedTuple):
    """One dk_flowedit_step launch.  ``index``: the schedule entry of the model evaluation the launch consumes (``prime``: no evaluation yet, the
    entry the first inputs are formed for); ``c``: the coefficient on V_tar - V_src, (sigmas[index + 1] - sigmas[index]) / n_avg (prime: 0);
    ``sigma_in``: the sigma the launch forms the next inputs at; ``draw``: the number of the draw it forms them with; ``next_index``: the schedule
    entry the next evaluation runs at (the row of the modulation table; past the last evaluation: the entry the edit phase hands on);
    ``ends_step``: Z is complete for its outer step."""
    index: int
    c: float
    sigma_in: float
    draw: int
    prime: bool
    next_index: int
    ends_step: bool


def check_flowedit(num_steps, n_max, n_min, n_avg):
    """(n_max, n_min, n_avg) as ints with 0 <= n_min < n_max <= num_steps and n_avg >= 1, else a ValueError that names the rule"""
    n_max, n_min, n_avg, num_steps = int(n_max), int(n_min), int(n_avg), int(num_steps)
    if n_min < 0 or n_min >= n_max:
        raise ValueError(f"edit_steps: n_min must satisfy 0 <= n_min < n_max, got (n_max, n_min) = ({n_max}, {n_min})")
    if n_max > num_steps:
        raise ValueError(f"edit_steps: n_max = {n_max} exceeds num_steps = {num_steps}")
    if n_avg < 1:
        raise ValueError(f"edit_n_avg must be at least 1, got {n_avg}")
    return n_max, n_min, n_avg


def flowedit_plan(sigmas, n_max, n_min=0, n_avg=1) -> List[FlowEditRow]:
    """The launches of the edit phase over the descending schedule ``sigmas`` [T + 1]: the prime row, which forms the inputs of the first evaluation
    at sigmas[T - n_max], then one row per evaluation -- n_avg per outer step i = T - n_max .. T - n_min - 1.  Draw k < n_avg - 1 of a step keeps
    ``sigma_in`` at sigmas[i]; the last one moves it to sigmas[i + 1], and its launch completes Z for the step.  The inputs of evaluation (i, k) are
    formed with draw i * n_avg + k: distinct, and a function of the schedule alone.  The last row forms, at sigmas[T - n_min], what the edit
    hands on: with n_min == 0 that sigma is 0 and the result is Z (Zt is Z but for the rounding of x_src + (Z - x_src)); otherwise Zt is the state the
    ordinary loop takes to sigma 0.  c is computed in
    float64 from the float32 schedule and rounded to float32 once."""
    s = [float(v) for v in np.asarray(sigmas, dtype=_F)]
    T = len(s) - 1
    n_max, n_min, n_avg = check_flowedit(T, n_max, n_min, n_avg)
    f = lambda v: float(_F(v))  # noqa: E731
    i0 = T - n_max
    rows = [FlowEditRow(i0, 0.0, f(s[i0]), i0 * n_avg, True, i0, False)]
    for i in range(i0, T - n_min):
        for k in range(n_avg):
            last = k == n_avg - 1
            nxt, nk = (i + 1, 0) if last else (i, k + 1)
            rows.append(FlowEditRow(i, f((s[i + 1] - s[i]) / n_avg), f(s[nxt]), nxt * n_avg + nk, False, nxt, last))
    return rows


def flowedit_row_reference(z, x_src, v_src, v_tar, row, xi):
    """One row in float64 numpy -> (Z', Zs, Zt): Z' = Z + c (V_tar - V_src) (prime: Z), Zs = (1 - sigma_in) x_src + sigma_in xi,
    Zt = Zs + (Z' - x_src).  ``v_src`` / ``v_tar``: the model's outputs in the latent's layout, already combined under CFG (``cfg_combine``);
    ignored by a prime row.  ``xi`` shaped like Z."""
    z, x_src, xi = (np.asarray(v, dtype=np.float64) for v in (z, x_src, xi))
    if not row.prime:
        z = z + row.c * (np.asarray(v_tar, dtype=np.float64) - np.asarray(v_src, dtype=np.float64))
    zs = (1.0 - row.sigma_in) * x_src + row.sigma_in * xi
    return z, zs, zs + (z - x_src)


def cfg_combine(pos, neg, w):
    """neg + w (pos - neg) in float64: how dk_euler_cfg_step and dk_flowedit_step combine the prompt row and the negative row"""
    pos, neg = np.asarray(pos, dtype=np.float64), np.asarray(neg, dtype=np.float64)
    return neg + float(w) * (pos - neg)


def flowedit_reference(x_src, sigmas, n_max, n_min, n_avg, velocity, seeds):
    """The edit phase in float64 numpy.  ``x_src`` [n_img, ...]; ``velocity(zs, zt, sigma, index)`` -> (V_src, V_tar), each shaped like x_src;
    ``seeds``: one per image, the noise of image j is ``philox_normal_reference(seeds[j], draw, n, stream=1)``.  Returns (Z, Zt) behind the last
    row: with n_min == 0 Z is the result; otherwise Zt is what the ordinary loop takes from sigmas[T - n_min] to 0."""
    x_src = np.asarray(x_src, dtype=np.float64)
    n = int(np.prod(x_src.shape[1:]))
    z, zs, zt = x_src.copy(), None, None
    for row in flowedit_plan(sigmas, n_max, n_min, n_avg):
        v_src = v_tar = None
        if not row.prime:
            v_src, v_tar = velocity(zs, zt, float(_F(np.asarray(sigmas, dtype=_F)[row.index])), row.index)
        xi = np.stack([philox_normal_reference(sd, row.draw, n, FLOWEDIT_STREAM) for sd in seeds]).reshape(x_src.shape)
        z, zs, zt = flowedit_row_reference(z, x_src, v_src, v_tar, row, xi)
    return z, zt


# ---- guidance modes: how the two predictions of a guided evaluation are combined (no reference counterpart) ---------------------------------
GUIDANCE = ("cfg", "rescale", "apg")


def check_guidance(name) -> str:
    """None -> "cfg"; an unknown name raises a ValueError that lists the valid ones"""
    if name is None:
        return "cfg"
    if name not in GUIDANCE:
        raise ValueError(f"unknown guidance mode {name!r}: valid modes are {', '.join(GUIDANCE)}")
    return name


def check_interval(interval):
    """None -> (0, inf), which guides every evaluation; otherwise (lo, hi) with lo <= hi, neither NaN, as float32 values"""
    if interval is None:
        return 0.0, math.inf
    lo, hi = (float(_F(v)) for v in interval)
    if not lo <= hi:
        raise ValueError(f"guidance_interval must be (lo, hi) with lo <= hi, got ({lo}, {hi})")
    return lo, hi


def guide_reference(c, u, w, mode="cfg", *, rescale=0.7, eta=0.0, norm_threshold=0.0, momentum=0.0, m=None, reads_m=False, writes_m=False):
    """The statement of the guidance modes, in float64 numpy: ``c`` and ``u`` [n_img, ...] are the x0 predictions of the prompt and the negative
    row, w the guidance weight; every mean, norm and inner product is taken per image, over all of its elements.  Returns (den, m').
      cfg      den = u + w (c - u)
      rescale  g = u + w (c - u);  s = phi std(c) / std(g) + (1 - phi), s = 1 if std(g) == 0;  den = g s       (Lin et al. 2023, section 3.4)
      apg      D = (c - u) + beta m under ``reads_m``, else c - u;  m' = D under ``writes_m``;  a = min(1, r / |D|), a = 1 if r <= 0 or |D| == 0;
               b = (1 - eta) a <D, c> / <c, c>, b = 0 if <c, c> == 0;  den = c + (w - 1)(a D - b c)               (Sadat et al. 2024)
    phi = ``rescale``, r = ``norm_threshold``, beta = ``momentum``.  m' is ``m`` itself (None allowed) where the row does not write it."""
    mode = check_guidance(mode)
    c, u, w = np.asarray(c, dtype=np.float64), np.asarray(u, dtype=np.float64), float(w)
    ax = tuple(range(1, c.ndim))
    per = lambda v: np.asarray(v, dtype=np.float64).reshape((-1,) + (1,) * (c.ndim - 1))  # noqa: E731
    if mode == "cfg":
        return u + w * (c - u), m
    if mode == "rescale":
        phi = float(rescale)
        g = u + w * (c - u)
        sc, sg = c.std(axis=ax), g.std(axis=ax)
        s = np.where(sg == 0.0, 1.0, phi * sc / np.where(sg == 0.0, 1.0, sg) + (1.0 - phi))
        return g * per(s), m
    delta = c - u
    if reads_m:
        delta = delta + float(momentum) * np.asarray(m, dtype=np.float64)
    m_new = delta.copy() if writes_m else m
    nd = np.sqrt((delta * delta).sum(axis=ax))
    r = float(norm_threshold)
    a = np.where((nd == 0.0) | (r <= 0.0), 1.0, np.minimum(1.0, r / np.where(nd == 0.0, 1.0, nd)))
    cc = (c * c).sum(axis=ax)
    b = np.where(cc == 0.0, 0.0, (1.0 - float(eta)) * a * (delta * c).sum(axis=ax) / np.where(cc == 0.0, 1.0, cc))
    return c + (w - 1.0) * (per(a) * delta - per(b) * c), m_new


class GuidedRow(NamedTuple):
    """``guided``: the evaluation runs both rows and combines them; ``first``: it is the first guided evaluation of its stretch (it does not read
    the momentum buffer); ``feeds``: the next evaluation is guided too (this one leaves the momentum buffer for it)"""
    guided: bool
    first: bool
    feeds: bool


def guidance_rows(plan, interval=None) -> List[GuidedRow]:
    """One entry per row of a ``step_plan``: guided iff lo <= sigma <= hi, compared in float32 on the sigma the row's model evaluation runs at
    (Heun's corrector: its own).  None guides every row."""
    lo, hi = check_interval(interval)
    g = [bool(_F(lo) <= _F(r.sigma) <= _F(hi)) for r in plan]
    return [GuidedRow(g[k], g[k] and (k == 0 or not g[k - 1]), g[k] and k + 1 < len(g) and g[k + 1]) for k in range(len(g))]


# ---- skip-layer guidance: a third evaluation with blocks skipped, and the steps that take its term (no reference counterpart) ---------------
def check_skip_layer_guidance(scale, layers, interval, depth):
    """The options of skip-layer guidance -> (scale, layers, (start, stop)): a finite float; the sorted tuple of distinct block indices, at least
    one, each in [0, depth); fractions of the schedule with 0 <= start <= stop <= 1 (None: (0, 1), every step but the first).  Anything else raises a
    ValueError that names the rule."""
    try:
        scale = float(scale)
    except (TypeError, ValueError):
        raise ValueError(f"skip_layer_guidance must be a float (the scale), got {scale!r}") from None
    if not math.isfinite(scale):
        raise ValueError(f"skip_layer_guidance (the scale) must be finite, got {scale}")
    if layers is None or isinstance(layers, (str, bytes)) or len(tuple(layers)) == 0:
        raise ValueError("skip_layers must name at least one block")
    raw = tuple(layers)
    if any(isinstance(b, bool) or int(b) != b for b in raw):
        raise ValueError(f"skip_layers must be block indices (integers), got {raw}")
    out = tuple(sorted(int(b) for b in raw))
    if len(set(out)) != len(out):
        raise ValueError(f"skip_layers names a block twice: {raw}")
    if out[0] < 0 or out[-1] >= int(depth):
        raise ValueError(f"skip_layers {raw}: every block must lie in [0, {int(depth)}), the model's double blocks")
    start, stop = (0.0, 1.0) if interval is None else (float(v) for v in interval)
    if not 0.0 <= start <= stop <= 1.0:
        raise ValueError(f"skip_layer_interval must be (start, stop) with 0 <= start <= stop <= 1, got ({start}, {stop})")
    return scale, out, (start, stop)


def slg_rows(plan, guided_rows, start, stop) -> List[bool]:
    """One bool per row of a ``step_plan``: whether its evaluation takes the skip-layer term.  Step i (0-based) of the plan's n steps takes it iff
    n start < i < n stop, strict on both sides (diffusers' rule for skip_layer_guidance_start / _stop); the rows of a step -- Heun's predictor and
    corrector -- share their step's decision, and a row that ``guided_rows`` (``guidance_rows`` of the same plan) leaves unguided takes no term."""
    n = sum(bool(r.ends_step) for r in plan)
    out, i = [], 0
    for r, g in zip(plan, guided_rows):
        out.append(bool(g.guided and n * float(start) < i < n * float(stop)))
        i += bool(r.ends_step)
    return out


def slg_reference(c, u, k, w, scale, mode="cfg", **kw):
    """``guide_reference`` with the skip-layer term, float64 numpy: ``k`` is the x0 prediction of the prompt rows evaluated with blocks skipped;
    den = G(c, u) + scale (c - k), G the mode's combination.  Returns (den, m') like ``guide_reference``, whose keywords ``kw`` are."""
    den, m_new = guide_reference(c, u, w, mode, **kw)
    c, k = np.asarray(c, dtype=np.float64), np.asarray(k, dtype=np.float64)
    return den + float(scale) * (c - k), m_new


# ---- perturbed-attention guidance: the same third evaluation, through blocks whose image queries attend to the text keys and to themselves -----
def check_perturbed_attention_guidance(scale, layers, interval, depth):
    """The options of perturbed-attention guidance -> (scale, layers, interval): a finite float >= 0; the sorted tuple of distinct block indices, at
    least one, each in [0, depth); None (every guided row carries the term) or fractions of the schedule (start, stop) with 0 <= start <= stop <= 1,
    read by ``slg_rows``.  The term itself is ``slg_reference``'s, with k the perturbed model's prediction.  Anything else raises a ValueError that
    names the rule."""
    try:
        scale = float(scale)
    except (TypeError, ValueError):
        raise ValueError(f"pag_scale must be a float, got {scale!r}") from None
    if not math.isfinite(scale) or scale < 0.0:
        raise ValueError(f"pag_scale must be finite and >= 0, got {scale}")
    if layers is None or isinstance(layers, (str, bytes)) or len(tuple(layers)) == 0:
        raise ValueError("pag_layers must name at least one block")
    raw = tuple(layers)
    if any(isinstance(b, bool) or int(b) != b for b in raw):
        raise ValueError(f"pag_layers must be block indices (integers), got {raw}")
    out = tuple(sorted(int(b) for b in raw))
    if len(set(out)) != len(out):
        raise ValueError(f"pag_layers names a block twice: {raw}")
    if out[0] < 0 or out[-1] >= int(depth):
        raise ValueError(f"pag_layers {raw}: every block must lie in [0, {int(depth)}), the model's double blocks")
    if interval is not None:
        try:
            start, stop = (float(v) for v in interval)
        except (TypeError, ValueError):
            raise ValueError(f"pag_interval must be None or (start, stop), got {interval!r}") from None
        if not 0.0 <= start <= stop <= 1.0:
            raise ValueError(f"pag_interval must be (start, stop) with 0 <= start <= stop <= 1, got ({start}, {stop})")
        interval = (start, stop)
    return scale, out, interval


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
