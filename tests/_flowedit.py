"""Helpers of the FlowEdit tests (tests/test_flowedit_cpu.py, tests/test_gpu_flowedit.py): the edit loop restated on the oracle with its noise from
``philox_normal_reference`` (stream 1), the synthetic source / target conditioning of the pipeline cases, and the analytic velocity fields.  Plain
numpy / torch; needs no GPU."""
import numpy as np
import torch

from diffusionkit_amd.sampler import FLOWEDIT_STREAM, flowedit_plan, philox_normal_reference
from tests._stochastic import reference_loop
from tests.test_inpaint_cpu import family_inputs

# (T, n_max, n_min, n_avg) of the closed-loop pipeline cases, and the source side's CFG weight where the family runs CFG (the target's is the
# family's own, 5.0)
LOOP_CASES = [(6, 4, 0, 1), (6, 5, 2, 2)]
W_SRC = 2.0
SRC_SCALE = 64.0
HL, WL, SEED = 8, 16, 2  # tests/test_gpu_inpaint.py's latent size and seed


def xi1_of(seeds, draw, shape):
    """float64 [len(seeds), *shape]: image j's normals of draw ``draw`` on the edit's stream"""
    n = int(np.prod(shape))
    return np.stack([philox_normal_reference(s, draw, n, FLOWEDIT_STREAM).reshape(shape) for s in seeds])


def source_inputs(name):
    """(text, pooled) of the SOURCE prompt, laid out like ``family_inputs``' target rows, with the same negative row under CFG.  The prompt row is the
    target's times -SRC_SCALE: on synthetic weights two independent unit-scale prompts move the latent by a few 1e-3 of its norm, which the pipeline
    gates (a few 1e-3 to 1e-2) could not tell from an edit that did nothing; this one moves it by 15 to 25 % (tests/test_flowedit_cpu.py prints and
    gates the figures)"""
    cfg, _, cfgw, text, pooled = family_inputs(name)
    src_t, src_p = text.clone(), pooled.clone()
    src_t[0:1], src_p[0:1] = -SRC_SCALE * text[0:1], -SRC_SCALE * pooled[0:1]
    return src_t, src_p


def edit_rows(src, tar):
    """[src | tar] or, with two rows each ([prompt, negative]), [src+ | tar+ | src- | tar-]: one image's batch rows of the edit"""
    return torch.cat([t for k in range(src.shape[0]) for t in (src[k:k + 1], tar[k:k + 1])], 0)


def oracle_edit_loop(model, x_src, sigmas, n_max, n_min, n_avg, src, tar, w_src, w_tar, act, seeds, t_act=None, sampler="euler"):
    """The whole edit on the oracle, one image: the rows of ``flowedit_plan`` with V the model's output on the activation-rounded inputs, combined
    under CFG as neg + w (pos - neg) in fp32, Z in fp32 like the kernel's, the noise the float64 reference's rounded to float32; with n_min > 0 the
    ordinary loop of ``sampler`` on the cut schedule with the target rows alone (tests/_stochastic.py's ``reference_loop``).  ``src`` / ``tar``:
    (text, pooled) with rows [prompt] or [prompt, negative].  x_src: fp32 [1, h, w, c].  Returns (Z, the final latent), before process_out."""
    cfg_on = w_tar > 0
    text, pooled = edit_rows(src[0], tar[0]), edit_rows(src[1], tar[1])
    timesteps = (t_act or act).r(sigmas * 1000.0)
    model.cache_modulation_params(pooled, timesteps)
    z, zs, zt = x_src.clone(), None, None
    for r in flowedit_plan(sigmas.numpy(), n_max, n_min, n_avg):
        if not r.prime:
            out = model(act.r(torch.cat([zs, zt] * (2 if cfg_on else 1), 0)), text, float(timesteps[r.index]))
            v_src, v_tar = out[0:1], out[1:2]
            if cfg_on:
                v_src = out[2:3] + np.float32(w_src) * (v_src - out[2:3])
                v_tar = out[3:4] + np.float32(w_tar) * (v_tar - out[3:4])
            z = z + np.float32(r.c) * (v_tar - v_src)
        xi = torch.from_numpy(xi1_of(seeds, r.draw, tuple(x_src.shape[1:]))).to(torch.float32)
        zs = np.float32(1.0 - np.float32(r.sigma_in)) * x_src + np.float32(r.sigma_in) * xi
        zt = zs + (z - x_src)
    if n_min == 0:
        return z, z
    cut = len(sigmas) - 1 - n_min
    return z, reference_loop(model, sampler, zt, sigmas[cut:], tar[0], tar[1], w_tar, act, seeds, t_act, first_draw=cut)


# ---- analytic velocity fields for ``flowedit_reference`` ----------------------------------------------------------------------------------------------
def field(z, sigma):
    """a smooth velocity field in float64: depends on the state and on sigma"""
    return np.sin(z) * (1.0 + sigma) - 0.3 * z

