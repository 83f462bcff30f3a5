"""Generator of tests/golden/step_loop_traces.json: what the host step loops (pipeline.sample_euler / sample_steps) ask of the engine and of the
step operators, in order, without a GPU.

    python tests/golden/make_step_loop_traces.py          # rewrites the fixture

The loops run on CPU tensors against three fakes: an engine that records its calls (``forward_head`` answers from a fixed probe sequence, so a
policy's decisions are deterministic), recording stand-ins for the five step wrappers of ``ops`` and ``guidance_workspace_bytes``, and
``torch.cuda.synchronize`` patched to a recorder.  A stand-in keeps the entry name, every scalar argument and which optional buffers are None.  A tree
whose pipeline still launches the Euler step through a private ``_euler`` has that recorded under the name ``euler_cfg_step``: same entry, same
arguments.  Two images, a 4 x 4 x 16 latent, patch 2, a four-entry schedule: the smallest shape with a first, a middle and a last step."""
import json
import os
import sys
from types import SimpleNamespace
from unittest import mock

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from diffusionkit_amd import ops, pipeline  # noqa: E402
from diffusionkit_amd.sampler import BlockCachePolicy, FixedSchedule, ModelSamplingDiscreteFlow, step_plan  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "step_loop_traces.json")
N_IMG, HL, WL, CH, PATCH, TEXT_LEN = 2, 4, 4, 16, 2, 3
SIGMAS = np.array([1.0, 0.7, 0.4, 0.0], dtype=np.float32)
INTERVAL = (0.5, 0.8)  # of the evaluations at 1.0, 0.7, 0.4 only the middle one is guided: unguided at the start, two changes
PROBE = [(4.0, 8.0), (1.0, 8.0), (2.0, 8.0), (0.5, 8.0), (3.0, 8.0), (1.5, 8.0)]  # (num, den) of the k-th head, the same for every batch row


class FakeEngine:
    dtype = torch.bfloat16

    def __init__(self, events):
        self.events, self.heads = events, 0

    def prepare(self, batch, latent_size, text_len, n_timesteps):
        self.batch = int(batch)
        self.events.append(["prepare", int(batch), [int(v) for v in latent_size], int(text_len), int(n_timesteps)])

    def cache_modulation_params(self, pooled, timesteps):
        self.events.append(["cache_modulation_params", int(pooled.shape[0]), [float(t) for t in timesteps]])

    def cache_context(self, text):
        self.events.append(["cache_context", int(text.shape[0])])

    def patchify(self, latent, dup=1):
        self.events.append(["patchify", int(dup)])
        n, hl, wl, c = latent.shape
        return torch.zeros(n * dup, (hl // PATCH) * (wl // PATCH), PATCH * PATCH * c, dtype=self.dtype)

    def enable_block_cache(self, on=True):
        self.events.append(["enable_block_cache", bool(on)])

    def reset_block_cache(self):
        self.events.append(["reset_block_cache"])

    def forward_tokens(self, tokens_in, text, step_index, tokens_out=None):
        self.events.append(["forward_tokens", int(step_index), int(tokens_in.shape[0]), text is None, int(tokens_out.shape[0])])
        return tokens_out

    def forward_head(self, tokens_in, text, step_index):
        self.events.append(["forward_head", int(step_index), int(tokens_in.shape[0]), text is None])
        num, den = PROBE[self.heads % len(PROBE)]
        self.heads += 1
        return torch.tensor([[num, den]] * self.batch, dtype=torch.float32)

    def forward_tail(self, step_index, reuse, tokens_out=None):
        self.events.append(["forward_tail", int(step_index), bool(reuse), int(tokens_out.shape[0])])
        return tokens_out


def _none(**buffers):
    return sorted(k for k, v in buffers.items() if v is None)


def _recorders(events):
    """name -> stand-in, for the attributes of ``ops`` that the loops look up"""

    def common(name, x, model_out, tokens, n_img, cfg_on, p, reshape_order, sigma, sigma_next, cfg_weight):
        return {"op": name, "n_img": int(n_img), "cfg_on": bool(cfg_on), "p": int(p), "reshape_order": int(reshape_order), "sigma": float(sigma),
                "sigma_next": float(sigma_next), "cfg_weight": float(cfg_weight), "x": list(x.shape), "out_rows": int(model_out.shape[0]),
                "tok_rows": int(tokens.shape[0])}

    def row(hist, coef, reads_h, writes_h):
        return {"coef": [float(v) for v in coef], "reads_h": bool(reads_h), "writes_h": bool(writes_h)}

    def euler_cfg_step(*a):
        events.append(common("euler_cfg_step", *a))

    def euler_cfg_step_masked(*a):
        events.append(dict(common("euler_cfg_step_masked", *a[:10]), none=_none(x_orig=a[10], noise=a[11], mask=a[12])))

    def lms_cfg_step(*a):
        events.append(dict(common("lms_cfg_step", *a[:10]), **row(*a[10:14]), none=_none(hist=a[10])))

    def lms_cfg_step_masked(*a):
        events.append(dict(common("lms_cfg_step_masked", *a[:10]), **row(*a[10:14]), none=_none(hist=a[10], x_orig=a[14], noise=a[15], mask=a[16])))

    def guided_cfg_step(*a, mode, workspace, rescale=0.0, eta=0.0, norm_threshold=0.0, momentum=0.0, reads_m=False, writes_m=False, m=None,
                        x_orig=None, noise=None, mask=None):
        events.append(dict(common("guided_cfg_step", *a[:10]), **row(*a[10:14]), mode=mode, rescale=float(rescale), eta=float(eta),
                           norm_threshold=float(norm_threshold), momentum=float(momentum), reads_m=bool(reads_m), writes_m=bool(writes_m),
                           none=_none(hist=a[10], workspace=workspace, m=m, x_orig=x_orig, noise=noise, mask=mask)))

    def guidance_workspace_bytes(*a):
        events.append(["guidance_workspace_bytes"] + [int(v) for v in a])
        return 64

    return {f.__name__: f for f in (euler_cfg_step, euler_cfg_step_masked, lms_cfg_step, lms_cfg_step_masked, guided_cfg_step,
                                    guidance_workspace_bytes)}


def run_case(sampler=None, cfg_weight=5.0, masked=False, block_cache=None, guidance=None):
    """One run of ``sample_euler`` (``sampler`` None) or of ``sample_steps`` over ``step_plan(sampler, SIGMAS)`` -> its trace"""
    events = []
    pipe = SimpleNamespace(mmdit=FakeEngine(events), mmdit_config=SimpleNamespace(patch_size=PATCH, patchify_via_reshape=True), _IS_FLUX=False,
                           device=torch.device("cpu"), sampler=ModelSamplingDiscreteFlow(shift=3.0), timestep_dtype=torch.float16)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N_IMG, HL, WL, CH, generator=g)
    extra = {"conditioning": torch.randn(2, TEXT_LEN, 8, generator=g), "pooled_conditioning": torch.randn(2, 8, generator=g), "cfg_weight": cfg_weight}
    if masked:
        extra.update(mask=torch.ones(1, HL, WL), x_orig=torch.zeros_like(x), noise=torch.zeros_like(x))
    if block_cache is not None:
        extra["block_cache"] = block_cache() if callable(block_cache) else block_cache
    if guidance is not None:
        extra["guidance"] = pipeline._guidance_options(guidance.get("mode"), guidance.get("rescale", 0.7), guidance.get("eta", 0.0),
                                                       guidance.get("norm_threshold", 0.0), guidance.get("momentum", 0.0),
                                                       guidance.get("interval"), cfg_weight)
    model = pipeline.CFGDenoiser(pipe)
    rec = _recorders(events)
    patches = [mock.patch.object(ops, n, f) for n, f in rec.items()]
    if hasattr(pipeline, "_euler"):
        cfg = pipe.mmdit_config
        patches.append(mock.patch.object(pipeline, "_euler", lambda pp, x_, out, tok, cfg_on, s, sn, w: rec["euler_cfg_step"](
            x_, out, tok, x_.shape[0], cfg_on, cfg.patch_size, int(cfg.patchify_via_reshape), s, sn, w)))
    patches.append(mock.patch.object(torch.cuda, "synchronize", lambda *a, **k: events.append(["synchronize"])))
    for p in patches:
        p.start()
    try:
        if sampler is None:
            out, iter_time = pipeline.sample_euler(model, x, SIGMAS, extra_args=extra)
        else:
            out, iter_time = pipeline.sample_steps(model, x, SIGMAS, step_plan(sampler, SIGMAS), extra_args=extra)
    finally:
        for p in reversed(patches):
            p.stop()
    trace = {"events": events, "n_iter_time": len(iter_time), "returns_copy": out is not x and list(out.shape) == list(x.shape),
             "block_cache_record": model.block_cache_record, "guidance_record": model.guidance_record}
    return json.loads(json.dumps(trace))  # (tuples become lists, as in the committed file)


CASES = {
    "euler_cfg_off": dict(cfg_weight=0.0),
    "euler_cfg_on": dict(),
    "euler_masked": dict(masked=True),
    "euler_block_cache": dict(block_cache=lambda: FixedSchedule({1})),
    "heun": dict(sampler="heun"),
    "ab2": dict(sampler="ab2"),
    "ab2_masked": dict(sampler="ab2", masked=True),
    "ab2_block_cache": dict(sampler="ab2", block_cache=0.2),  # (a float: wrapped in a BlockCachePolicy by the loop; rel = 0.5, 0.125, 0.25)
    "euler_plan_rescale": dict(sampler="euler", guidance=dict(mode="rescale", rescale=0.5)),
    "ab2_apg_momentum": dict(sampler="ab2", guidance=dict(mode="apg", eta=0.25, norm_threshold=2.0, momentum=-0.5)),
    "interval_block_cache": dict(sampler="euler", block_cache=lambda: FixedSchedule({1}), guidance=dict(interval=INTERVAL)),
    "interval_apg_momentum": dict(sampler="euler", block_cache=lambda: FixedSchedule({1}),
                                  guidance=dict(mode="apg", momentum=-0.5, interval=INTERVAL)),
    # (Heun evaluates twice at 0.7: a guided stretch of two rows between unguided ones, so that a row feeds the momentum buffer and a row reads it)
    "interval_apg_momentum_heun": dict(sampler="heun", guidance=dict(mode="apg", momentum=-0.5, interval=INTERVAL)),
    "ab2_masked_rescale_policy": dict(sampler="ab2", masked=True, block_cache=lambda: BlockCachePolicy(0.2, max_consecutive_skips=1),
                                      guidance=dict(mode="rescale", rescale=1.0)),
}


def run_all():
    return {name: run_case(**kw) for name, kw in CASES.items()}


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        json.dump(run_all(), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {FIXTURE}")
