"""Quantised attention without a GPU: the route of the launch (dk_attention_fp8_plan, host only), its refusals and the workspace size query."""
import pytest

from diffusionkit_amd import _lib, ops

KW = dict(q=4096, k=4096, v=4096, out=4096, B=2, H=3, S=300, D=128, ld=1152, ldo=384, scale=0.1)


@pytest.mark.parametrize("knob", [10, -1])
def test_route(knob):
    """kernel 12 whatever the "attn" knob says: 128-row blocks, pre-pass + attention, + the quantiser pass with an MX-fp8 copy (plain and split rows)"""
    ops.tune("attn", knob)
    try:
        plan = ops.attention_fp8_plan(**KW, score_bound=3.0)
    finally:
        ops.tune("attn", -1)
    assert (plan.kernel, plan.launches, plan.split, plan.jobs, plan.blocks, plan.quantize, plan.untracked) == (12, 2, 1, 0, 2 * 3 * 3, 0, 0)
    o8 = dict(O8=4096, O8_scales=4096, o8_ld=384, o8_rows=600)
    for split, quantize in ((0, 1), (44, 2)):
        plan = ops.attention_fp8_plan(o8_split=split, **KW, **o8)
        assert (plan.kernel, plan.launches, plan.quantize) == (12, 3, quantize)
    assert ops.attention_fp8_plan(**KW, qn_a=4096, qn_b=4096, qn_split=70).qfuse == 1


@pytest.mark.parametrize("change,rule", [(dict(D=64), "head_dim must be 128"), (dict(bias=4096, ldb=320), "no score bias"), (dict(scale=0.0), "positive scale"),
                                         (dict(S=65537, ld=384), "S <= 65536"), (dict(S=60000, ld=36864), "< 4 GiB"),
                                         (dict(workspace_bytes=2 * 3 * 384 * 264 - 1), "workspace smaller"), (dict(qn_a=4096), "qn_b missing")])
def test_refusals_name_their_rule(change, rule):
    with pytest.raises(_lib.DkHipError, match=rule):
        ops.attention_fp8_plan(**{**KW, **change})


def test_workspace_bytes_step_at_multiples_of_128():
    f = ops.attention_fp8_workspace_bytes
    sizes = [f(2, 3, S) for S in range(1, 514)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and [S + 1 for S in range(1, 513) if sizes[S] != sizes[S - 1]] == [129, 257, 385, 513]
    assert f(2, 3, 300) == 2 * 3 * 384 * (128 + 128 + 8) and f(1, 1, 128) * 6 == f(2, 3, 128)  # (test_route passes the query's answer: accepted)


def test_config_refusals():
    from dataclasses import replace
    from diffusionkit_amd import config as C
    C.validate_attention_dtype(replace(C.tiny_flux(), attention_dtype="fp8_e4m3"))
    for cfg, rule in ((replace(C.tiny_sd3(), attention_dtype="fp8_e4m3"), "FLUX geometry"), (replace(C.tiny_flux(), attention_dtype="fp8"), "unknown attention_dtype"),
                      (replace(C.float16_config(C.tiny_sd3()), attention_dtype="fp8_e4m3"), "activation_dtype float16")):
        with pytest.raises(ValueError, match=rule):
            C.validate_attention_dtype(cfg)


def test_cli_flag():
    from diffusionkit_amd import cli
    from diffusionkit_amd.config import MMDIT_CKPT
    parser = cli.build_parser(tuple(MMDIT_CKPT))
    flux, sd3 = (next(k for k in MMDIT_CKPT if ("FLUX" in k) == f) for f in (True, False))
    assert "attention_dtype" not in cli.resolve(parser.parse_args(["--prompt", "p", "--model-version", flux]))
    assert cli.resolve(parser.parse_args(["--prompt", "p", "--model-version", flux, "--attention-dtype", "fp8"]))["attention_dtype"] == "fp8_e4m3"
    with pytest.raises(ValueError, match="FLUX geometry"):
        cli.resolve(parser.parse_args(["--prompt", "p", "--model-version", sd3, "--attention-dtype", "fp8"]))
