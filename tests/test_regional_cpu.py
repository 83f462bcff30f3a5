"""Regional prompts without a GPU: group words from boxes, the refusals of the host side, the route of the grouped launch."""
import numpy as np
import pytest

from diffusionkit_amd import _lib, ops, regional
from tests import _regional as R


@pytest.mark.parametrize("base,isolate", [(True, False), (False, False), (False, True)])
def test_words_from_boxes(base, isolate):
    """a 4 x 6 token grid: region 1's right edge x1 = 40 is exactly the centre of column 2 (excluded: x < x1); region 2 starts there (included)"""
    regions = [{"prompt": "a", "box": (0, 0, 40, 64)}, {"prompt": "b", "box": (40, 0, 96, 64)}]
    got = regional.region_words(regions, 4, 6, 3, base=base, isolate_image=isolate)
    want = R.groups_for(4, 6, [3] * (2 + base), [r["box"] for r in regions], base=base, isolate_image=isolate)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    img = got[3 * (2 + base):].reshape(4, 6)
    shared = 0 if (not base and isolate) else 1
    assert (img[:, :2] == (2 | shared)).all() and (img[:, 2:] == (4 | shared)).all()
    see = R.allowed(got).numpy()
    t1, t2, i1, i2 = 3 * base, 3 * base + 3, 3 * (2 + base), 3 * (2 + base) + 5  # a token of each text and of each region's image part
    assert see[t1, t1] and not see[t1, t2] and see[t1, i1] and not see[t1, i2] and see[i2, t2] and not see[i2, t1] and see[i1, i2] == bool(shared)
    if base:
        assert see[0, i1] and see[0, i2] and see[i1, 0] and not see[0, t1]


def test_host_refusals():
    box = {"prompt": "p", "box": (0, 0, 96, 64)}
    with pytest.raises(ValueError, match="between 1 and 31"):
        regional.region_words([box] * 32, 4, 6, 3)
    with pytest.raises(ValueError, match="lie in no region"):
        regional.region_words([{"prompt": "p", "box": (0, 0, 40, 64)}], 4, 6, 3, base=False)
    with pytest.raises(ValueError, match="zero words"):
        ops.group_words(np.array([1, 0, 2], dtype=np.uint32), 1, 3, "cpu")


def test_words_from_a_mask():
    m = np.zeros((8, 12), dtype=np.uint8)  # on the 4 x 6 grid NEAREST at the cell centres reads pixel (2 y + 1, 2 x + 1): set for columns 0..2 alone
    m[1::2, 1:7:2] = 255
    for mask in (m, np.stack([m * 0, m, m * 0], axis=-1)):  # 2-D and RGB
        assert np.array_equal(regional.region_cells({"prompt": "p", "mask": mask}, 4, 6), regional.region_cells({"prompt": "p", "box": (0, 0, 48, 64)}, 4, 6))


def test_cli_region_parsing():
    assert regional.parse_region("0,16,512,1024:a red fox: close up") == {"prompt": "a red fox: close up", "box": (0.0, 16.0, 512.0, 1024.0)}
    assert regional.parse_region("m.png:sky", mask=True) == {"prompt": "sky", "mask": "m.png"}
    from diffusionkit_amd import cli
    from diffusionkit_amd.config import MMDIT_CKPT
    parser = cli.build_parser(tuple(MMDIT_CKPT))
    flux, sd3 = (next(k for k in MMDIT_CKPT if ("FLUX" in k) == f) for f in (True, False))
    r = cli.resolve(parser.parse_args(["--prompt", "p", "--model-version", flux, "--region", "0,0,512,1024:a fox", "--region-mask", "m.png:sky", "--no-region-base"]))
    assert r["regions"] == [{"prompt": "a fox", "box": (0.0, 0.0, 512.0, 1024.0)}, {"prompt": "sky", "mask": "m.png"}] and r["region_base"] is False
    for extra, rule in ((["--model-version", sd3, "--region", "0,0,5,5:x"], "FLUX"), (["--model-version", flux, "--region-isolate-image"], "need --region"),
                        (["--model-version", flux, "--region", "0,0,5,5:x", "--block-cache", "0.1"], "--block-cache")):
        with pytest.raises(ValueError, match=rule):
            cli.resolve(parser.parse_args(["--prompt", "p"] + extra))
    for bad in ("0,0,10:fox", "0,0,10,10", "10,0,0,10:fox", "a,b,c,d:fox", "0,0,10,10: "):
        with pytest.raises(ValueError):
            regional.parse_region(bad)


def test_route_and_launch_refusals():
    """dk_attention_groups_plan (host only): kernel 11 whatever the "attn" knob says; every refusal names its rule"""
    kw = dict(q=4096, k=4096, v=4096, out=4096, B=2, H=3, S=300, D=128, ld=1152, ldo=384, scale=0.1)
    for knob in (10, -1):  # (ends at the default)
        ops.tune("attn", knob)
        plan = ops.attention_groups_plan(**kw)
        assert (plan.kernel, plan.launches, plan.split, plan.jobs, plan.blocks) == (11, 1, 1, 0, 2 * 3 * 3)
    for change, rule in ((dict(D=64), "head_dim must be 128"), (dict(bias=4096, ldb=320), "no score bias"),
                         (dict(O8=4096, O8_scales=4096, o8_ld=384, o8_rows=600), "no MX-fp8 copy"), (dict(scale=0.0), "positive scale")):
        with pytest.raises(_lib.DkHipError, match=rule):
            ops.attention_groups_plan(**{**kw, **change})


def test_oracle_with_all_ones_words_is_the_plain_oracle():
    import torch
    from diffusionkit_amd.config import tiny_flux
    from diffusionkit_amd.weights import synth_mmdit_weights
    from oracle.mmdit import OracleMMDiT, Prec
    from tests._util import BF, randn
    cfg = tiny_flux()
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    text, pooled, lat = randn(1, 5, cfg.token_level_text_embed_dim, seed=3), randn(1, cfg.pooled_text_embed_dim, seed=4), randn(1, 4, 6, 16, seed=5)

    def final(m):
        m.cache_modulation_params(pooled, torch.tensor([500.0]))
        taps = {}
        m(lat, text, 500.0, taps=taps)
        return taps["final"]
    plain, ones, real = (final(m) for m in (OracleMMDiT(cfg, wf, Prec(BF)), R.RegionalOracle(cfg, wf, Prec(BF), np.full((1, 11), 0xFFFFFFFF, dtype=np.uint32)),
                                            R.RegionalOracle(cfg, wf, Prec(BF), R.groups_for(2, 3, [5], [(0, 0, 24, 32)], base=False)[None])))
    # ... and a real mask reaches the attention: it moves the output by more than twice the absolute term, 2e-3, of the GPU gate
    assert torch.equal(plain, ones) and float((real - plain).norm() / plain.norm()) > 4e-3
