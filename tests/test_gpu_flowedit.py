"""FlowEdit on an MI355X: the step launch (dk_flowedit_step / _f16) against the float64 statement fed the operator's own normals, its tokens against
dk_latent_to_tokens, its noise against dk_philox_normal_f32 bit for bit, its exact identities, batch invariance and a mutant of the reference that the
1e-5 gate must catch; the engine's guidance strength per batch row; and the pipeline (``edit_source_text=``) against the loop restated on the oracle
in tests/_flowedit.py under the project's model-level gates.  Every figure is printed before it is asserted.

Operator shapes: tests/test_gpu_stochastic.py's operands (latent 8 x 12 x 16, p 2, two images) and its ragged 6 x 10 x 16 with three images (240
quads per image: a ragged last workgroup, images that straddle workgroups); pipeline shapes: tests/test_gpu_inpaint.py's."""
import ctypes
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

from diffusionkit_amd.config import tiny_flux
from diffusionkit_amd.sampler import FlowEditRow, cfg_combine, flowedit_row_reference, step_plan
from diffusionkit_amd.weights import pack_mmdit, synth_mmdit_weights
from oracle import pipeline as op
from oracle.mmdit import OracleMMDiT, Prec, embed_dtype
from tests import _flowedit as fe
from tests import _footprint as fp
from tests import test_gpu_guidance as gg
from tests._util import BF, max_abs, psnr, randn, rel_l2
from tests.test_gpu_inpaint import RGB, SEED, pipe_for, same_bits, tokens_of
from tests.test_gpu_stochastic import SEEDS2, SEEDS3, seeds_on
from tests.test_inpaint_cpu import FAMILIES, family_inputs, t_act_of

pytestmark = pytest.mark.gpu

F16 = torch.float16
C, P_ = 16, 2
DRAW = 5
ROW = FlowEditRow(2, float(np.float32(-0.3)), float(np.float32(0.7)), DRAW, False, 3, True)  # (1 - sigma_in is not exact in fp32)
W_SRC, W_TAR = 2.0, 5.0
SHAPES = {2: (8, 12), 3: (6, 10)}  # images -> latent size


def gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def where_of(order, hl, wl):
    """[S_i, F] -> which element of ONE image's latent each token feature is (tests/test_gpu_guidance.py's map, whose image 0 starts at index 0)"""
    return gg.where_of(order, hl, wl)[0]


class Operands:
    """seeded unit-scale operands of one launch; ``step`` runs it on fresh copies and returns (z, zs, zt, tokens)"""

    def __init__(self, dev, order, cfg_on, dt, ld_pad=0, n_img=2):
        self.dev, self.order, self.cfg_on, self.dt, self.n = dev, order, bool(cfg_on), dt, n_img
        self.hl, self.wl = SHAPES[n_img]
        self.s_i, self.f = (self.hl // P_) * (self.wl // P_), P_ * P_ * C
        self.rows = (4 if cfg_on else 2) * n_img
        shape = (n_img, self.hl, self.wl, C)
        self.z, self.x_src = torch.randn(*shape, generator=gen(1)), torch.randn(*shape, generator=gen(3)) * 1.5 + 0.3
        self.out = torch.randn(self.rows, self.s_i, self.f + ld_pad, generator=gen(2)).to(dt)
        self.seeds = SEEDS2 if n_img == 2 else SEEDS3

    def step(self, row=ROW, images=None, out="own", z=None, x_src=None, want_zs=True, w=(W_SRC, W_TAR)):
        from diffusionkit_amd import ops
        imgs = list(range(self.n)) if images is None else images
        k = len(imgs)
        groups = self.rows // self.n
        pick = [g * self.n + j for g in range(groups) for j in imgs]
        z = (self.z if z is None else z)[imgs].to(self.dev).contiguous()
        x_src = (self.x_src if x_src is None else x_src)[imgs].to(self.dev).contiguous()
        o = self.out[pick].to(self.dev).contiguous() if isinstance(out, str) else out
        tok = torch.full((groups * k, self.s_i, self.f), 7.0, dtype=self.dt, device=self.dev)
        zs = torch.full_like(z, 9.0) if want_zs else None
        zt = torch.full_like(z, 9.0)
        ops.flowedit_step(z, x_src, o, tok, zt, k, self.cfg_on, P_, self.order, c=row.c, sigma_in=row.sigma_in, seeds=seeds_on(self.dev, [self.seeds[j] for j in imgs]),
                          draw=row.draw, w_src=w[0], w_tar=w[1], zs_out=zs, prime=row.prime)
        return z, zs, zt, tok

    def velocities(self, swap=False):
        """(V_src, V_tar) in float64, in the latent's layout: the rows unpatchified, combined under CFG"""
        where = where_of(self.order, self.hl, self.wl).reshape(-1)
        per = self.hl * self.wl * C
        u = torch.empty(self.rows, per, dtype=torch.float64)
        u[:, where] = self.out[:, :, :self.f].double().reshape(self.rows, -1)
        u = u.reshape(self.rows, self.hl, self.wl, C).numpy()
        n = self.n
        if not self.cfg_on:
            return u[:n], u[n:2 * n]
        ws, wt = (W_TAR, W_SRC) if swap else (W_SRC, W_TAR)
        return cfg_combine(u[:n], u[2 * n:3 * n], ws), cfg_combine(u[n:2 * n], u[3 * n:], wt)

    def xi(self, draw=DRAW, stream=1):
        from diffusionkit_amd import ops
        return ops.philox_normal(seeds_on(self.dev, self.seeds), self.hl * self.wl * C, draw, stream).reshape(self.z.shape)

    def ref64(self, swap=False, drop_x_src=False):
        """``flowedit_row_reference`` on the fp32 operands and the operator's normals; the two mutants of test_mutant_fails_the_gate"""
        vs, vt = self.velocities(swap)
        z, zs, zt = flowedit_row_reference(self.z.numpy(), self.x_src.numpy(), vs, vt, ROW, self.xi().double().cpu().numpy())
        if drop_x_src:
            zt = zs + z
        return z, zs, zt

    def tokens_ok(self, tok, zs, zt):
        """the source and target token rows are dk_latent_to_tokens of zs_out and zt_out, under CFG in both copies"""
        k, dup = zs.shape[0], 2 if self.cfg_on else 1
        want = tokens_of(torch.cat([zs, zt], 0).contiguous(), self.dt, 2 * k, dup, self.hl, self.wl, C, P_, self.order)
        return same_bits(tok, want) and (not self.cfg_on or same_bits(tok[:2 * k], tok[2 * k:]))


def errs(ref, got):
    return tuple(float(np.abs(r - g.double().cpu().numpy()).max()) for r, g in zip(ref, got))


# ---- 1. the step against float64 ----------------------------------------------------------------------------------------------------------------------
STEP_CASES = [(order, cfg_on, dt, 0) for order in (0, 1) for cfg_on in (False, True) for dt in (BF, F16)] + [(1, True, BF, 8), (0, False, F16, 8)]
step_cases = pytest.mark.parametrize("order,cfg_on,dt,ld_pad", STEP_CASES,
                                     ids=[f"order{o}-cfg{int(c)}-{'bf16' if d == BF else 'f16'}-ld+{l}" for o, c, d, l in STEP_CASES])


@step_cases
def test_step_operator(dev, order, cfg_on, dt, ld_pad):
    """z, zs_out and zt_out within 1e-5 of ``flowedit_row_reference`` fed the normals of ops.philox_normal(..., stream=1), at unit-scale inputs (the bound
    of test_noisy_step_operator); the token rows are the patchified outputs; z moved, and another draw gives other inputs"""
    o = Operands(dev, order, cfg_on, dt, ld_pad)
    z, zs, zt, tok = o.step()
    e = errs(o.ref64(), (z, zs, zt))
    print(f"[flowedit] step order={order} cfg={int(cfg_on)} {dt} ld+{ld_pad}: max_abs z {e[0]:.2e}, zs {e[1]:.2e}, zt {e[2]:.2e}")
    assert max(e) < 1e-5
    assert o.tokens_ok(tok, zs, zt), "tokens are not the patchified zs_out / zt_out"
    assert not same_bits(z, o.z.to(dev)) and not same_bits(zs, o.step(ROW._replace(draw=DRAW + 1))[1])


@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("order", [0, 1], ids=["sd3", "flux"])
def test_step_operator_ragged(dev, order, dt):
    """latent 6 x 10 x 16, three images with three seeds, CFG on: the same gate and the same token check"""
    o = Operands(dev, order, True, dt, n_img=3)
    z, zs, zt, tok = o.step()
    e = errs(o.ref64(), (z, zs, zt))
    print(f"[flowedit] ragged step order={order} {dt}: max_abs z {e[0]:.2e}, zs {e[1]:.2e}, zt {e[2]:.2e}")
    assert max(e) < 1e-5 and o.tokens_ok(tok, zs, zt)


@pytest.mark.parametrize("mutant", ["swapped-weights", "no-x_src"])
def test_mutant_fails_the_gate(dev, mutant):
    """the reference with the source and target CFG weights swapped, or with Zt = Zs + Z: the launch is far outside 1e-5 of either, so the gate of
    test_step_operator sees the arithmetic it is there for"""
    o = Operands(dev, 0, True, BF)
    got = o.step()[:3]
    e = errs(o.ref64(swap=mutant == "swapped-weights", drop_x_src=mutant == "no-x_src"), got)
    print(f"[flowedit] mutant {mutant}: max_abs z {e[0]:.2e}, zs {e[1]:.2e}, zt {e[2]:.2e}")
    assert max(e) > 1e-3 and max(errs(o.ref64(), got)) < 1e-5


# ---- 2. the noise is the operator's, on stream 1 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("order", [0, 1], ids=["sd3", "flux"])
def test_noise_is_the_operators(dev, order, dt):
    """c = 0, x_src = 0, sigma_in = 1: zs_out is ops.philox_normal(seeds, n, draw, stream=1) bit for bit, up to the sign of a zero; not stream 0's, not
    the next draw's"""
    o = Operands(dev, order, True, dt)
    zero = torch.zeros_like(o.x_src)
    z, zs, zt, tok = o.step(ROW._replace(c=0.0, sigma_in=1.0), x_src=zero)
    xi = o.xi()
    differ = fp.bits(zs) != fp.bits(xi)  # (allowed only between +0 and -0)
    assert bool(torch.isfinite(zs).all()) and bool((zs.cpu()[differ.cpu()] == 0.0).all()) and bool((xi.cpu()[differ.cpu()] == 0.0).all()), \
        f"{int(differ.sum())} elements differ from the operator's, beyond the sign of a zero"
    assert same_bits(z, o.z.to(dev))  # (c = 0 over finite rows)
    assert not same_bits(zs, o.xi(stream=0)) and not same_bits(zs, o.xi(draw=DRAW + 1))
    assert o.tokens_ok(tok, zs, zt)


# ---- 3. identities ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,cfg_on,dt", [(0, True, BF), (1, False, F16)], ids=["sd3-cfg-bf16", "flux-f16"])
def test_identities(dev, order, cfg_on, dt):
    """(a) identical source and target rows with w_src == w_tar: z keeps its bits; with z == x_src, zt_out has the bits of zs_out.  (b) prime = 1 does not
    read model_out -- a NaN-filled one between sentinel margins, or none at all -- and leaves z alone.  (c) zs_out = None: the other outputs keep
    their bits"""
    o = Operands(dev, order, cfg_on, dt)
    n = o.n
    same = o.out.clone()
    same[n:2 * n] = same[:n]
    if cfg_on:
        same[3 * n:] = same[2 * n:3 * n]
    z, zs, zt, tok = o.step(out=same.to(dev), w=(W_TAR, W_TAR))
    assert same_bits(z, o.z.to(dev))
    z, zs, zt, tok = o.step(out=same.to(dev), w=(W_TAR, W_TAR), z=o.x_src)
    assert same_bits(z, o.x_src.to(dev)) and same_bits(zt, zs) and o.tokens_ok(tok, zs, zt)
    # (b)
    prime = ROW._replace(prime=True, c=0.0)
    clean = o.step(prime)
    poison, guard = fp.guarded(torch.full(tuple(o.out.shape), fp.NAN, device=dev).to(dt), 8, fp.SENTINEL)
    got = o.step(prime, out=poison)
    guard.check("model_out")
    none = o.step(prime, out=None)
    for name, a, b, c in zip(("z", "zs", "zt", "tokens"), clean, got, none):
        assert same_bits(a, b) and same_bits(a, c), f"prime: {name} depends on model_out"
    assert same_bits(clean[0], o.z.to(dev)) and bool(torch.isfinite(clean[2]).all())
    assert not same_bits(clean[2], o.step()[2])  # (the unprimed launch moved z, and zt with it)
    # (c)
    full, bare = o.step(), o.step(want_zs=False)
    assert bare[1] is None and all(same_bits(a, b) for a, b in zip((full[0], full[2], full[3]), (bare[0], bare[2], bare[3])))


# ---- 4. batch invariance -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF, F16], ids=["bf16", "f16"])
def test_batch_invariance_of_the_operator(dev, dt):
    """image j of three (6 x 10 x 16: the images straddle workgroups) equals its single-image launch bit for bit, tokens included"""
    o = Operands(dev, 0, True, dt, n_img=3)
    z3, zs3, zt3, tok3 = o.step()
    for j in range(3):
        z1, zs1, zt1, tok1 = o.step(images=[j])
        for name, a, b in (("z", z3, z1), ("zs", zs3, zs1), ("zt", zt3, zt1)):
            assert same_bits(a[j:j + 1], b), f"{name} of image {j} differs from its single launch"
        assert same_bits(tok3[[j, 3 + j, 6 + j, 9 + j]], tok1), f"tokens of image {j}"


def test_operator_refuses(dev):
    from diffusionkit_amd import ops
    from diffusionkit_amd._lib import DkHipError
    o = Operands(dev, 0, True, BF)
    z, x, out = o.z.to(dev), o.x_src.to(dev), o.out.to(dev)
    tok, zt, sd = torch.empty(o.rows, o.s_i, o.f, dtype=BF, device=dev), torch.empty_like(z), seeds_on(dev, o.seeds)
    kw = dict(c=-0.1, sigma_in=0.5, seeds=sd, draw=1)
    for args, text in (((z, x, out[:4], tok, zt, 2, True, P_, 0), "model_out"), ((z, x, out, tok[:4], zt, 2, True, P_, 0), "tokens"),
                       ((z, x[:1], out, tok, zt, 2, True, P_, 0), "x_src"), ((z, x, None, tok, zt, 2, True, P_, 0), "model_out is None"),
                       ((z, x, out.to(F16), tok, zt, 2, True, P_, 0), "model_out")):
        with pytest.raises(DkHipError, match=text):
            ops.flowedit_step(*args, **kw)
    with pytest.raises(DkHipError, match="seeds"):
        ops.flowedit_step(z, x, out, tok, zt, 2, True, P_, 0, **dict(kw, seeds=sd[:1]))
    with pytest.raises(DkHipError, match="must be finite"):
        ops.flowedit_step(z, x, out, tok, zt, 2, True, P_, 0, **dict(kw, c=float("nan")))


# ---- 5. the engine: guidance strength per batch row ------------------------------------------------------------------------------------------------------
def mod_table(eng, n_t, dev):
    """a copy of the engine's modulation table [n_t * B, mod_rows * h] (dk_mmdit_debug_buffer, as tests/test_gpu_model.py reads it)"""
    torch.cuda.synchronize()
    tab = torch.empty(n_t * eng.batch, eng.mod_rows() * eng.config.hidden_size, dtype=BF, device=dev)
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(tab.data_ptr()), ctypes.c_void_p(eng.lib.dk_mmdit_debug_buffer(eng._h, 1)), ctypes.c_size_t(tab.numel() * 2), 3) == 0
    return tab


def test_guidance_rows(dev):
    """rows [g, g]: the modulation table and the output have the bits of scalar g.  Rows [g1, g2]: batch row b follows the oracle at g_b under the
    gate of tests/test_gpu_fp8.py::test_guidance_embedding (the yardstick on the model's output), and its table rows are within
    test_modulation_table_matches_oracle's 1.5e-2 of the emulating oracle's.  Unsetting the rows restores the scalar's bits."""
    from diffusionkit_amd.engine import MMDiTEngine
    from tests.test_gpu_model import yardstick_ok
    cfg = replace(tiny_flux(), guidance_embed=True)
    named = synth_mmdit_weights(cfg, seed=1234)
    eng = MMDiTEngine(cfg, pack_mmdit(cfg, named, dev))
    B, ts, g1, g2 = 2, [1000.0, 752.0], 3.5, 1.0
    text, pooled, lat = randn(B, 20, cfg.token_level_text_embed_dim, seed=3), randn(B, cfg.pooled_text_embed_dim, seed=4), randn(B, 8, 12, 16, seed=5)
    eng.prepare(B, (8, 12), 20, len(ts))
    tok = eng.patchify(lat.to(dev))

    def run(rows=None):
        eng.cache_modulation_params(pooled.to(dev), ts, **({} if rows is None else {"guidance_rows": rows}))
        out = eng.forward_tokens(tok, text.to(dev, BF), 1).clone()
        return mod_table(eng, len(ts), dev), out
    eng.guidance = g1
    tab_s, out_s = run()
    tab_r, out_r = run([g1, g1])
    assert same_bits(tab_r, tab_s) and same_bits(out_r, out_s), "rows [g, g] differ from scalar g"
    tab_m, out_m = run([g1, g2])
    assert same_bits(tab_m[0::B], tab_s[0::B]) and not same_bits(tab_m[1::B], tab_s[1::B])  # (row 0 sees g1 as before, row 1 something else)
    wf = {k: v.float() for k, v in named.items()}
    for b, g in enumerate((g1, g2)):
        ref = {}
        for name, P in (("fp32", Prec()), ("emu", Prec(BF))):
            m = OracleMMDiT(cfg, wf, P, guidance=g)
            m.cache_modulation_params(pooled[b:b + 1], torch.tensor(ts))
            taps = {}
            m(lat[b:b + 1], text[b:b + 1], ts[1], taps=taps)
            ref[name] = taps["final"]
            if name == "emu":
                from diffusionkit_amd.weights import adaln_order
                off = 0
                for mname in adaln_order(cfg):
                    n = m._mod[mname][ts[0]].shape[-1]
                    for si, t in enumerate(ts):
                        assert rel_l2(m._mod[mname][t][:, 0], tab_m[si * B + b:si * B + b + 1, off:off + n].float().cpu()) < 1.5e-2, (mname, t, b)
                    off += n
        e_h, e_e = yardstick_ok(out_m[b:b + 1].float().cpu(), ref["emu"], ref["fp32"], f"guidance row {b} = {g}")
        print(f"[flowedit] guidance rows: batch row {b} at g = {g}: hip-vs-fp32 {e_h:.3e}, emu-vs-fp32 {e_e:.3e}")
    tab_u, out_u = run()
    assert same_bits(tab_u, tab_s) and same_bits(out_u, out_s), "unsetting the rows does not restore the scalar's bits"
    from diffusionkit_amd._lib import DkHipError
    with pytest.raises(DkHipError, match="guidance_rows holds 3 values"):
        eng.cache_modulation_params(pooled.to(dev), ts, guidance_rows=[1.0, 2.0, 3.0])


# ---- 6. the pipeline -------------------------------------------------------------------------------------------------------------------------------------------
def x_src_of(pipe):
    """the pipeline's own x_src: the posterior mean of the encoded image after process_in"""
    return pipe.latent_format.process_in(pipe.encode_mean_latents(pipe.read_image(RGB))).to(torch.float32).contiguous()


def edited(pipe, family, dev, case, seed=SEED, src=None, w_src=fe.W_SRC, **kw):
    cfg, _, cfgw, text, pooled = family_inputs(family)
    T, n_max, n_min, n_avg = case
    src_t, src_p = fe.source_inputs(family) if src is None else src
    lat, iter_time = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=T, cfg_weight=cfgw, seed=seed, image_path=RGB,
                                          edit_source_text=(src_t.to(dev, BF), src_p.to(dev, BF)), edit_steps=(n_max, n_min), edit_n_avg=n_avg,
                                          **({"edit_source_cfg": w_src} if cfgw > 0 else {}), **kw)
    n = len(seed) if isinstance(seed, list) else 1
    assert lat.shape == (n, fe.HL, fe.WL, 16) and lat.dtype == torch.float32 and len(iter_time) == n_max
    return lat


@functools.lru_cache(maxsize=None)
def loop_references(family, case, x_key):
    """tests/_flowedit.py's loop on the fp32 and the bf16-emulating oracle, after process_out.  Both start from the pipeline's own x_src (``x_key``: its
    bytes): the test is about the edit loop, and the VAE encoder has its own tests (as tests/test_gpu_inpaint.py's fp16 case argues)"""
    cfg, shift, cfgw, text, pooled = family_inputs(family)
    wf = {k: v.float() for k, v in synth_mmdit_weights(cfg, seed=1234).items()}
    T, n_max, n_min, n_avg = case
    sigmas = op.get_sigmas(shift, cfg.is_flux, T)
    x_src = torch.from_numpy(np.frombuffer(x_key, dtype=np.float32).reshape(1, fe.HL, fe.WL, 16).copy())
    return {pname: op.process_out(fe.oracle_edit_loop(OracleMMDiT(cfg, wf, P), x_src, sigmas, n_max, n_min, n_avg, fe.source_inputs(family), (text, pooled),
                                                      fe.W_SRC, cfgw, Prec(BF), [SEED], t_act_of(cfg))[1], "flux" if cfg.is_flux else "sd3")
            for pname, P in (("fp32", Prec()), ("emu", Prec(BF)))}


@pytest.mark.parametrize("case", fe.LOOP_CASES, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_pipeline_parity(dev, family, case):
    """tiny FLUX and tiny SD3 + CFG (source 2, target 5): the gates of tests/test_gpu_stochastic.py::test_pipeline_parity -- err(hip) <= 2 err(bf16-emulating
    oracle) + 2e-3, and 35 dB where the emulating oracle reaches 37 dB -- and the bookkeeping: n_avg (n_max - n_min) + n_min evaluations"""
    from tests.test_gpu_model import yardstick_ok
    pipe = pipe_for(family, dev)
    T, n_max, n_min, n_avg = case
    lat = edited(pipe, family, dev, case)
    x_src = x_src_of(pipe)
    res = loop_references(family, case, x_src.cpu().numpy().tobytes())
    p_h, p_e = psnr(res["fp32"], lat), psnr(res["fp32"], res["emu"])
    moved = rel_l2(lat, pipe.latent_format.process_out(x_src))
    print(f"[flowedit] {family} {case}: rel_l2 hip {rel_l2(res['fp32'], lat):.3e} / emu {rel_l2(res['fp32'], res['emu']):.3e}, PSNR hip {p_h:.1f} dB / emu "
          f"{p_e:.1f} dB; the edit moved the latent by {moved:.3e} of its norm")
    yardstick_ok(lat, res["emu"], res["fp32"], f"{family} {case}")
    if p_e >= 37.0:
        assert p_h > 35.0, f"{family} {case}: PSNR {p_h:.1f} dB"
    cfg_on = FAMILIES[family][2] > 0
    e = pipe.last_edit
    assert e["model_evals"] == n_avg * (n_max - n_min) + n_min and e["tail_evals"] == n_min and e["draws"] == 1 + n_avg * (n_max - n_min)
    assert (e["n_max"], e["n_min"], e["n_avg"], e["rows"]) == (n_max, n_min, n_avg, 4 if cfg_on else 2)
    assert (e["source_cfg"], e["target_cfg"]) == ((fe.W_SRC, 5.0) if cfg_on else (None, None)) and e["guidance_rows"] is None
    assert pipe.last_sampler == {"sampler": "euler", "model_evals": e["model_evals"]}


def test_pipeline_parity_f16(dev):
    """activation_dtype = "float16", SD3 + CFG, (6, 4, 0, 1): the gates of tests/test_gpu_f16_model.py's pipeline test"""
    from tests.test_gpu_f16_model import f16_weights, gate
    family, case = "sd3_cfg", fe.LOOP_CASES[0]
    pipe = pipe_for(family, dev, f16=True)
    assert pipe.mmdit.dtype == F16
    lat = edited(pipe, family, dev, case)
    cfg, shift, cfgw, text, pooled = family_inputs(family)
    _, wf = f16_weights(cfg)
    T, n_max, n_min, n_avg = case
    sigmas = op.get_sigmas(shift, False, T)
    x_src = x_src_of(pipe).cpu()
    res = {}
    for oname, (m, act) in {"fp32": (OracleMMDiT(cfg, wf, Prec(), embed_prec=Prec(embed_dtype(cfg))), Prec(F16)),
                            "emu16": (OracleMMDiT(cfg, wf, Prec(F16)), Prec(F16)), "emubf": (OracleMMDiT(cfg, wf, Prec(BF)), Prec(BF))}.items():
        res[oname] = op.process_out(fe.oracle_edit_loop(m, x_src, sigmas, n_max, n_min, n_avg, fe.source_inputs(family), (text, pooled), fe.W_SRC, cfgw, act,
                                                        [SEED], Prec(F16))[1], "sd3")
    gate(lat, res["emu16"], res["emubf"], res["fp32"], "flowedit f16")


@pytest.mark.parametrize("family", list(FAMILIES))
def test_equal_prompts_return_the_source(dev, family):
    """target prompt == source prompt with equal weights: the source and the target rows of every evaluation are the same data through the same code,
    V_tar - V_src is an exact zero, and the result is x_src bit for bit"""
    pipe = pipe_for(family, dev)
    _, _, cfgw, text, pooled = family_inputs(family)
    lat = edited(pipe, family, dev, (6, 4, 0, 2), src=(text, pooled), w_src=cfgw)
    want = pipe.latent_format.process_out(x_src_of(pipe))
    print(f"[flowedit] {family} equal prompts: max_abs against x_src {max_abs(want, lat):.3e}")
    assert same_bits(lat, want), "the engine's source and target rows are not bit-equal"


@pytest.mark.parametrize("family", list(FAMILIES))
def test_determinism_and_seed_lists(dev, family):
    """the same seed gives the same bits, another seed other bits; seed = [2, 3, 4] gives each image the bits of its single-seed run"""
    pipe = pipe_for(family, dev)
    case = fe.LOOP_CASES[1]
    three = edited(pipe, family, dev, case, seed=[2, 3, 4])
    for i, s in enumerate((2, 3, 4)):
        one = edited(pipe, family, dev, case, seed=s)
        print(f"[flowedit] {family} seed list: image {i} (seed {s}) against its single-seed run: max_abs {max_abs(three[i:i + 1], one):.3e}")
        assert same_bits(three[i:i + 1], one), f"image {i} of the seed list differs from the single-seed run"
    assert same_bits(edited(pipe, family, dev, case, seed=3), three[1:2]) and not same_bits(three[0:1], three[1:2])


@pytest.mark.parametrize("family", list(FAMILIES))
def test_tail_is_the_ordinary_loop(dev, family):
    """n_min = 2 under sampler "euler_a": the edit phase by hand (``sample_flowedit``), then ``sample_steps`` on Zt over the cut schedule with the target
    rows alone, gives the pipeline's bits"""
    from diffusionkit_amd.pipeline import CFGDenoiser, sample_flowedit, sample_steps
    pipe = pipe_for(family, dev)
    cfg, _, cfgw, text, pooled = family_inputs(family)
    case = T, n_max, n_min, n_avg = fe.LOOP_CASES[1]
    lat = edited(pipe, family, dev, case, sampler="euler_a")
    assert pipe.last_sampler["noise_draws"] == n_min - 1 and pipe.last_edit["tail_evals"] == n_min
    src_t, src_p = fe.source_inputs(family)
    den = CFGDenoiser(pipe)
    sigmas = pipe.get_sigmas(pipe.sampler, T)
    args = dict(conditioning=fe.edit_rows(src_t, text).to(dev, BF), pooled_conditioning=fe.edit_rows(src_p, pooled).to(dev, BF), cfg_weight=cfgw,
                noise_seeds=[SEED], edit_source_cfg=fe.W_SRC)
    z, zt, iter_time = sample_flowedit(den, x_src_of(pipe), sigmas, n_max, n_min, n_avg, extra_args=args)
    assert len(iter_time) == n_max - n_min and den.flowedit_record["model_evals"] == n_avg * (n_max - n_min) and not same_bits(z, zt)
    cut = T - n_min
    plan = step_plan("euler_a", sigmas[cut:], None, first_draw=cut)
    out, _ = sample_steps(den, zt, sigmas[cut:], plan, extra_args=dict(conditioning=text.to(dev, BF), pooled_conditioning=pooled.to(dev, BF),
                                                                       cfg_weight=cfgw, noise_seeds=[SEED]))
    assert same_bits(pipe.latent_format.process_out(out), lat)
    assert not same_bits(lat, edited(pipe, family, dev, case))  # (the Euler tail is another result)


def test_default_is_untouched(dev, monkeypatch):
    """without edit_source_text: generate_image launches what it launched -- one dk_euler_cfg_step per step, never the new entry, and the engine is never
    told about guidance rows -- and the keywords at their defaults give the bits of the call without them"""
    from diffusionkit_amd import ops
    pipe = pipe_for("flux", dev)
    calls = []
    for name in ("euler_cfg_step", "flowedit_step", "lms_cfg_step", "noisy_cfg_step"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _f=real, **k: (calls.append(_n), _f(*a, **k))[1])
    kw = dict(num_steps=4, latent_size=(fe.HL, fe.WL), seed=SEED, verbose=False)
    img, log = pipe.generate_image("a cat", **kw)
    assert calls == ["euler_cfg_step"] * 4 and "edit" not in log["denoising"] and pipe.last_edit is None
    assert not getattr(pipe.mmdit, "_guidance_rows_set", False)
    img2, _ = pipe.generate_image("a cat", edit_source_text=None, edit_steps=None, edit_n_avg=None, edit_source_cfg=None, **kw)
    assert np.array_equal(np.asarray(img), np.asarray(img2)) and calls == ["euler_cfg_step"] * 8
    _, _, _, text, pooled = family_inputs("flux")
    a, _ = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=4, cfg_weight=0.0, latent_size=(fe.HL, fe.WL), seed=SEED)
    edited(pipe, "flux", dev, fe.LOOP_CASES[0])  # (an edit in between leaves nothing behind)
    b, _ = pipe.denoise_latents(text.to(dev, BF), pooled.to(dev, BF), num_steps=4, cfg_weight=0.0, latent_size=(fe.HL, fe.WL), seed=SEED)
    assert same_bits(a, b) and pipe.last_edit is None


def test_generate_image_and_cli(dev, tmp_path):
    """generate_image(edit_source_text=) logs what ran; --edit-source-prompt reaches it; the refusals raise with their texts on a live pipeline"""
    from PIL import Image
    from diffusionkit_amd import cli
    from diffusionkit_amd.config import tiny_vae, tiny_vae_encoder
    pipe = pipe_for("sd3_cfg", dev)
    img, log = pipe.generate_image("a dog", num_steps=6, cfg_weight=5.0, seed=SEED, verbose=False, image_path=RGB, edit_source_text="a cat",
                                   edit_steps=(4, 1), edit_n_avg=2, edit_source_cfg=2.0)
    e = log["denoising"]["edit"]
    assert img.size == (RGB.shape[1], RGB.shape[0]) and e["model_evals"] == 2 * 3 + 1 and e["rows"] == 4 and len(log["denoising"]["iter_time"]) == 4
    for kw, text in ((dict(mask_path=np.zeros(RGB.shape[:2], dtype=np.uint8)), "mask_path"), (dict(block_cache=0.1), "block_cache"),
                     (dict(denoise=0.5), "denoise"), (dict(edit_steps=(7, 0)), "exceeds num_steps"), (dict(guidance="rescale"), "guidance mode")):
        with pytest.raises(ValueError, match=text):
            pipe.generate_image("a dog", num_steps=6, cfg_weight=5.0, seed=SEED, verbose=False, image_path=RGB, edit_source_text="a cat", **kw)
    path = tmp_path / "in.png"
    Image.fromarray(RGB).save(path)
    over = dict(mmdit_config=tiny_flux(), vae_config=tiny_vae(), vae_encoder_config=tiny_vae_encoder(), text_len=20)
    argv = ["--prompt", "a dog", "--steps", "4", "--seed", "7", "--image-path", str(path), "-o", str(tmp_path / "out.png"), "--edit-source-prompt", "a cat"]
    img, log = cli.main(argv + ["--edit-steps", "3", "1", "--edit-n-avg", "2"], pipeline_overrides=over)
    e = log["denoising"]["edit"]
    assert img.size == (RGB.shape[1], RGB.shape[0]) and (e["n_max"], e["n_min"], e["n_avg"], e["model_evals"], e["rows"]) == (3, 1, 2, 5, 2)
    _, log = cli.main(argv, pipeline_overrides=over)  # (the defaults: 24 / 28 of 4 steps, rounded: 3, and n_min 0)
    assert (log["denoising"]["edit"]["n_max"], log["denoising"]["edit"]["n_min"]) == (3, 0)
