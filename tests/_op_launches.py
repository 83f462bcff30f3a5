"""The operator launches of the footprint families (tests/_footprint.py), shared by tests/test_gpu_op_footprints.py (NaN footprints) and
tests/test_gpu_address_boundaries.py (operands across 4 GiB address multiples).

A launch here is ``launch(v)``: ``v`` maps operand names to device tensors -- the family's inputs, the outputs the caller owns ("out", "C", "C2",
"tok0", "tok") and, where the launch takes one, the workspace ("ws": the GEMM / conv K-split scratch; "attn_ws": the attention key-split scratch).
It returns the output tensor or a dict of them.  Nothing is asserted here: what a test demands of a launch stays in that test.

``SPECS`` is the catalogue the address tests walk: one ``Spec`` per launch form, built on the first use."""
import math
from contextlib import contextmanager

import torch

from tests import _footprint as fp
from tests import _fp8 as f8
from tests import _fused_cases as fc
from tests._util import TOL_SINGLE_OP

BF, F16 = torch.bfloat16, torch.float16
SENTINEL = fp.SENTINEL
TOL_F16 = TOL_SINGLE_OP / 8  # tests/test_gpu_f16_ops.py


@contextmanager
def tuned(**knobs):
    """ops.tune(key, value) for the block, the defaults afterwards (conv_v4's default is 1)"""
    from diffusionkit_amd import ops
    try:
        for k, v in knobs.items():
            ops.tune(k, v)
        yield
    finally:
        for k in knobs:
            ops.tune(k, 1 if k == "conv_v4" else -1)


def _ws(v):
    ws = v.get("ws")
    return dict(workspace=ws.data_ptr(), workspace_bytes=ws.numel()) if ws is not None else {}


# ---- GEMM ---------------------------------------------------------------------------------------------------------------------------
GEMM_FORMS = [("bf16_128", BF, dict(gemm=128)), ("bf16_v3_mf8", BF, dict(gemm=9, gemm_mf=8)), ("bf16_v3_mf7", BF, dict(gemm=9, gemm_mf=7)),
              ("bf16_v4", BF, dict(gemm=10)), ("f16_auto", F16, dict(gemm=-1)), ("f16_v3", F16, dict(gemm=9))]


def gemm_joint_desc(v, B, S_t, S_i, epi, h=192, N=512):
    """dk_gemm_desc fields of the text stream of a joint [B, S_t + S_i] buffer (test_gemm_v3_ragged_and_straddling_segments)"""
    from diffusionkit_amd import ops
    S = S_t + S_i
    kw = dict(A=v["att"], W=v["w"], C=v["X"], bias=v["b"], M=B * S_t, N=N, K=h, lda=h, ldc=N, a_seg_len=S_t, a_seg_stride=S, c_seg_len=S_t,
              c_seg_stride=S, alpha=1.0, epilogue=ops.DK_EPI_BIAS, **_ws(v))
    if epi == "gate_res":
        kw.update(epilogue=ops.DK_EPI_GATE_RES, res=v["X"], ldr=N, r_seg_len=S_t, r_seg_stride=S, gate=v["gate"].data_ptr() + N * 2,
                  gate_seg_len=S_t, gate_stride=2 * N)
    return kw


def gemm_joint(dt, knobs, B, S_t, S_i, epi):
    from diffusionkit_amd import ops

    def launch(v):
        with tuned(**knobs):
            ops.gemm_desc_call(dtype=dt, **gemm_joint_desc(v, B, S_t, S_i, epi))
        return v["X"]
    return launch


def gemm_ksplit(split):
    """test_gemm_v3_remainder_split's launch: gate + residual on gemm256v3.hip, the remainder tiles cut along K (``split`` 1) or not (0)"""
    from diffusionkit_amd import ops

    def launch(v):
        M = v["x"].shape[0]
        with tuned(gemm=9, gemm_mf=8, gemm_split=split):
            return ops.linear(v["x"], v["w"], v["b"], epilogue=ops.DK_EPI_GATE_RES, gate=v["gate"], res=v["res"], gate_seg_len=M, out=v.get("out"),
                              workspace=v["ws"])
    return launch


def fused_args(call, v):
    ws = v.get("ws")
    return fc.resolve(call, lambda name: v[name].data_ptr(), ws.numel() if ws is not None else 0)


def fused(call):
    """dk_gemm_fused_bf16 of a tests/_fused_cases.py call on the buffers ``v`` names"""
    from diffusionkit_amd import ops

    def launch(v):
        with tuned(**call.tune):
            ops.gemm_fused_call(*fused_args(call, v))
    return launch


# ---- attention ------------------------------------------------------------------------------------------------------------------------
# (id, dtype, knobs, (B, H, S, D), query block of the kernel: attention2.hip QB = NW * 32 = 128, attention4.hip 256, attention5.hip 4 waves x 64)
ATTN_FORMS = [("lean_100_d64", BF, dict(attn=4), (2, 2, 100, 64), 128), ("lean_129_d128", BF, dict(attn=4), (2, 2, 129, 128), 128),
              ("alt_129", BF, dict(attn=9), (2, 2, 129, 128), 256), ("alt_250", BF, dict(attn=9), (1, 2, 250, 128), 256),
              ("wave_768", BF, dict(attn=10), (2, 2, 768, 128), 256), ("wave_key_split_3072", BF, dict(attn=10, attn_split=2), (1, 2, 3072, 128), 256),
              ("f16_lean_100_d64", F16, dict(), (2, 2, 100, 64), 128)]


def attention_desc(v, B, H, S, D, **extra):
    h = H * D
    base = v["qkv"].data_ptr()
    return dict(q=base, k=base + 2 * h, v=base + 4 * h, out=v["out"], B=B, H=H, S=S, D=D, ld=3 * h, ldo=h, scale=1.0 / math.sqrt(D), **extra)


@contextmanager
def attention_workspace(v):
    """the key-split scratch of the calling thread is ``v["attn_ws"]`` for the block (dk_attention_set_workspace), the library's own afterwards"""
    from diffusionkit_amd import _lib
    ws = v.get("attn_ws")
    if ws is None:
        _lib.ensure_attention_workspace(torch.cuda.current_device())
        yield
        return
    lib = _lib.load()
    _lib.ensure_attention_workspace(torch.cuda.current_device())
    _lib.check(lib.dk_attention_set_workspace(ws.data_ptr(), ws.numel()), "dk_attention_set_workspace")
    try:
        yield
    finally:
        torch.cuda.synchronize()
        lib.dk_attention_set_workspace(None, 0)
        _lib.forget_attention_workspace()


def attention(dt, knobs, B, H, S, D, extra=lambda v: {}):
    """dk_attention_desc_* on the packed ``v["qkv"]`` into ``v["out"]``; ``extra(v)``: further descriptor fields (fused Q load, score bound)"""
    from diffusionkit_amd import ops

    def launch(v):
        with tuned(**knobs), attention_workspace(v):
            ops.attention_desc_call(dtype=dt, **attention_desc(v, B, H, S, D, **extra(v)))
        return v["out"]
    return launch


def attention_q_extra(c):
    """descriptor fields of the fused Q load of a tests/_fused_cases.py ATTN_Q case: operands "qa", "qb", "rope" of ``v``"""
    def extra(v):
        return dict(qn_a=v["qa"] if c["norm"] else None, qn_b=v["qb"] if c["norm"] else None, qn_split=c["split"], qn_eps=fc.KN_EPS,
                    q_rope=v.get("rope"))
    return extra


def attention_mx8(c):
    """attention with the MX-fp8 copy of the output (ATTN_O8 case): "out", "o8" [M, h] bytes and "o8_scales" of ``v``"""
    B, H, S, D = c["B"], c["H"], c["S"], c["D"]
    h, M = H * D, B * S
    return attention(BF, dict(attn=c["mode"], attn_split=0), B, H, S, D,
                     lambda v: dict(O8=v["o8"], O8_scales=v["o8_scales"], o8_ld=h, o8_rows=M))


# ---- convolutions ------------------------------------------------------------------------------------------------------------------------
def conv(form, res, knobs=None):
    from diffusionkit_amd import ops

    def launch(v):
        with tuned(**(knobs or {})):
            return ops.conv3x3(v["x"], v["w"], v["b"], upsample=form == "up", res=v.get("res") if res else None, downsample=form == "s2",
                               workspace=v.get("ws"))
    return launch


# (id, dtype, conv_v4 knob, (B, H, W, C, O) with H x W the INPUT size, upsample, table, residual, shortcut columns)
HALO_FORMS = [("halo_table", BF, 0, (2, 16, 16, 64, 128), False, True, False, 0), ("halo_plain_res", BF, 0, (2, 16, 16, 64, 128), False, False, True, 0),
              ("halo_table_shortcut", BF, 0, (2, 16, 16, 64, 128), False, True, False, 64), ("halo_upsample", BF, 0, (2, 8, 8, 64, 128), True, False, False, 0),
              ("f16_halo_table_res", F16, 0, (2, 16, 16, 64, 128), False, True, True, 0),
              ("v4_256_table_res", BF, 2, (2, 32, 48, 128, 256), False, True, True, 0), ("v4_128_table", BF, 2, (2, 32, 48, 128, 128), False, True, False, 0),
              ("v4_upsample", BF, 2, (2, 16, 24, 128, 256), True, False, False, 0)]


def conv_gn(v4, O, C2, G, stats, ups, tab=None):
    """norm -> silu -> conv in one launch; the GroupNorm table is ``tab`` or the operand "tab" of ``v``"""
    from diffusionkit_amd import ops

    def launch(v):
        wk = v["w"].reshape(O, -1)
        if C2:
            wk = torch.cat([wk, v["ws_w"] if "ws_w" in v else v["ws"]], dim=1)
        with tuned(conv_v4=v4):
            y = ops.conv3x3_gn(v["x"], wk, v["b"], gn_table=v.get("tab", tab), silu=True, res=v.get("res"), x2=v.get("x2"), bias2=v.get("bs"),
                               stats_groups=G if stats else 0, upsample=ups)
        return dict(y=y[0], part=y[1]) if stats else y
    return launch


def image_tail(tab=None):
    from diffusionkit_amd import ops

    def launch(v):
        img, u8, raw = ops.conv3x3_gn(v["x"], v["w"].reshape(3, -1), v["b"], gn_table=v.get("tab", tab), image=True)
        return dict(img=img, u8=u8, raw=raw)
    return launch


# ---- patchify + step ----------------------------------------------------------------------------------------------------------------------
def patchify_step(flux, step, p=2):
    from diffusionkit_amd import _lib, ops
    from diffusionkit_amd.engine import _stream
    sigma, sigma_next, w = step

    def launch(v):
        n_img, Hl, Wl, C = v["x"].shape
        _lib.check(_lib.load().dk_latent_to_tokens(v["x"].data_ptr(), v["tok0"].data_ptr(), n_img, 2, Hl, Wl, C, p, int(flux), _stream()))
        ops.euler_cfg_step(v["x"], v["out"], v["tok"], n_img, True, p, int(flux), sigma, sigma_next, w)
        return dict(tok0=v["tok0"], x=v["x"], tok=v["tok"])
    return launch


# ---- the catalogue of the address tests ---------------------------------------------------------------------------------------------------
class Spec:
    """one launch form.  ``ops``: name -> CPU tensor (fp32 values representable in ``dt``, uploaded as ``dt`` unless ``dtypes`` names another type; integer
    tensors as they are); ``outs``: name -> (shape, dtype) of the outputs the caller owns (filled with the sentinel before every launch); ``ws``:
    (name, bytes) of the zeroed workspace the launch takes, or None; ``launch(v)``; ``ref(ops in fp64)`` -> what ``pick(launch's result)`` must be
    within ``gate`` = (rel_l2 bound -- or "exact": equal element for element --, max_abs bound or None, the parity test the numbers are from),
    ``differ``: the largest share of elements that may differ at all, where that test bounds it; ``plan(v)``: the planner's answer as a tuple, or
    None; ``main_in`` / ``main_out``: the operands that also go across the odd multiple of 2^31 (``main_out`` None: the output is allocated by the
    wrapper -- every allocation of the wrapper is placed in turn)"""

    def __init__(self, ops, launch, ref, gate, dt=BF, dtypes=None, outs=None, ws=None, plan=None, main_in=None, main_out=None, pick=None,
                 modules=("ops",), differ=None):
        self.ops, self.launch, self.ref, self.gate, self.dt, self.dtypes = ops, launch, ref, gate, dt, dict(dtypes or {})
        self.outs, self.ws, self.plan, self.main_in, self.main_out = dict(outs or {}), ws, plan, main_in or next(iter(ops)), main_out
        self.pick, self.modules, self.differ = pick or (lambda y: y), modules, differ

    def kind(self, name):
        t = self.ops[name]
        if not t.is_floating_point():
            return t.dtype
        return self.dtypes.get(name, torch.float32 if name in ("tab", "rope") else self.dt)


SPECS = {}


def spec(name):
    def deco(fn):
        SPECS[name] = fn
        return fn
    return deco


def _plan_tuple(p):
    return tuple(getattr(p, f) for f, _ in p._fields_)


GATE_GEMM = (TOL_SINGLE_OP, None, "test_gpu_ops.py::test_gemm_v3_ragged_and_straddling_segments")
GATE_GEMM_F16 = (TOL_F16, None, "test_gpu_f16_ops.py::test_gemm256v3_f16 (TOL_F16)")
GATE_ATTN = (6e-3, 0.03, "test_gpu_ops.py::test_attention_kernel_variants")
GATE_ATTN_F16 = (6e-3 / 8, 0.03, "test_gpu_f16_ops.py::test_attention_f16_ragged (TOL_ATTN_F16)")


def _mx_scale_bytes(rows, k):
    from diffusionkit_amd import ops
    return ops.mx_scale_bytes(rows, k)


def _gemm_ws_bytes():
    from diffusionkit_amd import _lib
    return int(_lib.load().dk_gemm_workspace_bytes())


def _attn_ws_bytes():
    from diffusionkit_amd import _lib
    return max(int(_lib.load().dk_attention_workspace_bytes()), 256)


def _gemm_joint_spec(form, epi, shape=fp.GEMM_JOINT_SHAPES[0]):
    name, dt, knobs = form
    B, S_t, S_i = shape

    def build():
        from diffusionkit_amd import ops
        o, ref, _ = fp.gemm_joint_family(B, S_t, S_i, epi, dt)

        def plan(v):
            with tuned(**knobs):
                return _plan_tuple(ops.gemm_plan(gemm_joint_desc(v, B, S_t, S_i, epi), dtype=dt))
        return Spec(o, gemm_joint(dt, knobs, B, S_t, S_i, epi), lambda q: ref(q)[:, :S_t], GATE_GEMM if dt == BF else GATE_GEMM_F16, dt=dt,
                    ws=("ws", _gemm_ws_bytes()), plan=plan, main_in="att", main_out="X", pick=lambda y: y[:, :S_t])
    return build


for _form in GEMM_FORMS:
    SPECS[f"gemm_{_form[0]}_gate_res"] = _gemm_joint_spec(_form, "gate_res")
SPECS["gemm_bf16_v4_bias_589"] = _gemm_joint_spec(GEMM_FORMS[3], "bias", fp.GEMM_JOINT_SHAPES[1])
SPECS["gemm_bf16_v3_mf7_bias_589"] = _gemm_joint_spec(GEMM_FORMS[2], "bias", fp.GEMM_JOINT_SHAPES[1])


@spec("gemm_k_split")
def _():
    o, ref, _ = fp.gemm_ksplit_family(BF)
    M, N = o["res"].shape
    return Spec(o, gemm_ksplit(1), ref, (TOL_SINGLE_OP, None, "test_gpu_ops.py::test_gemm_v3_remainder_split"), outs={"out": ((M, N), BF)},
                ws=("ws", _gemm_ws_bytes()), main_in="x", main_out="out")


def _fused_plan(call):
    from diffusionkit_amd import ops

    def plan(v):
        with tuned(**call.tune):
            return _plan_tuple(ops.gemm_fused_plan(*fused_args(call, v)))
    return plan


GATE_FUSED = (TOL_SINGLE_OP, None, "test_gpu_fused_ops.py (its gate(): TOL_SINGLE_OP)")


@spec("gemm_fused_pair")
def _():
    case = fp.chosen_fused_cases()["pair"]
    call, o, ref, _ = fp.pair_family(case)
    run = fused(call)

    def launch(v):
        run(v)
        return v["C"]
    return Spec(o, launch, ref, GATE_FUSED, plan=_fused_plan(call), main_in="A", main_out="C")


@spec("gemm_fused_qknorm_rope_tail")
def _():
    case = fp.chosen_fused_cases()["knorm"]
    call, o, ref, rows, _ = fp.knorm_family(case)
    run = fused(call)

    def launch(v):
        run(v)
        return v["C"][rows.to(v["C"].device)]
    return Spec(o, launch, lambda q: ref(q)[:, 2 * case["h"]:], (TOL_SINGLE_OP, None, "test_gpu_fused_ops.py::test_qknorm_rope_in_gemm_tail (v columns: TOL_SINGLE_OP)"),
                outs={"C": (call.buffers["C"], BF)}, plan=_fused_plan(call), main_in="A", main_out="C",
                pick=lambda y: y[:, 2 * case["h"]:], dtypes={k: torch.float32 for k, b in call.buffers.items() if b[0] == "f32"})


@spec("gemm_fused_column_split")
def _():
    case = fp.chosen_fused_cases()["split"]
    call, o, ref, rows, _ = fp.split_family(case)
    n1, n2, c0 = case["n1"], case["n2"], call.side["C2"][1]
    run = fused(call)

    def launch(v):
        run(v)
        r = rows.to(v["C"].device)
        return dict(C=v["C"][r, :n1], C2=v["C2"][r, c0:c0 + n2])
    return Spec(o, launch, ref, GATE_FUSED, outs={n: (call.buffers[n], BF) for n in ("C", "C2")}, plan=_fused_plan(call), main_in="A", main_out="C")


# fp8: the activation bytes and their scale side array are produced by quantize_mx8 once (on the device, in ordinary memory) and are operands here
ROWS8, K8 = 384, 384  # tests/test_gpu_fp8_ragged.py


def act8():
    x = fp.rounder(BF)(ROWS8, K8, seed=801)
    x[:, :K8 // 2] *= 4.0
    return x


@spec("quantize_mx8")
def _():
    from diffusionkit_amd import ops
    from oracle import fp8 as o8
    x = act8()

    def launch(v):
        q, s = ops.quantize_mx8(v["x"], out=v["q"], scales=v["scales"])
        return dict(q=q, scales=s)

    def ref(o):  # test_quantize_mx8_bit_exact: the bytes and the block scales of oracle.fp8.mx8_encode, bit for bit
        q_ref, e_ref = o8.mx8_encode(x)
        return dict(q=q_ref, e=e_ref)

    def pick(y):
        return dict(q=y["q"].cpu(), e=f8.array_to_scales(y["scales"].cpu(), ROWS8, K8))
    return Spec(dict(x=x), launch, ref, ("exact", None, "test_gpu_fp8.py::test_quantize_mx8_bit_exact"),
                outs={"q": ((ROWS8, K8), torch.uint8), "scales": (lambda: (ops.mx_scale_bytes(ROWS8, K8),), torch.uint8)}, main_in="x", main_out="q", pick=pick)


@spec("gemm_fp8_bias")
def _():
    from diffusionkit_amd import ops
    from diffusionkit_amd.weights import quantize_weight_e4m3
    N, M = 256, 376
    dev = torch.device("cuda", 0)
    a8, sa = ops.quantize_mx8(act8().to(dev, BF))
    qw, wsc = quantize_weight_e4m3(fp.rounder(BF)(N, K8, seed=802, scale=0.02).to(BF))
    bias = fp.rounder(BF)(N, seed=803, scale=0.5)
    o = dict(a8=a8.cpu(), sa=sa.cpu(), w8=qw.cpu(), wsc=wsc.cpu().float(), bias=bias)

    def launch(v):
        ops.gemm_fp8(v["a8"], v["sa"], v["w8"], v["wsc"], bias=v["bias"], M=M, k=K8, out=v["out"], workspace=v.get("ws"))
        return v["out"][:M]

    def ref(q):
        a = f8.mx8_decode(o["a8"], f8.array_to_scales(o["sa"], ROWS8, K8)).double()[:M]
        w = o["w8"].view(torch.float8_e4m3fn).to(torch.float64) * o["wsc"].double().reshape(N, -1)[:, :1]
        return a @ w.t() + q["bias"]
    return Spec(o, launch, ref, (TOL_SINGLE_OP, None, "test_gpu_fp8.py::test_gemm_fp8_bias"), dtypes={"wsc": torch.float32},
                outs={"out": ((ROWS8, N), BF)}, ws=("ws", _gemm_ws_bytes()), main_in="a8", main_out="out")


def _attention_spec(form):
    name, dt, knobs, (B, H, S, D), QB = form

    def build():
        from diffusionkit_amd import ops
        o, ref, _ = fp.attention_family(B, H, S, D, QB, dt)

        def plan(v):
            with tuned(**knobs):
                return _plan_tuple(ops.attention_plan(dtype=dt, workspace_bytes=_attn_ws_bytes(), **attention_desc(v, B, H, S, D)))
        return Spec(o, attention(dt, knobs, B, H, S, D), ref, GATE_ATTN if dt == BF else GATE_ATTN_F16, dt=dt, outs={"out": ((B, S, H * D), dt)},
                    ws=("attn_ws", _attn_ws_bytes()) if "attn_split" in knobs else None, plan=plan, main_in="qkv", main_out="out")
    return build


for _form in ATTN_FORMS:
    SPECS[f"attention_{_form[0]}"] = _attention_spec(_form)


@spec("attention_q_load_norm_rope")
def _():
    c = fp.chosen_fused_cases()["attn_q"]
    B, H, S, D = c["B"], c["H"], c["S"], c["D"]
    o, tab, ref = fp.attention_q_family(c)
    o = dict(o, **({"rope": tab} if tab is not None else {}))
    knobs = dict(attn=c["mode"], attn_split=c.get("attn_split", -1))
    return Spec(o, attention(BF, knobs, B, H, S, D, attention_q_extra(c)), ref, (6e-3, 0.03, "test_gpu_fused_ops.py::test_query_norm_rope_in_attention_q_load"),
                outs={"out": ((B, S, H * D), BF)}, main_in="qkv", main_out="out")


def _untracked_inputs(B, H, S, D=128):
    """tests/test_gpu_attention_untracked.py: q, k scaled by sqrt(2), v by 1 / 4; the bound handed over is the measured one"""
    rnd = fp.rounder(BF)
    h = H * D
    qkv = rnd(B, S, 3 * h, seed=33)
    qkv[..., :2 * h] = (qkv[..., :2 * h] * math.sqrt(2.0)).to(BF).float()
    qkv[..., 2 * h:] = (qkv[..., 2 * h:] * 0.25).to(BF).float()
    q, k, _ = fp.split_heads(qkv, H, D)
    bound = float((q.double() @ k.double().transpose(-1, -2)).abs().max()) / math.sqrt(D) * 1.02
    rope = torch.zeros(S, D // 2, 2)
    rope[..., 0] = 1.0
    return qkv, rope, bound


@spec("attention_wave_untracked_768")
def _():
    from diffusionkit_amd import ops
    B, H, S, D = 1, 2, 768, 128
    qkv, rope, bound = _untracked_inputs(B, H, S)
    knobs = dict(attn=10, attn_track=0)
    extra = lambda v: dict(q_rope=v["rope"], score_bound=bound)

    def plan(v):
        with tuned(**knobs):
            p = ops.attention_plan(workspace_bytes=_attn_ws_bytes(), **attention_desc(v, B, H, S, D, **extra(v)))
        assert p.kernel == 10 and p.untracked == 1, "the launch was meant to take attention5.hip's untracked body"
        return _plan_tuple(p)
    return Spec(dict(qkv=qkv, rope=rope), attention(BF, knobs, B, H, S, D, extra), lambda o: fp.ref_attention(o["qkv"], H, D),
                (6e-3, 0.03, "test_gpu_attention_untracked.py::test_untracked_body_against_the_oracle_and_the_tracked_body"),
                outs={"out": ((B, S, H * D), BF)}, plan=plan, main_in="qkv", main_out="out")


def _attention_bias_spec(B, H, S, D, per_head):
    def build():
        from diffusionkit_amd.text import attention_bias
        o, ref, scale, _ = fp.attention_bias_family(B, H, S, D, per_head)

        def launch(v):
            return attention_bias(v["qkv"], H, D, scale, v["bias"] if per_head else v["bias"][0], per_head)
        return Spec(o, launch, ref, (6e-3, 0.03, "test_gpu_text.py::test_attention_with_score_bias"), main_in="qkv", modules=("text",))
    return build


SPECS["attention_score_bias_per_head"] = _attention_bias_spec(1, 4, 150, 64, True)
SPECS["attention_score_bias_shared"] = _attention_bias_spec(2, 2, 77, 64, False)


@spec("attention_mx8_copy")
def _():
    c = fp.chosen_fused_cases()["attn_o8"]
    B, H, S, D = c["B"], c["H"], c["S"], c["D"]
    h, M = H * D, B * S
    QB = 256 if (c["mode"] in (9, 10) and D == 128) else 128
    o, ref, _ = fp.attention_family(B, H, S, D, QB, BF)
    run = attention_mx8(c)

    def launch(v):
        run(v)
        return dict(out=v["out"], o8=v["o8"], o8_scales=v["o8_scales"])
    return Spec(o, launch, ref, GATE_ATTN, outs={"out": ((B, S, h), BF), "o8": ((M, h), torch.uint8), "o8_scales": (lambda: (_mx_scale_bytes(M, h),), torch.uint8)},
                main_in="qkv", main_out="o8", pick=lambda y: y["out"])


def _identity_spec(dt):
    def build():
        from diffusionkit_amd import ops
        B, H, S, D, F = 2, 2, 200, 64, 77
        o = dict(qkv=fp.rounder(dt)(B, S, 3 * H * D, seed=140))

        def ref(q):
            from tests._pag import ref_identity_attention
            return ref_identity_attention(q["qkv"], H, D, F)
        return Spec(o, lambda v: ops.attention_identity(v["qkv"], H, D, F), ref,
                    (TOL_SINGLE_OP if dt == BF else TOL_F16, 0.03, "test_gpu_pag.py's operator gate: TOL_SINGLE_OP / TOL_F16, test_attention's max_abs"),
                    dt=dt, main_in="qkv")
    return build


SPECS["attention_identity_bf16"] = _identity_spec(BF)
SPECS["attention_identity_f16"] = _identity_spec(F16)


def _d512_spec(dt):
    def build():
        from diffusionkit_amd import ops
        o, ref, _ = fp.attention_d512_family(2, 100, dt)
        return Spec(o, lambda v: ops.attention_d512(v["q"], v["k"], v["v"]), ref,
                    (6e-3, 0.03, "test_gpu_ops.py::test_attention_d512_flash") if dt == BF else
                    (6e-3 / 8, 0.03, "test_gpu_vae_f16.py: attention_d512 (TOL_ATTN_F16)"), dt=dt, main_in="q")
    return build


SPECS["attention_d512_bf16"] = _d512_spec(BF)
SPECS["attention_d512_f16"] = _d512_spec(F16)


# ---- row kernels
def _ref_ln(x, shift, scale, dt, eps=1e-6):
    """test_ln_modulate's / test_ln_modulate_f16's reference: the operator rounds (1 + scale) to the element type before it multiplies"""
    from oracle import mmdit as om
    return om.layer_norm(x, eps) * (1.0 + scale[:, None]).to(dt).to(x.dtype) + shift[:, None]


def _ln_spec(dt, h, form):
    def build():
        from diffusionkit_amd import ops
        B, S = 2, 77
        o, _, _ = fp.ln_modulate_family(B, S, h, dt)
        rnd = fp.rounder(dt)
        gate = (2e-3, None, "test_gpu_ops.py::test_ln_modulate") if dt == BF else (TOL_F16, None, "test_gpu_f16_ops.py::test_ln_modulate_f16 (TOL_F16)")

        def ref(q):
            return _ref_ln(q["x"], q["shift"], q["scale"], dt)
        if form == "plain":
            return Spec(o, lambda v: ops.ln_modulate(v["x"], v["shift"], v["scale"]), ref, gate, dt=dt, main_in="x")
        if form == "dual":  # two modulated outputs of one pass: the four [B, h] rows are views of ONE table [B, 4 h]
            o = dict(x=o["x"], mod=rnd(B, 4 * h, seed=45, scale=0.5))

            def launch(v):
                m = v["mod"]
                a, b = ops.ln_modulate_dual(v["x"], m[:, :h], m[:, h:2 * h], m[:, 2 * h:3 * h], m[:, 3 * h:])
                return dict(a=a, b=b)

            def ref2(q):
                m = q["mod"]
                return dict(a=_ref_ln(q["x"], m[:, :h], m[:, h:2 * h], dt), b=_ref_ln(q["x"], m[:, 2 * h:3 * h], m[:, 3 * h:], dt))
            return Spec(o, launch, ref2, gate, dt=dt, main_in="x")
        if form == "add":  # x <- round(x + s * tap) in place, then the modulated LayerNorm of the new rows
            s = 0.5
            o = dict(o, tap=rnd(B, S, h, seed=46))

            def launch(v):
                x, out = ops.ln_modulate_add(v["x"], v["tap"], s, v["shift"], v["scale"])
                return dict(x=x, out=out)

            def ref3(q):
                xn = (q["x"] + s * q["tap"]).to(dt).to(q["x"].dtype)
                return dict(x=xn, out=_ref_ln(xn, q["shift"], q["scale"], dt))
            return Spec(o, launch, ref3, gate, dt=dt, main_in="x", main_out="x")
        assert form == "mx8" and dt == BF
        o2 = dict(x=o["x"].reshape(B * S, h), shift=o["shift"][:1], scale=o["scale"][:1])

        def launch(v):
            q, sc = ops.ln_modulate_mx8(v["x"], v["shift"], v["scale"])
            return dict(q=q, scales=sc)

        def pick(y):
            return f8.mx8_decode(y["q"].cpu(), f8.array_to_scales(y["scales"].cpu(), B * S, h)).double()
        def ref_mx8(q):  # test_ln_modulate_mx8: the oracle's modulated LayerNorm in bf16, then the oracle's MX-fp8 rounding of it
            from oracle import fp8 as o8
            from oracle.mmdit import Prec, affine_transform
            y = affine_transform(q["x"].float()[None], q["shift"].float()[None], q["scale"].float()[None], 1e-6, Prec(BF))[0]
            return o8.mx8_fake_quant(y)
        return Spec(o2, launch, ref_mx8, (4e-3, None, "test_gpu_fp8.py::test_ln_modulate_mx8 (and fewer than 2 % of the elements differ)"), main_in="x",
                    pick=pick, differ=0.02)
    return build


for _dt, _n in ((BF, "bf16"), (F16, "f16")):
    SPECS[f"ln_modulate_{_n}_2432"] = _ln_spec(_dt, 2432, "plain")
    SPECS[f"ln_modulate_dual_{_n}_1536"] = _ln_spec(_dt, 1536, "dual")
    SPECS[f"ln_modulate_add_{_n}_1536"] = _ln_spec(_dt, 1536, "add")
SPECS["ln_modulate_mx8_1536"] = _ln_spec(BF, 1536, "mx8")


def _qk_spec(dt, D):
    def build():
        from diffusionkit_amd import ops
        o, ref, _ = fp.qk_norm_rope_family(D, dt)
        return Spec(o, lambda v: ops.qk_norm_rope_(v["qkv"], 3, D, v["qw"], v["kw"], v["tab"]), ref,
                    (2e-3, None, "test_gpu_ops.py::test_qk_norm_rope") if dt == BF else (TOL_F16, None, "test_gpu_f16_ops.py::test_qk_norm_rope_f16 (TOL_F16)"),
                    dt=dt, main_in="qkv", main_out="qkv")
    return build


SPECS["qk_norm_rope_bf16_d128"], SPECS["qk_norm_rope_bf16_d64"], SPECS["qk_norm_rope_f16_d64"] = _qk_spec(BF, 128), _qk_spec(BF, 64), _qk_spec(F16, 64)


def _gn_spec(dt, table):
    def build():
        from diffusionkit_amd import ops
        G = fp.GN_SHAPE[4]
        o, ref, _ = fp.groupnorm_family(dt, table=table)
        gate = (3e-3, None, "test_gpu_ops.py::test_groupnorm") if dt == BF else (TOL_F16, None, "test_gpu_vae_f16.py::test_groupnorm_f16 (TOL_F16)")
        if table:
            return Spec(o, lambda v: ops.groupnorm_table(v["x"], v["gamma"], v["beta"], G, 1e-5), ref, gate, dt=dt, main_in="x")
        return Spec(o, lambda v: ops.groupnorm(v["x"], v["gamma"], v["beta"], G, 1e-5, True), ref, gate, dt=dt, main_in="x")
    return build


for _dt, _n in ((BF, "bf16"), (F16, "f16")):
    SPECS[f"groupnorm_{_n}"], SPECS[f"groupnorm_table_{_n}"] = _gn_spec(_dt, False), _gn_spec(_dt, True)


def _softmax_spec(dt, what):
    def build():
        from diffusionkit_amd import ops
        o, ref, _ = (fp.softmax_family if what == "softmax" else fp.transpose_family)(dt)
        fn = ops.softmax_rows_ if what == "softmax" else ops.transpose
        return Spec(o, lambda v: fn(v["x"]), ref, (TOL_SINGLE_OP if dt == BF else TOL_F16, None, "test_gpu_ops.py::test_softmax_and_transpose"), dt=dt,
                    main_in="x", main_out="x" if what == "softmax" else None)
    return build


for _dt, _n in ((BF, "bf16"), (F16, "f16")):
    SPECS[f"softmax_rows_{_n}"], SPECS[f"transpose_{_n}"] = _softmax_spec(_dt, "softmax"), _softmax_spec(_dt, "transpose")


def _patchify_spec(flux):
    def build():
        o, ref, step, _ = fp.patchify_family(flux)
        shape = tuple(o["out"].shape)
        sigma, sigma_next, _ = step

        def ref_x(q):
            """test_patchify_and_euler_step's restatement: the denoised image is formed from the bf16-rounded latent (what the model saw), the step
            from the fp32 one.  The family's reference uses one latent in both places and is linear in it: with xb = bf16(x) the difference is
            (x - xb) * (1 + (sigma_next - sigma) / sigma).  (fp32: the family's gather works on fp32 index tensors.)"""
            x = q["x"].float()
            xb = x.to(BF).float()
            return ref(dict(x=xb, out=q["out"].float()))["x"].double() + (x - xb).double() * (1.0 + (sigma_next - sigma) / sigma)
        return Spec(o, patchify_step(flux, step), ref_x, (None, 1e-5, "test_gpu_ops.py::test_patchify_and_euler_step (max_abs of the latent)"),
                    dtypes={"x": torch.float32}, outs={"tok0": (shape, BF), "tok": (shape, BF)}, main_in="x", main_out="tok", pick=lambda y: y["x"])
    return build


SPECS["patchify_step_flux"], SPECS["patchify_step_sd3"] = _patchify_spec(True), _patchify_spec(False)


# ---- convolutions
GATE_CONV = (TOL_SINGLE_OP, None, "test_gpu_ops.py::test_conv3x3")


def _conv_spec(dt, form, res, shape=(2, 16, 16, 64, 128), knobs=None, tile=16, ws=False, gate=GATE_CONV):
    def build():
        o, ref, _ = fp.conv_family(*shape, form, dt, res=res, tile=tile)
        g = gate if dt == BF else (TOL_F16, None, "test_gpu_f16_ops.py (TOL_F16)")
        return Spec(o, conv(form, res, knobs), ref, g, dt=dt, main_in="x", ws=("ws", _gemm_ws_bytes()) if ws else None)
    return build


for _dt, _n in ((BF, "bf16"), (F16, "f16")):
    for _f, _r in (("plain", False), ("plain", True), ("s2", False), ("up", False)):
        SPECS[f"conv3x3_128_{_n}_{_f}{'_res' if _r else ''}"] = _conv_spec(_dt, _f, _r)
_V3 = dict(gemm=9, gemm_mf=8)
_GATE_V3 = (TOL_SINGLE_OP, None, "test_gpu_ops.py::test_conv3x3_on_256_tile_kernel")
SPECS["conv3x3_v3_plain_res"] = _conv_spec(BF, "plain", True, (2, 16, 24, 128, 256), _V3, 8, gate=_GATE_V3)
SPECS["conv3x3_v3_up"] = _conv_spec(BF, "up", False, (2, 8, 12, 128, 256), _V3, 8, gate=_GATE_V3)
SPECS["conv3x3_v3_k_split_workspace"] = _conv_spec(BF, "plain", False, (2, 16, 16, 512, 256), _V3, 8, ws=True, gate=_GATE_V3)


def _rnd(t, dt):
    return t.to(dt).to(t.dtype)


def _conv_gn_spec(form):
    name, dt, v4, (B, H, W, C, O), ups, table, res, C2 = form

    def build():
        G = 32
        rnd = fp.rounder(dt)
        gamma, beta = rnd(C, seed=81, scale=0.1, shift=1.0), rnd(C, seed=82, scale=0.1)
        kind = "up" if ups else "plain"
        x_clean = fp.conv_family(B, H, W, C, O, kind, dt)[0]["x"]
        o, _, _ = fp.conv_family(B, H, W, C, O, kind, dt, res=res, C2=C2)
        if C2:
            o["ws_w"] = o.pop("ws")  # ("ws" names the workspace in a launch's ``v``)
        stats = not ups
        if table:  # the table the device builds is an fp32 operand of the conv launch; the reference restates it in fp64
            o["tab"] = fp.ref_groupnorm_table(x_clean, gamma, beta, G)

        def ref(q):
            act = None
            if table:
                t = q["tab"]

                def act(x):  # (the launch rounds the normalised value and the activation to the element type: conv_halo.hip's round_act / pack2,
                    y = _rnd(x * t[:, 0][:, None, None] + t[:, 1][:, None, None], dt)  # the oracle's Prec(BF) in test_conv3x3_gn_halo)
                    return _rnd(y * torch.sigmoid(y), dt)
            return fp.ref_conv(q["x"], q["w"], q["b"], kind, q.get("res"), act, q.get("x2"), q.get("ws_w"), q.get("bs"))
        tests = "test_gpu_ops.py::test_conv256v4_equals_conv_halo" if v4 else "test_gpu_ops.py::test_conv3x3_gn_halo"
        return Spec(o, conv_gn(v4, O, C2, G, stats, ups), ref, (TOL_SINGLE_OP if dt == BF else TOL_F16, None, tests), dt=dt, main_in="x",
                    pick=(lambda y: y["y"]) if stats else None)
    return build


for _form in HALO_FORMS:
    SPECS[f"conv3x3_gn_{_form[0]}"] = _conv_gn_spec(_form)


@spec("conv_out_image_tail")
def _():
    B, H, W, C, G = 2, 32, 48, 128, 32
    rnd = fp.rounder(BF)
    gamma, beta = rnd(C, seed=92, scale=0.1, shift=1.0), rnd(C, seed=93, scale=0.1)
    o, _, _ = fp.conv_family(B, H, W, C, 3, "plain", BF)
    o["tab"] = fp.ref_groupnorm_table(o["x"], gamma, beta, G)

    def ref(q):
        t = q["tab"]
        y = _rnd(q["x"] * t[:, 0][:, None, None] + t[:, 1][:, None, None], BF)
        return fp.ref_conv(_rnd(y * torch.sigmoid(y), BF), q["w"], q["b"])
    return Spec(o, image_tail(), ref, (TOL_SINGLE_OP, None, "test_gpu_ops.py::test_conv_out_image_tail_halo"), main_in="x", pick=lambda y: y["raw"][..., :3])


# ---- text ops (diffusionkit_amd/text.py's device helpers at the shapes of tests/test_gpu_text_ops.py's smallest cases)
def _text_spec(what):
    def build():
        from diffusionkit_amd import text
        rnd = fp.rounder(BF)
        n, dim = 77, 768
        gate = (TOL_SINGLE_OP, None, "tests/_util.py: TOL_SINGLE_OP (one rounding of an fp32 result, test_gpu_text_ops.py)")
        if what == "embedding":
            o = dict(table=rnd(1000, dim, seed=150), ids=torch.randint(0, 1000, (n,), generator=torch.Generator().manual_seed(151), dtype=torch.int32),
                     pos=rnd(n, dim, seed=152))
            return Spec(o, lambda v: text._embedding(v["table"], v["ids"], v["pos"])[0], lambda q: q["table"][q["ids"].long()] + q["pos"], gate,
                        main_in="table", modules=("text",))
        x = rnd(n, dim, seed=153, scale=2.0, shift=0.3)
        w, b = rnd(dim, seed=154, scale=0.1, shift=1.0), rnd(dim, seed=155, scale=0.1)
        if what == "layernorm":
            def ref(q):
                mu = q["x"].mean(-1, keepdim=True)
                var = ((q["x"] - mu) ** 2).mean(-1, keepdim=True)
                return (q["x"] - mu) * torch.rsqrt(var + 1e-5) * q["w"] + q["b"]
            return Spec(dict(x=x, w=w, b=b), lambda v: text._layernorm(v["x"], v["w"], v["b"]), ref, gate, main_in="x", modules=("text",))
        if what == "t5_rmsnorm":
            return Spec(dict(x=x, w=w), lambda v: text._t5_rmsnorm(v["x"], v["w"], 1e-6),  # (the T5 stream is fp32)
                        lambda q: q["x"] * torch.rsqrt((q["x"] ** 2).mean(-1, keepdim=True) + 1e-6) * q["w"], gate, main_in="x", modules=("text",),
                        dtypes={"x": torch.float32})
        assert what == "product"
        return Spec(dict(a=x, b=rnd(n, dim, seed=156)), lambda v: text._elementwise(1, v["a"], v["b"]), lambda q: q["a"] * q["b"], gate, main_in="a",
                    modules=("text",))
    return build


for _w in ("embedding", "layernorm", "t5_rmsnorm", "product"):
    SPECS[f"text_{_w}"] = _text_spec(_w)
