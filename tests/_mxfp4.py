"""Operands and oracle weights for the MX-fp4 (W4A8) tests: the product quantiser (diffusionkit_amd/weights.py) is the format's definition
and tests/test_fp4_host.py checks it against a float64 restatement; here it only builds what the GPU tests compare against."""
import torch

from diffusionkit_amd.weights import dequantize_weight_mxfp4, pack_mxfp4, quantize_weight_mxfp4
from oracle import fp8 as o8
from tests import _fp8 as f8
from tests._util import BF, bf16r, randn


def fake_quant_weight(w):
    """fp32 values of the MX-fp4 quantisation of a (bf16) weight"""
    return dequantize_weight_mxfp4(*quantize_weight_mxfp4(w.to(BF)))


def weight_operands(w, pitch=None):
    """bf16 weight -> (packed bytes, packed block scales, wscale, fp32 dequantised values)"""
    code, e8, ws = quantize_weight_mxfp4(w)
    w4, sw = pack_mxfp4(code, e8, pitch)
    return w4, sw, ws, dequantize_weight_mxfp4(code, e8, ws)


def fp4_problem(M, N, K, seed, w_pitch=None, w=None):
    """operands as tests/test_gpu_fp8.py::_fp8_problem builds them: activations with one half scaled by 4, weights at 0.02"""
    a = bf16r(randn(M, K, seed=seed, scale=1.0))
    a[:, :K // 2] *= 4.0
    if w is None:
        w = randn(N, K, seed=seed + 1, scale=0.02).to(BF)
    qa, ea = o8.mx8_encode(a)
    return (qa, ea) + weight_operands(w, w_pitch) + (f8.mx8_decode(qa, ea),)


def fake_quant_block_weights(cfg, named):
    """oracle/fp8.py: fake_quant_block_weights with the MX-fp4 quantiser: what pack_mmdit(weight_dtype="mxfp4") makes of the block Linears -- row-wise,
    so the fused [q|k|v](|fc1) matrices quantise like their parts; the single blocks' linear2 = [o_proj | fc2] is quantised as the concatenation"""
    out = {k: v.to(torch.float32) for k, v in named.items()}
    n_bf = min(int(cfg.fp8_bf16_double_blocks), cfg.depth_multimodal)
    parts = ("attn.q_proj", "attn.k_proj", "attn.v_proj", "attn.o_proj", "mlp.fc1", "mlp.fc2")
    for i in range(n_bf, cfg.depth_multimodal):
        for s in ("image_transformer_block", "text_transformer_block"):
            for n in parts:
                key = f"multimodal_transformer_blocks.{i}.{s}.{n}.weight"
                if key in named:
                    out[key] = fake_quant_weight(named[key])
    for i in range(cfg.depth_unified):
        p = f"unified_transformer_blocks.{i}.transformer_block"
        for n in ("attn.q_proj", "attn.k_proj", "attn.v_proj", "mlp.fc1"):
            out[f"{p}.{n}.weight"] = fake_quant_weight(named[f"{p}.{n}.weight"])
        o, f2 = named[p + ".attn.o_proj.weight"], named[p + ".mlp.fc2.weight"]
        both = fake_quant_weight(torch.cat([o.to(BF), f2.to(BF)], dim=1))
        out[p + ".attn.o_proj.weight"], out[p + ".mlp.fc2.weight"] = both[:, :o.shape[1]], both[:, o.shape[1]:]
    return out
