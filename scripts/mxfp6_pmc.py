"""The program of the counter run of profiles/mxfp6_activations.md: three launches each of the W4A8 and the W4A6 GEMM at FLUX's qkv shape at 1024^2
(4096 x 9216 x 3072).  Counters only, two passes, the program after `--`:
    rocprofv3 --pmc SQ_BUSY_CYCLES SQ_WAIT_INST_LDS SQ_WAIT_INST_ANY SQ_INSTS_LDS -d out/p1 --output-format csv -- python scripts/mxfp6_pmc.py
    rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_LDS_BANK_CONFLICT SQ_WAVE_CYCLES SQ_INSTS_VALU_MFMA_MOPS_F8 -d out/p2 --output-format csv -- python scripts/mxfp6_pmc.py
    python scripts/pmc_summary.py out gemm256f4 > profiles/mxfp6_pmc.log"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from diffusionkit_amd import ops
from diffusionkit_amd.weights import pack_mxfp4, quantize_weight_mxfp4
dev, BF = torch.device("cuda"), torch.bfloat16
M, N, K = 4096, 9216, 3072
x = torch.randn(M, K, device=dev, dtype=BF)
a8, s8 = ops.quantize_mx8(x)
a6, s6 = ops.quantize_rows_mx6(x)
code, e8, wsc = quantize_weight_mxfp4((torch.randn(N, K, device=dev) * 0.02).to(BF))
w4, sw = pack_mxfp4(code, e8)
out = torch.empty(M, N, device=dev, dtype=BF)
for i in range(3):
    ops.gemm_fp4(a8, s8, w4, sw, wsc, M=M, k=K, out=out)
    ops.gemm_fp4(a6, s6, w4, sw, wsc, M=M, k=K, out=out, activations="mxfp6")
torch.cuda.synchronize()
