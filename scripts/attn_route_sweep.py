#!/usr/bin/env python3
"""dk_attention_route under the host sanitizers, on the CPU (no GPU is touched; never run this through a GPU job).

    python scripts/attn_route_sweep.py [output file]

Builds scripts/attn_route_sweep.hip together with csrc/attention.hip -- host code with -fsanitize=address,undefined -- into a program of its own,
linked against the built libdk_hip.so for what attention.hip calls (the kernels' launchers, dk_attention5_eligible, the error string), runs it,
and compares every line it prints for 256 compute units with what dk_attention_plan answers for the same input.  Exit status 1 on a sanitizer
report or a line that differs."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = os.path.join(ROOT, "diffusionkit_amd")


def main(out_path=None):
    from diffusionkit_amd import _lib, ops
    lib = _lib.load()
    with tempfile.TemporaryDirectory() as t:
        exe = os.path.join(t, "attn_route_sweep")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                               "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "scripts", "attn_route_sweep.hip"),
                               os.path.join(PKG, "csrc", "attention.hip"), "-L" + PKG, "-ldk_hip", "-Wl,-rpath," + PKG, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True)
    if out_path:
        open(out_path, "w").write(r.stdout)
    if r.returncode != 0 or r.stderr.strip():
        print(r.stderr)
        print(f"sanitizer report or failure (exit status {r.returncode})")
        return 1
    lines, compared, bad = r.stdout.splitlines(), 0, 0
    for ln in lines:
        left, right = ln.split(" -> ")
        a = {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", left)}
        if a["n_cu"] != 256:  # (dk_attention_plan takes the CU count from the device: 256 without one)
            continue
        h = a["H"] * a["D"]
        d = dict(q=0x10000000, k=0x10000000 + 2 * h, v=0x10000000 + 4 * h, out=0x20000000, B=a["B"], H=a["H"], S=a["S"], D=a["D"], ld=3 * h, ldo=h, scale=1.0)
        if a["bias"]:
            ldb = (a["S"] + 63) // 64 * 64
            d.update(bias=0x30000000, ldb=ldb, bias_head_stride=ldb * a["S"])
        if a["qn"]:
            d.update(qn_a=0x40000000, qn_b=0x40000000)
        if a["o8"]:
            d.update(O8=0x50000000, O8_scales=0x60000000, o8_ld=h, o8_rows=a["B"] * a["S"])
        lib.dk_tune_set(b"attn", a["attn"])
        lib.dk_tune_set(b"attn_split", a["attn_split"])
        try:
            p = ops.attention_plan(dtype=ops.F16 if a["dtype"] else ops.BF, workspace_bytes=a["ws"], o8_split=a["o8_split"], **d)
            got = " ".join(f"{f}={getattr(p, f)}" for f in ("kernel", "qfuse", "blocks", "whole", "split", "jobs", "quantize", "launches"))
        except _lib.DkHipError as e:
            got = "refused: " + str(e).split("): ", 1)[1]
        finally:
            lib.dk_tune_set(b"attn", -1)
            lib.dk_tune_set(b"attn_split", -1)
        compared += 1
        if got != right:
            bad += 1
            print(f"DIFFERENT: {left}\n  route: {right}\n  plan:  {got}")
    print(f"{len(lines)} routes, sanitizers clean; {compared} of them (256 compute units) compared with dk_attention_plan, {bad} different")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:2]))
