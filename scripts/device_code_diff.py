#!/usr/bin/env python3
"""Is the gfx950 device code of two builds the same?  (CPU; for host-only changes.)

    python scripts/device_code_diff.py <build dir A> <build dir B>

For every *.o of either directory: unbundle the gfx950 code object (the commands of tests/test_codegen_guards.py::kernel_metadata) and compare
the bytes of its .text section and the output of `llvm-readelf --notes` (kernel names, register counts, LDS / scratch sizes, argument layouts).
The whole code object is not the criterion: a host-only edit of a file that also defines kernels moves a few bytes elsewhere in it.  Prints one
markdown table row per object; exit status 1 when any differs or exists on one side only."""
import glob
import hashlib
import os
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def device_code(obj):
    """(.text bytes, notes text) of the object's gfx950 code object; None for a host-only object."""
    with tempfile.TemporaryDirectory() as t:
        r = subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={t}/fb.bin", obj, f"{t}/copy.o"], capture_output=True)
        if r.returncode != 0:
            return None
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={t}/fb.bin",
                               f"--output={t}/k.co", "--unbundle"])
        notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", f"{t}/k.co"], text=True)
        r = subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.text", f"{t}/k.co", f"{t}/text.bin"], capture_output=True)
        text = open(f"{t}/text.bin", "rb").read() if r.returncode == 0 and os.path.exists(f"{t}/text.bin") else b""
    return text, notes.replace(f"{t}/k.co", "k.co")


def main(a, b):
    names = sorted({os.path.basename(p) for d in (a, b) for p in glob.glob(os.path.join(d, "*.o"))})
    print("| object | .text bytes | .text sha256 (A) | .text | notes |")
    print("|---|---|---|---|---|")
    bad = 0
    for n in names:
        pa, pb = os.path.join(a, n), os.path.join(b, n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"| {n} | | | only in {'A' if os.path.exists(pa) else 'B'} | |")
            bad += 1
            continue
        ca, cb = device_code(pa), device_code(pb)
        if ca is None or cb is None:
            same = ca is None and cb is None
            print(f"| {n} | | | {'host only' if same else 'device code on one side only'} | |")
            bad += not same
            continue
        t_ok, n_ok = ca[0] == cb[0], ca[1] == cb[1]
        print(f"| {n} | {len(ca[0])} | {hashlib.sha256(ca[0]).hexdigest()[:16]} | {'identical' if t_ok else 'DIFFERENT'} | {'identical' if n_ok else 'DIFFERENT'} |")
        bad += not (t_ok and n_ok)
    print(f"\n{len(names)} objects, {bad} with differences")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
