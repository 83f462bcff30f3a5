#!/usr/bin/env python3
"""Is the gfx950 device code of two builds the same?  (CPU; for host-only changes.)

    python scripts/device_code_diff.py <build dir A> <build dir B>

For every *.o of either directory: unbundle the gfx950 code object (the commands of tests/test_codegen_guards.py::kernel_metadata) and compare
the bytes of its .text section and the output of `llvm-readelf --notes` (kernel names, register counts, LDS / scratch sizes, argument layouts).
The whole code object is not the criterion: a host-only edit of a file that also defines kernels moves a few bytes elsewhere in it.  Prints one
markdown table row per object; exit status 1 when any differs or exists on one side only.

    python scripts/device_code_diff.py --kernels <build dir A> <build dir B>

For changes that ADD kernels to an object (A: the parent's build): the object's .text grows, so every function of A's code object is compared on
its own -- its disassembly (instructions and operands, without addresses) and its block of the notes (argument layout, register counts, LDS /
scratch) -- against the function of the same name in B.  One row per object with the functions of A that differ or are gone, and the names B adds;
exit status 1 when a function of A differs or is missing.

    python scripts/device_code_diff.py --kernels --rename OLD=NEW [--rename ...] <build dir A> <build dir B>

... where a kernel template gained a parameter: function OLD of A is compared with function NEW of B (mangled names; the name itself is
taken out of the notes before they are compared)."""
import glob
import hashlib
import os
import re
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


def kernel_code(obj):
    """{function name: (instructions, notes block)} of the object's gfx950 code object; None for a host-only object."""
    with tempfile.TemporaryDirectory() as t:
        r = subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={t}/fb.bin", obj, f"{t}/copy.o"], capture_output=True)
        if r.returncode != 0:
            return None
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={t}/fb.bin",
                               f"--output={t}/k.co", "--unbundle"])
        notes = subprocess.check_output([f"{LLVM}/llvm-readelf", "--notes", f"{t}/k.co"], text=True)
        dis = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", f"{t}/k.co"], text=True)
    blocks = {}
    for b in re.split(r"\n  - \.agpr_count", notes)[1:]:
        b = b.split("\namdhsa.target")[0]  # (the last kernel's block would carry the trailer of the notes)
        m = re.search(r"\.name:\s+(\S+)", b)
        if m:
            blocks[m.group(1)] = b
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line.strip())
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur is not None and line.strip() and line.strip() != "...":  # ("...": the disassembler's mark for the zero padding behind the last function)
            out[cur].append(re.sub(r"//.*$", "", line).strip())
    return {k: (v, blocks.get(k)) for k, v in out.items()}


def main_kernels(a, b, rename=None):
    rename = rename or {}
    names = sorted({os.path.basename(p) for p in glob.glob(os.path.join(a, "*.o"))})
    print("| object | functions in A | identical in B | different or missing in B | added by B |")
    print("|---|---|---|---|---|")
    bad = 0
    for n in names:
        pa, pb = os.path.join(a, n), os.path.join(b, n)
        ka = kernel_code(pa)
        kb = kernel_code(pb) if os.path.exists(pb) else None
        if ka is None:
            continue
        if kb is None:
            print(f"| {n} | {len(ka)} | 0 | no device code in B | |")
            bad += len(ka)
            continue
        def same(k):
            k2 = rename.get(k, k)
            if k2 not in kb:
                return False
            (ia, na), (ib, nb) = ka[k], kb[k2]
            return ia == ib and (na or "").replace(k, "@") == (nb or "").replace(k2, "@")
        diff = [k for k in ka if not same(k)]
        added = [k for k in kb if k not in ka and k not in rename.values()]
        print(f"| {n} | {len(ka)} | {len(ka) - len(diff)} | {', '.join(diff) or 'none'} | {len(added)} |")
        bad += len(diff)
    print(f"\n{len(names)} objects, {bad} functions of A with differences")
    return 1 if bad else 0


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
    if len(sys.argv) >= 4 and sys.argv[1] == "--kernels":
        args, ren = sys.argv[2:], {}
        while len(args) >= 2 and args[0] == "--rename":
            old, new = args[1].split("=", 1)
            ren[old] = new
            args = args[2:]
        if len(args) != 2:
            sys.exit(__doc__)
        sys.exit(main_kernels(args[0], args[1], ren))
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
