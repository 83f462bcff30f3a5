"""Guarded, poisoned, exact-size engine workspaces (plain torch; the helper itself needs no GPU).

The engines (dk_mmdit_*, dk_vae_decode, dk_vae_encode) carve every internal buffer out of ONE caller-supplied workspace, and the Python
wrappers keep that allocation when a later shape needs fewer bytes.  tests/_footprint.py poisons the *operands* of single launches; this
file does the same one layer up, to the workspace:

  * ``GuardedWorkspace``: one uint8 tensor = margin | interior | margin.  The interior is handed to an engine as its ``_ws`` at exactly the
    size the engine's own ``dk_*_workspace_bytes`` reports (the wrappers reuse a ``_ws`` whose numel() >= nbytes and pass numel() on, so
    the engine sees the size it declared, its own + 256 slack included).
  * whole-buffer fills: 0x00, and 0xFF -- a NaN in every element type the workspaces hold (bf16, fp16, fp32, e4m3) and the E8M0 NaN code
    of the MX scale arrays; "stale": no refill after a run at a larger shape in the same allocation.
  * ``check()``: everything outside the interior is byte for byte what it was when the run was armed; the first offending byte is
    reported as an offset relative to the interior (negative: in front of it; >= nbytes: behind it).

tests/_footprint.py's ``Guard`` counts written margin elements on a host copy of the WHOLE allocation; an engine workspace at production
width is half a gigabyte, so the comparison here runs on the device and over the margins only.  ``bits`` is shared with it.
"""
import torch

from tests._footprint import bits

MARGIN = 1 << 20  # bytes on each side of the largest interior; a multiple of 256 (the engines want a 256-byte-aligned workspace)
FILL_ZERO, FILL_NAN = 0x00, 0xFF
NAN_DTYPES = (torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fn)


class GuardedWorkspace:
    """``capacity`` bytes between two margins of ``margin`` bytes each.  ``interior(nbytes)`` is the view [margin, margin + nbytes) an
    engine gets; ``arm(nbytes)`` records everything outside it, ``check(nbytes, what)`` compares."""

    def __init__(self, capacity: int, device, margin: int = MARGIN):
        assert margin >= MARGIN and margin % 256 == 0, "margins: at least 1 MiB and a multiple of 256"
        self.capacity, self.margin = int(capacity), margin
        n = margin + self.capacity + margin
        self._alloc = torch.empty(n + 256, dtype=torch.uint8, device=device)  # (the host allocator promises 64-byte alignment only)
        skew = -self._alloc.data_ptr() % 256
        self.whole = self._alloc[skew:skew + n]
        assert self.whole.data_ptr() % 256 == 0
        self._armed = None

    def fill(self, byte: int) -> None:
        self.whole.fill_(byte)

    def interior(self, nbytes: int) -> torch.Tensor:
        assert 0 < nbytes <= self.capacity
        return self.whole[self.margin:self.margin + nbytes]

    def arm(self, nbytes: int) -> None:
        """remember the bytes in front of and behind the interior of ``nbytes`` (after a fill they are the fill; in a stale buffer the
        bytes behind it are whatever the larger run left)"""
        self._armed = (nbytes, self.whole[:self.margin].clone(), self.whole[self.margin + nbytes:].clone())

    def first_written(self, nbytes: int):
        """None, or the offset (relative to the interior) of the first byte outside it that changed since ``arm``"""
        n, lo, hi = self._armed
        assert n == nbytes, "check() of another interior than the armed one"
        d = self.whole[:self.margin] != lo
        if bool(d.any()):
            return int(torch.nonzero(d)[0]) - self.margin
        d = self.whole[self.margin + nbytes:] != hi
        if bool(d.any()):
            return nbytes + int(torch.nonzero(d)[0])
        return None

    def check(self, nbytes: int, what: str, fill=None) -> None:
        """``fill``: the byte the whole allocation was filled with before the run (None for a stale buffer): the margins must hold it"""
        off = self.first_written(nbytes)
        if off is None and fill is not None:
            assert self.margins_hold(fill, nbytes), f"{what}: the margins were not filled with {fill:#04x} when the run was armed"
        assert off is None, (f"{what}: a byte outside the declared workspace of {nbytes} bytes was written, first at offset {off} "
                             f"relative to the workspace ({'in front of it' if off < 0 else f'{off - nbytes} bytes behind its end'})")

    def margins_hold(self, byte: int, nbytes: int) -> bool:
        """both margins still hold the fill byte (what ``check`` proves after ``fill(byte); arm(nbytes)``)"""
        return bool((self.whole[:self.margin] == byte).all()) and bool((self.whole[self.margin + nbytes:] == byte).all())


def lend(eng, ws: GuardedWorkspace, nbytes: int) -> None:
    """hand the interior to an engine wrapper (MMDiTEngine / VAEDecoderEngine / VAEEncoderEngine) and arm the guard"""
    eng._ws = ws.interior(nbytes)
    assert eng._ws.numel() == nbytes and eng._ws.data_ptr() % 256 == 0
    ws.arm(nbytes)


def assert_identical(outs: dict, what: str) -> None:
    """``outs``: label -> tensor, or label -> tuple of tensors; every entry is finite and equal to the first one in its raw bit patterns"""
    labels = list(outs)
    as_tuple = lambda v: v if isinstance(v, (tuple, list)) else (v,)
    first = as_tuple(outs[labels[0]])
    for lab in labels:
        for i, t in enumerate(as_tuple(outs[lab])):
            if t.is_floating_point():
                bad = ~torch.isfinite(t.float())
                assert not bool(bad.any()), (f"{what}: output {i} of the '{lab}' run holds {int(bad.sum())} non-finite values, first at "
                                             f"{tuple(int(j) for j in torch.nonzero(bad)[0])}")
            ref = first[i]
            assert t.shape == ref.shape and t.dtype == ref.dtype, f"{what}: output {i} of '{lab}': {tuple(t.shape)} {t.dtype}"
            if not torch.equal(bits(t), bits(ref)):  # (the raw patterns: -0.0 is not 0.0)
                d = bits(t) != bits(ref)
                assert False, (f"{what}: output {i} of the '{lab}' run differs from the '{labels[0]}' run in {int(d.sum())} of {d.numel()} "
                               f"elements, first at {tuple(int(j) for j in torch.nonzero(d)[0])}")
