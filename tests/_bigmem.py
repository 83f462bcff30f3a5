"""A poisoned arena that holds operands across 4 GiB address multiples, and strided views whose extents pass 2^31 / 2^32 bytes.

Every hot kernel addresses memory through 32-bit quantities ("Address-range guards").  Two things the rest of the suite never does are
done here: an operand is put at an address where a multiple of 2^32 (or an odd multiple of 2^31) falls INSIDE it, so that an address sum that drops
its carry lands 4 GiB (2 GiB) lower; and a few rows are spread over an extent larger than 2^31 / 2^32 bytes, so that offsets with bit 31 or bit 32
set are really formed.  Both happen inside one allocation filled with the footprint tests' NaN (tests/_footprint.py: NAN, as bfloat16 -- the same
two bytes read as float16 and, in pairs, as float32 are a NaN too), so a stray read returns NaN and a stray write shows up in ``assert_poison``:
a defect becomes a failed assertion, not a fault.

The arithmetic (``boundaries``, ``place_offset``, ``span_elems``) is plain Python and is swept on the CPU by tests/test_address_range_cpu.py."""
import torch

from tests import _footprint as fp

ARENA_BYTES = 2 ** 33 + 2 ** 29
MARGIN = 2 ** 28  # the boundaries lie at least this far from either end of the arena
ALIGN = 512       # torch's caching allocator hands out 512-byte aligned blocks: a placed view starts at such an address too


def boundaries(base: int, size: int = ARENA_BYTES, margin: int = MARGIN):
    """(b32, b31) for an allocation [base, base + size): the UPPER of the multiples of 2^32 that lie at least ``margin`` bytes from either end (an
    address that lost its carry lands at b32 - 2^32 + ..., still inside the allocation), and the upper odd multiple of 2^31 with the same margins"""
    lo, hi = base + margin, base + size - margin
    b32 = hi // 2 ** 32 * 2 ** 32
    k = hi // 2 ** 31
    b31 = (k if k % 2 else k - 1) * 2 ** 31
    assert lo <= b32 - 2 ** 32 and lo <= b31 - 2 ** 31, "the allocation is too small to hold two multiples of 2^32 inside its margins"
    return b32, b31


def span_elems(shape, stride) -> int:
    """elements between the first and one past the last element of a strided view"""
    if any(s == 0 for s in shape):
        return 0
    return 1 + sum((s - 1) * st for s, st in zip(shape, stride))


def row_sizes(shape, stride, itemsize):
    """byte sizes of a 'row' of the view, innermost first: the pitch of each dimension but the last one"""
    return [stride[i] * itemsize for i in range(len(shape) - 2, -1, -1) if shape[i] > 1 and stride[i] > 0]


def place_offset(nbytes: int, rows, at: float, itemsize: int, align: int = ALIGN):
    """(off, align): the boundary falls ``off`` bytes behind the start of an operand of ``nbytes`` bytes.  0 < off < nbytes (strictly inside), off is a
    multiple of ``align`` (the boundary is a multiple of 2^31, so the start keeps that alignment), off is no multiple of the row size (the boundary
    falls in the middle of a row, never on a row or tile edge), and off is the nearest such offset at or behind ``at * nbytes`` (in front of it
    where none lies behind).  ``rows``: candidate row sizes, innermost first -- where the innermost row divides ``align`` (a 64-channel pixel of
    128 bytes) every aligned offset is an edge of it, and the next outer row (the image row) is used.  Only an operand too small to hold such an
    offset at 512 bytes gets a smaller alignment (halved down to the element size); an operand of one element cannot be placed."""
    assert nbytes > itemsize, "an operand of one element has no inside"
    while align >= itemsize:
        for rb in list(rows) + [0]:  # (0: no row structure -- a vector, or a single row)
            if rb and (align % rb == 0 or rb >= nbytes):
                continue
            n = (nbytes - 1) // align  # candidates align * 1 .. align * n
            k0 = min(max(-(-int(at * nbytes) // align), 1), max(n, 1))
            for d in range(0, 2 * (n + 1)):
                k = k0 + (d + 1) // 2 * (1 if d % 2 else -1)
                if 1 <= k <= n and (rb == 0 or (k * align) % rb != 0):
                    return k * align, align
                if d > 4096:
                    break
        align //= 2
    raise AssertionError(f"no offset inside an operand of {nbytes} bytes")


class Arena:
    """one uint8 allocation of ``nbytes`` filled with NaN; ``place`` puts operands across a boundary, ``strided`` builds far-strided views,
    ``assert_poison`` scans everything outside them on the GPU, ``release`` refills what was handed out"""

    def __init__(self, dev, nbytes: int = ARENA_BYTES):
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.base, self.nbytes = self.buf.data_ptr(), nbytes
        assert self.base % ALIGN == 0 and nbytes % 8 == 0
        self.buf.view(torch.bfloat16).fill_(fp.NAN)
        self.words = self.buf.view(torch.int64)
        self.word = int(self.words[0].item())
        self.pair = self.buf[:8].clone()
        if nbytes >= ARENA_BYTES:
            self.b32, self.b31 = boundaries(self.base, nbytes)
        self.live = []  # [(lo, hi)] byte ranges handed out, relative to the arena

    def _view(self, lo: int, shape, stride, dtype):
        isz = torch.empty((), dtype=dtype).element_size()
        assert lo % isz == 0
        hi = lo + span_elems(shape, stride) * isz
        assert 0 <= lo and hi <= self.nbytes, f"view [{lo}, {hi}) leaves the arena of {self.nbytes} bytes"
        for a, b in self.live:
            assert hi <= a or b <= lo, "views of the arena overlap"
        self.live.append((lo, hi))
        return torch.as_strided(self.buf.view(dtype), tuple(shape), tuple(stride), lo // isz)

    def place(self, t: torch.Tensor, boundary: int, at: float) -> torch.Tensor:
        """a view with ``t``'s dtype, shape, strides and values; ``boundary`` falls inside it at about the fraction ``at`` of its bytes (place_offset)"""
        isz = t.element_size()
        off, _ = place_offset(span_elems(t.shape, t.stride()) * isz, row_sizes(t.shape, t.stride(), isz), at, isz)
        v = self._view(boundary - off - self.base, t.shape, t.stride(), t.dtype)
        v.copy_(t)
        assert v.data_ptr() < boundary < v.data_ptr() + span_elems(t.shape, t.stride()) * isz
        return v

    def strided(self, lo: int, shape, stride, dtype) -> torch.Tensor:
        """an (uninitialised: NaN) view at byte ``lo`` of the arena; the caller writes the rows it addresses.  The whole span counts as handed out: a test
        that wants the bytes between its rows checked poisons the rows again, empties ``live`` and scans the whole arena"""
        return self._view(lo, shape, stride, dtype)

    def _clean(self, a: int, b: int) -> int:
        """number of 8-byte words / edge bytes in [a, b) that no longer hold the poison (0: intact)"""
        if a >= b:
            return 0
        a8, b8 = min(-(-a // 8) * 8, b), max(b // 8 * 8, a)
        bad = 0
        if a8 >= b8:
            return int((self.buf[a:b] != self.pair.repeat(2)[a % 8:a % 8 + (b - a)]).sum())
        if a < a8:
            bad += int((self.buf[a:a8] != self.pair[a % 8:]).sum())
        if b8 < b:
            bad += int((self.buf[b8:b] != self.pair[:b - b8]).sum())
        lo, hi = torch.aminmax(self.words[a8 // 8:b8 // 8])
        if int(lo) != self.word or int(hi) != self.word:
            bad += int((self.words[a8 // 8:b8 // 8] != self.word).sum())
        return bad

    def assert_poison(self, what: str) -> None:
        """the arena outside the views handed out still holds the poison everywhere (one min / max pass over the gaps, on the GPU)"""
        edge, bad = 0, 0
        for a, b in sorted(self.live):
            bad += self._clean(edge, a)
            edge = b
        bad += self._clean(edge, self.nbytes)
        assert bad == 0, f"{what}: {bad} words of the arena outside the placed operands were written"

    def release(self) -> None:
        """refill every view handed out with the poison (their spans, rounded outward to 8 bytes)"""
        for a, b in self.live:
            self.words[a // 8:-(-b // 8)] = self.word
        self.live = []


def need_free(dev, need: int) -> None:
    """skip (the only skip these tests know) when the device has less free memory than ``need`` + 2 GiB"""
    import pytest
    free, _ = torch.cuda.mem_get_info(dev)
    if free < need + 2 ** 31:
        pytest.skip(f"needs {need / 2 ** 30:.1f} GiB + 2 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
