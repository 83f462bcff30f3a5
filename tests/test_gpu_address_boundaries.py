"""Operands across 4 GiB address multiples on an MI355X (small shapes; DESIGN.md: "Address-range guards").

Every launch form of tests/_op_launches.py runs once with all operands in ordinary memory -- the baseline, anchored against the family's reference in
fp64 at the tolerance of the parity test of the same kernel (``Spec.gate`` names it) -- and then again with ONE operand inside the arena of
tests/_bigmem.py, placed so that a multiple of 2^32 falls into the middle of one of its rows:

  * every input and every output the caller owns, at 0.4 of its bytes and one row in;
  * every tensor the Python wrapper allocates for the launch (outputs and scratch: the wrapper's ``torch.empty`` / ``zeros`` calls are answered from
    the arena for the one allocation under test), the same two ways;
  * the main input and the main output once more across an ODD multiple of 2^31 (bit 31 of the address changes inside the operand);
  * the workspace of the launches that take one (GEMM / conv K split, attention5.hip's key split).

Each rerun demands: the output is BIT-identical to the baseline (same kernel, route and values; only the address differs -- a tolerance would hide
exactly the dropped carry looked for) and the planner's answer is unchanged where a planner exists; the arena outside the placed operand still holds
its NaN everywhere (an address that lost its carry lands 4 GiB lower, inside the arena: a stray write shows here, a stray read returns NaN); the output
holds no NaN.  Needs 8.5 GiB of device memory (the arena), held by the module's fixture and freed at its teardown."""
import importlib
from contextlib import contextmanager

import pytest
import torch

from tests import _bigmem as bm
from tests import _footprint as fp
from tests import _op_launches as L
from tests._util import max_abs, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arena(dev):
    from diffusionkit_amd import _lib, ops
    bm.need_free(dev, bm.ARENA_BYTES)
    ops.zero_page(dev), ops.gemm_workspace(dev), _lib.ensure_attention_workspace(dev)  # (cached by the package: never to be answered from the arena)
    a = bm.Arena(dev)
    print(f"[address] arena at {a.base:#x}, 2^32 multiple {a.b32:#x}, odd 2^31 multiple {a.b31:#x}")
    yield a
    a.buf = a.words = a.pair = None
    del a
    torch.cuda.empty_cache()


class _Torch:
    """stands in for the ``torch`` module inside a wrapper module: ``empty`` / ``empty_like`` / ``zeros`` go through ``hook``, the rest is torch's"""

    def __init__(self, hook):
        self._hook = hook

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *a, **k):
        return self._hook(torch.empty(*a, **k), False)

    def empty_like(self, *a, **k):
        return self._hook(torch.empty_like(*a, **k), False)

    def zeros(self, *a, **k):
        return self._hook(torch.zeros(*a, **k), True)


@contextmanager
def allocations(modules, hook):
    """``torch.empty`` / ``torch.empty_like`` / ``torch.zeros`` calls made through the module global ``torch`` of diffusionkit_amd.<module> go through
    ``hook`` for the block.  That is every allocation the wrappers in ops.py and text.py make today.  NOT covered: ``torch.empty_strided``,
    ``Tensor.new_empty`` / ``.clone()`` / ``.contiguous()`` copies, allocations in other modules or inside the library -- those would stay in
    ordinary memory without notice (the count check below only compares a rerun with the baseline of the same wrapper)."""
    mods = [importlib.import_module("diffusionkit_amd." + m) for m in modules]
    try:
        for m in mods:
            m.torch = _Torch(hook)
        yield
    finally:
        for m in mods:
            m.torch = torch


def _cpu(y):
    return {k: v.detach().clone().cpu() for k, v in y.items()} if isinstance(y, dict) else {"": y.detach().clone().cpu()}


def _one_row_in(t):
    isz = t.element_size()
    rows = bm.row_sizes(t.shape, t.stride(), isz)
    return rows[0] / (bm.span_elems(t.shape, t.stride()) * isz) if rows else None


def run_spec(dev, arena, s, what):
    def fresh():
        v = {k: t.to(dev, s.kind(k)).contiguous() for k, t in s.ops.items()}
        for k, (shape, dt) in s.outs.items():
            shape = shape() if callable(shape) else shape
            v[k] = torch.zeros(shape, dtype=dt, device=dev) if dt == torch.uint8 else torch.full(shape, L.SENTINEL, dtype=dt, device=dev)
        if s.ws:
            v[s.ws[0]] = torch.zeros(s.ws[1], dtype=torch.uint8, device=dev)
        return v

    # the baseline: everything in ordinary memory; the wrapper's allocations are counted
    made = []

    def count(t, zero):
        made.append(t)
        return t
    v = fresh()
    with allocations(s.modules, count):
        res = s.launch(v)
    base = _cpu(res)
    plan0 = s.plan(v) if s.plan else None
    torch.cuda.synchronize()
    stores = {t.untyped_storage().data_ptr() for t in (res.values() if isinstance(res, dict) else [res])}
    made_out = [i for i, t in enumerate(made) if t.untyped_storage().data_ptr() in stores]
    made_ok = [i for i, t in enumerate(made) if t.numel() * t.element_size() >= 8]
    n_made = len(made)
    del made[:]
    for k, y in base.items():
        if y.is_floating_point():
            assert bool(torch.isfinite(y).all()), f"{what}: the baseline output {k} holds non-finite values"
    ref = s.ref({k: (t.double() if t.is_floating_point() else t) for k, t in s.ops.items()})
    got = s.pick(res)
    tol_rel, tol_abs, src = s.gate
    for k, r in (ref.items() if isinstance(ref, dict) else [("", ref)]):
        g = (got[k] if isinstance(got, dict) else got).detach().double().cpu()
        if tol_rel == "exact":
            assert torch.equal(g, r.double()), f"{what} {k}: the baseline is not the reference element for element ({src})"
            print(f"[address] {what} {k}: baseline equals the reference element for element [{src}]")
            continue
        e, m = rel_l2(r, g), max_abs(r, g)
        if s.differ is not None:
            share = float((g != r.double()).double().mean())
            print(f"[address] {what}: {share:.4f} of the elements differ from the reference (< {s.differ})")
            assert share < s.differ, f"{what}: {share:.4f} of the elements differ from the reference ({src})"
        print(f"[address] {what}{' ' + k if k else ''}: baseline vs fp64 rel_l2 {e:.3e} (< {tol_rel}), max_abs {m:.3e} (< {tol_abs}) [{src}]")
        assert tol_rel is None or e < tol_rel, f"{what} {k}: baseline rel_l2 {e:.3e} >= {tol_rel} ({src})"
        assert tol_abs is None or m < tol_abs, f"{what} {k}: baseline max_abs {m:.3e} >= {tol_abs} ({src})"

    # the placements
    todo = []
    for k, t in v.items():
        if s.ws and k == s.ws[0]:
            todo.append((k, "b32", 0.4))
            continue
        if t.numel() * t.element_size() < 8:
            continue
        todo.append((k, "b32", 0.4))
        if _one_row_in(t) is not None:
            todo.append((k, "b32", _one_row_in(t)))
    for i in made_ok:
        todo += [(i, "b32", 0.4), (i, "b32", "row")]
    for k in (s.main_in, s.main_out):
        if k is not None and (k, "b31", 0.4) not in todo:
            todo.append((k, "b31", 0.4))
    if s.main_out is None:
        todo += [(i, "b31", 0.4) for i in made_out[:1]]
    n = 0
    for target, which, at in todo:
        boundary = arena.b32 if which == "b32" else arena.b31
        label = f"{what}: {'allocation ' + str(target) if isinstance(target, int) else target} across {which} at {at if at == 'row' else round(at, 4)}"
        v = fresh()
        if not isinstance(target, int):
            v[target] = arena.place(v[target], boundary, at)
        seen = []

        def hook(t, zero):
            seen.append(1)
            if len(seen) - 1 != target:
                return t
            frac = (_one_row_in(t) or 0.4) if at == "row" else at
            return arena.place(t.zero_() if zero else t.fill_(fp.NAN) if t.is_floating_point() else t.fill_(0xFF), boundary, frac)
        with allocations(s.modules, hook):
            res = s.launch(v)
        y = _cpu(res)
        plan = s.plan(v) if s.plan else None
        assert len(seen) == n_made, f"{label}: the wrapper made {len(seen)} allocations, the baseline {n_made}"
        for k, b in base.items():
            diff = fp.bits(y[k]) != fp.bits(b)
            assert not bool(diff.any()), (f"{label}: output {k or 'y'}: {int(diff.sum())} of {diff.numel()} elements differ in their bits from the baseline, "
                                          f"first at {tuple(int(i) for i in torch.nonzero(diff)[0])}")
            if y[k].is_floating_point():
                assert not bool(torch.isnan(y[k]).any()), f"{label}: NaN in output {k or 'y'}"
        assert plan == plan0, f"{label}: the plan changed with the address: {plan} against {plan0}"
        del res, v
        arena.assert_poison(label)
        arena.release()
        n += 1
    print(f"[address] {what}: {n} placements bit-identical to the baseline, arena intact")


@pytest.mark.parametrize("name", list(L.SPECS))
def test_operand_across_address_multiples(dev, arena, name):
    """module docstring; the baseline's tolerance and the parity test it is taken from are printed with the measured figures"""
    run_spec(dev, arena, L.SPECS[name](), name)
