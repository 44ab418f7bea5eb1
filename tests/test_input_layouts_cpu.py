"""Without a GPU: the re-layouts of tests/input_layouts.py hold the same values in the stated places, the registry's
``refuses`` names only (input, variant) pairs a contiguity assert stands behind, and ``run_layouts`` reports the mistakes
it is for - planted here in torch ops on CPU tensors."""
import inspect
import re
import types

import numpy as np
import pytest

from tests import input_layouts as il
from tests import stream_order as so

torch = pytest.importorskip("torch")

DTYPES = (torch.float32, torch.float64, torch.int32, torch.int64, torch.complex64, torch.complex128)
SHAPES = ((7,), (5, 3), (6, 6), (4, 5, 6), (1, 9))


def _values(shape, dtype):
    n = int(np.prod(shape))
    t = torch.arange(1, n + 1, dtype=torch.float64).reshape(shape)
    return torch.complex(t, -t).to(dtype) if dtype.is_complex else t.to(dtype)


def _padding_elements(v):
    """How many elements of the variant's allocation still hold the padding pattern once the view's own values are
    zeroed in a copy of it."""
    chk = v.buffer.clone()
    torch.as_strided(chk, v.view.shape, v.view.stride(), v.view.storage_offset()).zero_()
    if chk.is_complex():
        r = torch.view_as_real(chk)
        return int((torch.isnan(r[..., 0]) & torch.isnan(r[..., 1])).sum())
    if chk.is_floating_point():
        return int(torch.isnan(chk).sum())
    return int((chk == int.from_bytes(bytes([il.INT_PAD_BYTE]) * chk.element_size(), "little")).sum())


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d)[6:] for d in DTYPES])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_device_variants(shape, dtype):
    t = _values(shape, dtype)
    found = {v.name: v for v in il.variants(t, on_device=True)}
    square_or_table = len(shape) == 2 and (shape[0] == shape[1] or shape[1] == 3) and min(shape) > 1
    assert set(found) == {"offset", "strided"} | ({"transposed"} if square_or_table else set())
    for v in found.values():
        if v.view is None:
            assert v.note and ((v.name == "offset" and dtype == torch.complex128) or (v.name == "strided" and shape == (1, 9)))
            continue
        assert v.view.dtype == t.dtype and v.view.shape == t.shape and torch.equal(v.view, t)
        assert v.view.untyped_storage().data_ptr() == v.buffer.untyped_storage().data_ptr()
        assert v.buffer.untyped_storage().data_ptr() % 64 == 0
        assert _padding_elements(v) == v.buffer.numel() - t.numel()
    off = found["offset"]
    if off.view is not None:
        assert off.view.is_contiguous() and off.buffer.numel() == t.numel() + 1 and off.view.storage_offset() == 1
        assert off.view.data_ptr() % 16 == t.element_size()
    st = found["strided"]
    if st.view is not None:
        assert not st.view.is_contiguous() and st.view.data_ptr() == st.buffer.data_ptr()
        if len(shape) == 1:
            assert st.view.stride() == (2,) and st.buffer.numel() == 2 * t.numel()
        else:
            rows = torch.empty(shape[:-1] + (shape[-1] + 1,)).stride()
            assert st.view.stride() == rows and tuple(st.buffer.shape) == shape[:-1] + (shape[-1] + 1,)
    if "transposed" in found:
        tr = found["transposed"]
        assert not tr.view.is_contiguous() and tr.view.stride() == (1, shape[0]) and tr.buffer.is_contiguous()
        assert torch.equal(tr.buffer, t.T) and tr.buffer.numel() == t.numel()


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32, np.complex128], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(7,), (5, 3), (4, 5, 6)], ids=str)
def test_host_variants(shape, dtype):
    a = _values(shape, torch.float64).numpy().astype(dtype)
    found = {v.name: v for v in il.variants(a, on_device=False)}
    assert set(found) == set(il.HOST_VARIANTS) - ({"fortran"} if len(shape) == 1 else set())
    for v in found.values():
        assert v.view.shape == a.shape and np.array_equal(v.view, a)
    if "fortran" in found:
        assert found["fortran"].view.flags.f_contiguous and not found["fortran"].view.flags.c_contiguous
    assert all(s < 0 for s in found["negative_strides"].view.strides[:1]) and not found["negative_strides"].view.flags.c_contiguous
    assert not found["read_only"].view.flags.writeable and found["read_only"].view.dtype == a.dtype
    assert not found["byteswapped"].view.dtype.isnative and found["byteswapped"].view.dtype.newbyteorder() == a.dtype


# ------------------------------------------------------------------ the registry
CONTIGUITY_ASSERT = re.compile(r"^\s*assert\b[^\n]*\bis_contiguous\(\)", re.M)


def _resolve(name):
    from astrild_amd import device, lensing
    obj = lensing if name.startswith("lensing.") else device
    for part in name.replace("lensing.", "", 1).split("."):
        obj = getattr(obj, part)
    return obj


def registry_problems(cases):
    """What is wrong with the ``refuses`` / ``refused_by`` / ``mutates`` of these cases, as a list of sentences."""
    problems = []
    for c in cases:
        ins, _ = c.make()
        for i, names in c.refuses.items():
            if not 0 <= i < len(ins):
                problems.append(f"{c.name}: refuses names input {i} of {len(ins)}")
            if "offset" in names:
                problems.append(f"{c.name}: a contiguous tensor (offset) is valid input to every function")
            if not set(names) <= {"strided", "transposed"}:
                problems.append(f"{c.name}: unknown variants {sorted(set(names) - set(il.DEVICE_VARIANTS))}")
        if bool(c.refuses) != bool(c.refused_by):
            problems.append(f"{c.name}: refusals and the functions that hold the check are named together")
        if c.refuses and c.host_inputs:
            problems.append(f"{c.name}: a host array is never refused for its layout")
        for name in c.refused_by:
            try:
                src = inspect.getsource(_resolve(name))
            except AttributeError:
                problems.append(f"{c.name}: {name} does not exist")
                continue
            if not CONTIGUITY_ASSERT.search(src):
                problems.append(f"{c.name}: {name} holds no assert of is_contiguous()")
        if any(not 0 <= i < len(ins) for i in c.mutates):
            problems.append(f"{c.name}: mutates names an input that does not exist")
    return problems


def test_refusals_stand_on_a_contiguity_assert():
    assert registry_problems(so.CASES) == []
    assert sum(bool(c.refuses) for c in so.CASES) > 20                        # (the paint, FFT and in-place families)
    by_name = {c.name: c for c in so.CASES}
    import dataclasses
    # the check has teeth: a function without an assert, and an "offset" entry, are both reported
    wrong = dataclasses.replace(by_name["total_mass"], refuses={0: frozenset({"strided"})}, refused_by=("total_mass",))
    assert any("holds no assert" in p for p in registry_problems([wrong]))
    wrong = dataclasses.replace(by_name["r2c_tile_256"], refuses={0: frozenset({"offset", "strided"})})
    assert any("offset" in p for p in registry_problems([wrong]))
    wrong = dataclasses.replace(by_name["r2c_tile_256"], refused_by=())
    assert any("named together" in p for p in registry_problems([wrong]))


# ------------------------------------------------------------------ the checker, on CPU tensors
def _cpu_case(op, name="planted", **kw):
    def make():
        x = np.arange(1.0, 31.0).reshape(6, 5)
        w = np.arange(1, 7, dtype=np.int32)
        return [x, w, 3.0], [x[::-1].copy(), w[::-1].copy(), 3.0]
    return so.Case(name=name, covers=(), make=make, call=lambda dev, lens, x, w, k: op(x, w, k), **kw)


def _run(case):
    lines = []
    upload = lambda a: torch.from_numpy(np.ascontiguousarray(a)).clone() if isinstance(a, np.ndarray) else a
    return il.run_layouts(case, None, None, upload=upload, report=lines.append), lines


def _correct(x, w, k):
    return (x * k).sum(dim=1) * w, x.clone()


def test_a_correct_op_is_the_same_on_every_layout():
    outcomes, lines = _run(_cpu_case(_correct))
    labels = [label for label, _ in outcomes]
    assert labels == ["input 0: offset", "input 0: strided", "input 1: offset", "input 1: strided",
                      "all inputs: offset", "all inputs: strided"]              # ((6, 5) is neither square nor a table)
    assert all(outcome == "same" for _, outcome in outcomes) and len(lines) == len(outcomes)


def test_planted_flat_walk_of_a_strided_input():
    def op(x, w, k):
        flat = torch.as_strided(x, (x.numel(),), (1,), x.storage_offset())        # what ptr(t) + a flat index reads
        return (flat.reshape(x.shape) * k).sum(dim=1) * w, flat.reshape(x.shape).clone()
    with pytest.raises(il.LayoutMismatch) as e:
        _run(_cpu_case(op))
    text = str(e.value)
    assert "input 0: strided: the result differs" in text and "all inputs: strided: the result differs" in text
    assert "offset" not in text and "input 1" not in text and "written" not in text


def test_planted_dropped_storage_offset():
    def op(x, w, k):
        base = torch.as_strided(x, x.shape, x.stride(), 0)                        # the allocation's start, not the view's
        return (base * k).sum(dim=1) * w, base.clone()
    with pytest.raises(il.LayoutMismatch) as e:
        _run(_cpu_case(op))
    text = str(e.value)
    assert "input 0: offset: the result differs" in text and "all inputs: offset: the result differs" in text
    assert "strided" not in text and "input 1" not in text


def test_planted_write_to_an_input_and_to_its_padding():
    def op(x, w, k):
        out = _correct(x, w, k)
        w.add_(1)
        return out
    with pytest.raises(il.LayoutMismatch) as e:
        _run(_cpu_case(op))
    text = str(e.value)
    assert "plain: input 1 was written" in text and "input 1: strided: input 1 (strided) or its padding was written" in text
    assert "input 0: offset: input 1 (plain) or its padding was written" in text
    _run(_cpu_case(op, mutates=(1,)))                                             # documented: not a finding (the result is the same)

    def pads(x, w, k):
        out = _correct(x, w, k)
        torch.as_strided(x, (1,), (1,), max(x.storage_offset() - 1, 0)).copy_(x.reshape(-1)[:1])    # one element in front
        return out
    with pytest.raises(il.LayoutMismatch) as e:
        _run(_cpu_case(pads))
    assert "input 0: offset: input 0 (offset) or its padding was written" in str(e.value)


def _asserting(x, w, k):
    assert x.is_contiguous()
    return _correct(x, w, k)


def test_refusals_are_held_against_the_registry():
    outcomes, _ = _run(_cpu_case(_asserting, refuses={0: so._NCT}, refused_by=("r2c",)))
    assert dict(outcomes)["input 0: strided"] == "refused" and dict(outcomes)["all inputs: strided"] == "refused"
    assert dict(outcomes)["input 0: offset"] == "same" and dict(outcomes)["input 1: strided"] == "same"
    with pytest.raises(il.LayoutMismatch, match="input 0: strided: refused, but the registry does not allow it"):
        _run(_cpu_case(_asserting))
    with pytest.raises(il.LayoutMismatch, match="input 0: strided: refused, but the registry does not allow it"):
        _run(_cpu_case(_asserting, refuses={1: so._NC}, refused_by=("r2c",)))   # (another input's entry does not cover it)


def test_an_exception_after_a_library_call_is_never_a_refusal(monkeypatch):
    from astrild_amd import _lib
    fake = types.SimpleNamespace(ast_sum=lambda *a: 0, ast_fft_tile_supported=lambda *a: 1,
                                 ast_last_error=lambda: b"")
    monkeypatch.setattr(_lib, "lib", lambda: fake)

    def op(x, w, k):
        _lib.lib().ast_fft_tile_supported(0, 256)                                # a query: not work
        assert x.is_contiguous() or _lib.lib().ast_sum(None, 0, 0, None, None) != 0, "late"
        return _correct(x, w, k)
    with pytest.raises(il.LayoutMismatch, match=r"input 0: strided: raised after 1 library calls \(ast_sum last\)"):
        _run(_cpu_case(op, refuses={0: so._NCT}, refused_by=("r2c",)))
    with il.LibraryGuard() as g:
        _lib.lib().ast_fft_tile_supported(0, 256)
        assert g.calls == 0
        _lib.lib().ast_sum(None, 0, 0, None, None)
        assert g.calls == 1 and g.names == ["ast_sum"]
    assert _lib.lib() is fake


def test_host_inputs_take_the_host_variants():
    seen = []

    def op(cat):
        seen.append({k: (v.flags.writeable, v.dtype.isnative, v.strides[0] > 0) for k, v in cat.items()})
        if not all(v.dtype.isnative for v in cat.values()):
            raise TypeError("byte order")
        return torch.from_numpy(np.ascontiguousarray(cat["a"]) * 2.0 + np.ascontiguousarray(cat["b"]))
    make = lambda: ([{"a": np.arange(1.0, 6.0), "b": np.arange(5.0, 0.0, -1.0)}], [{"a": np.zeros(5), "b": np.ones(5)}])
    case = so.Case(name="host", covers=(), make=make, call=lambda dev, lens, cat: op(cat), host_inputs=True)
    outcomes, _ = _run(case)
    assert dict(outcomes) == {"input 0: negative_strides": "same", "input 0: read_only": "same", "input 0: byteswapped": "refused"}
    assert seen[1] == {"a": (True, True, False), "b": (True, True, False)} and seen[2]["a"][0] is False
    refusing = so.Case(name="host", covers=(), make=make, host_inputs=True,
                       call=lambda dev, lens, cat: op({k: np.require(v, requirements="W") for k, v in cat.items()})
                       if all(v.flags.writeable for v in cat.values()) else (_ for _ in ()).throw(ValueError("read-only")))
    with pytest.raises(il.LayoutMismatch, match="input 0: read_only: refused, but the registry does not allow it"):
        _run(refusing)
