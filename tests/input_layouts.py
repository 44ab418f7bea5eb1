"""How an input lies in memory: re-layouts of one tensor that hold exactly the same values, and the check that a call's
result does not depend on them (Input layouts).  tests/test_gpu_input_layouts.py points it at every entry
family of tests/stream_order.py on the GPU; tests/test_input_layouts_cpu.py checks the re-layouts, the registry's
``refuses`` and the checker itself - with planted mistakes on CPU tensors - without one.  A helper module: no test
functions.

Device variants (torch tensors, on the device of the tensor they are made from):
  offset      contiguous, starting ONE ELEMENT into a flat buffer of numel + 1: ``data_ptr() % 16 == itemsize`` for 4- and
              8-byte types, 8 for complex64.  complex128 cannot be placed off 16 bytes by torch (a storage offset counts
              elements): skipped, and the variant says so.
  strided     not contiguous, the same shape as the leading part of an allocation with one more element per row
              (``buf[..., :n]`` of ``(..., n + 1)``; 1-D: every second element of a buffer twice as long).
  transposed  square 2-D maps and (N, 3) tables: the memory holds the transpose, the tensor is its ``.T``.
Every element of the allocation that is not a value of the input - the leading element, the extra column, the skipped
elements - is PADDING: NaN for real and complex types, the byte 0x7F for integers.  A read through a flat index shows in
the result; a write shows in the padding, which is compared byte by byte after the call, with the values.

Host variants (numpy arrays, for functions that take host arrays): Fortran order, negative strides
(``a[::-1].copy()[::-1]``), read-only, non-native byte order.  The last may be refused with TypeError / ValueError before
any library call; the others must give the same result.

``run_layouts(case, dev, lens)``: the call on plain inputs is the reference; then every variant of every array input,
one input at a time and all inputs together, all under ``dirty_memory.dirty(NAN_BYTES)``, compared by the case's own rule
(tests/test_gpu_stream_order.py: ``_compare``).  ``LibraryGuard`` counts the library calls that are handed device memory
or a stream (size and capability queries take plain numbers and are not work): a REFUSAL is an exception raised while
that count is still zero, and only the (input, variant) pairs of ``Case.refuses`` may be refused; any exception after a
library call is a failure.
"""
import ctypes as ct
import dataclasses

import numpy as np
import pytest

from tests import dirty_memory as dm
from tests import stream_order as so

torch = pytest.importorskip("torch")

DEVICE_VARIANTS = ("offset", "strided", "transposed")
HOST_VARIANTS = ("fortran", "negative_strides", "read_only", "byteswapped")
MAY_REFUSE_ON_HOST = ("byteswapped",)
INT_PAD_BYTE = 0x7F


class LayoutMismatch(AssertionError):
    """What run_layouts raises: every finding of the case, one per line."""


@dataclasses.dataclass
class Variant:
    """One re-layout.  ``view``: the input as the call gets it (None: the variant does not exist for this input, and
    ``note`` says why); ``buffer``: the whole allocation behind it, padding included."""
    name: str
    view: object = None
    buffer: object = None
    note: str = ""


def pad(buf):
    """Every byte of ``buf`` as padding: NaN for floating and complex types, 0x7F bytes for integers."""
    if buf.is_floating_point() or buf.is_complex():
        buf.fill_(complex(float("nan"), float("nan")) if buf.is_complex() else float("nan"))
    else:
        dm.fill_bytes(buf, INT_PAD_BYTE)
    return buf


def raw_bytes(t):
    """The whole storage behind ``t`` (torch) or the elements of ``t`` in index order (numpy), as bytes on the host."""
    if isinstance(t, torch.Tensor):
        return dm._bytes_of(t).cpu().numpy().tobytes()
    return np.asarray(t).tobytes()


def device_variants(t):
    """The device variants of the torch tensor ``t``, on its device."""
    new = lambda shape: pad(torch.empty(shape, dtype=t.dtype, device=t.device))
    n = t.numel()
    if t.dim() == 0 or n == 0:
        return
    if t.element_size() >= 16:
        yield Variant("offset", note=f"{t.dtype}: a storage offset counts whole elements, so no view lies off 16 bytes")
    else:
        flat = new(n + 1)
        view = flat[1:].view(t.shape)
        view.copy_(t)
        yield Variant("offset", view, flat)
    if t.dim() == 1:
        buf = new(2 * n)
        view = buf[::2]
    else:
        buf = new(tuple(t.shape[:-1]) + (t.shape[-1] + 1,))
        view = buf[..., :t.shape[-1]]
    if view.is_contiguous():
        yield Variant("strided", note=f"shape {tuple(t.shape)}: a single row, every view of it is contiguous")
    else:
        view.copy_(t)
        yield Variant("strided", view, buf)
    if t.dim() == 2 and (t.shape[0] == t.shape[1] or t.shape[1] == 3) and min(t.shape) > 1:
        buf = new((t.shape[1], t.shape[0]))
        view = buf.T
        view.copy_(t)
        yield Variant("transposed", view, buf)


def host_variants(a):
    """The host variants of the numpy array ``a``."""
    a = np.asarray(a)
    if a.ndim == 0 or a.size == 0:
        return
    if a.ndim >= 2:
        f = np.asfortranarray(a)
        yield Variant("fortran", f, f)
    base = a[::-1].copy()
    yield Variant("negative_strides", base[::-1], base)
    ro = a.copy()
    ro.setflags(write=False)
    yield Variant("read_only", ro, ro)
    if a.dtype.itemsize > 1 and a.dtype.kind in "iufc":
        sw = a.astype(a.dtype.newbyteorder())
        yield Variant("byteswapped", sw, sw)


def variants(a, on_device):
    """Named re-layouts of one input that hold exactly the same values: the device variants (torch tensors on the device
    of ``a``; a numpy array is taken to the CPU) or the host variants (numpy arrays)."""
    if on_device:
        yield from device_variants(a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)))
    else:
        yield from host_variants(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)


# ------------------------------------------------------------------ the guard around the library
def _is_work(name):
    """Does the C entry ``name`` take device memory or a stream?  An ``ast_*`` entry that returns a status code and has
    a pointer among its arguments; size and capability queries take numbers (or return a size) and are not work."""
    from astrild_amd import _lib
    sig = _lib.SIGNATURES.get(name)
    return name.startswith("ast_") and (sig is None or (sig[0] is ct.c_int and any(a is ct.c_void_p for a in sig[1])))


class LibraryGuard:
    """``with LibraryGuard() as g``: ``astrild_amd._lib.lib()`` hands out a proxy that counts the work calls
    (``g.calls``, their names in ``g.names``)."""

    def __init__(self):
        self.calls, self.names = 0, []

    def __enter__(self):
        from astrild_amd import _lib
        guard, real_lib = self, _lib.lib

        class Proxy:
            def __getattr__(self, name):
                f = getattr(real_lib(), name)
                if not _is_work(name):
                    return f

                def counted(*args):
                    guard.calls += 1
                    guard.names.append(name)
                    return f(*args)
                return counted
        self._mp = pytest.MonkeyPatch()
        self._mp.setattr(_lib, "lib", lambda: Proxy())
        return self

    def __exit__(self, *exc):
        self._mp.undo()
        return False


# ------------------------------------------------------------------ the check
def _is_array(a):
    return isinstance(a, (np.ndarray, torch.Tensor))


def _upload(a):
    return so.cuda_backend().upload(a)


def _host(v):
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return so.tree_map(lambda t: t.detach().cpu().numpy(), v)


def compare(case, got, want, ins):
    """tests/test_gpu_stream_order.py: ``_compare`` (a ``verify`` that raises its own test's assertion: False)."""
    if case.compare == "equal":
        return so.same_bits(got, want)
    if case.verify is not None:
        try:
            return bool(case.verify(got, *ins))
        except AssertionError:
            return False
    return so.close(got, want, *case.compare)


def _input_variants(case, ins, plain, only=None):
    """{input index: {variant name: Variant}} (``only``: of these inputs).  A device input: the device variants of the
    uploaded tensor; the inputs of a ``host_inputs`` case: the host variants (a dict of columns: of every column at once)."""
    out = {}
    for i, a in enumerate(ins):
        if only is not None and i not in only:
            continue
        if case.host_inputs and isinstance(a, dict):
            per = {}
            for key, col in a.items():
                for v in host_variants(np.asarray(col)):
                    per.setdefault(v.name, {})[key] = v
            out[i] = {name: Variant(name, {k: (cols[k].view if k in cols else a[k]) for k in a},
                                    [cols[k].buffer for k in sorted(cols)]) for name, cols in per.items()}
        elif _is_array(a):
            vs = host_variants(a) if case.host_inputs else device_variants(plain[i])
            out[i] = {v.name: v for v in vs}
    return out


def _buffers(v):
    return v.buffer if isinstance(v.buffer, list) else [v.buffer]


def run_layouts(case, dev, lens, upload=_upload, report=print):
    """The module docstring's check for one case.  ``upload``: host array -> the plain tensor the call takes (the GPU
    tests: a fresh contiguous device tensor; the self-tests: a CPU tensor).  Returns the outcomes, one
    ``(label, "same" | "refused" | "skipped: ...")`` per run; raises LayoutMismatch with every finding otherwise."""
    ins, _ = case.make()
    fn = lambda *a: case.call(dev, lens, *a)
    findings, outcomes = [], []
    # ONE dirty allocator around the reference and every variant, as in tests/test_gpu_stream_order.py: the hidden
    # caches (shell geometry: float atomics, the same to the last bit only while it stays cached) are emptied once
    with so.environment(case.env), dm.dirty(dm.NAN_BYTES):
        fresh = lambda i: ins[i] if case.host_inputs else upload(ins[i])
        plain = [fresh(i) for i in range(len(ins))]
        table = _input_variants(case, ins, plain)
        before = [raw_bytes(a) if _is_array(a) else None for a in plain]
        ref = _host(fn(*plain))                                   # the reference: plain inputs
        for i, (a, b) in enumerate(zip(plain, before)):
            if b is not None and i not in case.mutates and raw_bytes(a) != b:
                findings.append(f"plain: input {i} was written")
        want = ref if case.oracle is None else case.oracle(*ins)
        if not compare(case, ref, want, ins):
            findings.append("plain: the result on plain inputs misses the reference")
        names = HOST_VARIANTS if case.host_inputs else DEVICE_VARIANTS
        runs = [(f"input {i}: {name}", {i: name}) for i in sorted(table) for name in names if name in table[i]]
        runs += [(f"all inputs: {name}", {i: name for i in table if name in table[i]}) for name in names
                 if sum(name in table[i] for i in table) > 1]
        for label, chosen in runs:
            for i in case.mutates:                                # what the last run wrote is made anew
                plain[i] = fresh(i)
            table.update(_input_variants(case, ins, plain, only=case.mutates))
            used = {i: table[i][name] for i, name in chosen.items()}
            missing = [f"input {i}: {v.note}" for i, v in used.items() if v.view is None]
            used = {i: v for i, v in used.items() if v.view is not None}
            if not used:
                outcomes.append((label, "skipped: " + "; ".join(missing)))
                continue
            args = [used[i].view if i in used else plain[i] for i in range(len(plain))]
            watched = [(f"input {i} ({v.name})", buf, i) for i, v in used.items() for buf in _buffers(v)]
            watched += [(f"input {i} (plain)", plain[i], i) for i in range(len(plain)) if i not in used and _is_array(plain[i])]
            snaps = [raw_bytes(buf) for _, buf, _ in watched]
            may_refuse = any(name in case.refuses.get(i, ()) for i, name in chosen.items() if i in used) or \
                (case.host_inputs and any(name in MAY_REFUSE_ON_HOST for name in chosen.values()))
            error = None
            with LibraryGuard() as guard:
                try:
                    got = _host(fn(*args))
                except Exception as e:                            # noqa: BLE001 - every exception is classified below
                    error = e
            for (what, buf, i), snap in zip(watched, snaps):
                if i not in case.mutates and raw_bytes(buf) != snap:
                    findings.append(f"{label}: {what} or its padding was written")
            if error is not None:
                kind = f"{type(error).__name__}: {str(error)[:200]}"
                if guard.calls:
                    findings.append(f"{label}: raised after {guard.calls} library calls ({guard.names[-1]} last) - {kind}")
                elif not may_refuse:
                    findings.append(f"{label}: refused, but the registry does not allow it - {kind}")
                elif case.host_inputs and not isinstance(error, (TypeError, ValueError)):
                    findings.append(f"{label}: a host array is refused with TypeError or ValueError - {kind}")
                else:
                    outcomes.append((label, "refused"))
                continue
            if compare(case, got, want, ins):
                outcomes.append((label, "same"))
            else:
                findings.append(f"{label}: the result differs from the plain layout's")
    for label, outcome in outcomes:
        report(f"INPUT_LAYOUTS {case.name}: {label}: {outcome}")
    if findings:
        raise LayoutMismatch(f"{case.name}:\n  " + "\n  ".join(findings))
    return outcomes
