"""A dirty allocator for the tests: for the duration of one test every ``torch.empty``, ``torch.empty_like`` and
``Tensor.new_empty`` that returns a non-empty tensor on the poisoned device type comes back with EVERY BYTE set to one
pattern, so that a kernel which reads scratch or output memory it did not write itself shows up against its oracle.

The C ABI's contract for the scratch and output buffers the wrappers allocate that way is "contents undefined on
entry"; the buffers whose contract is ``+=`` are allocated with ``torch.zeros`` and are left alone here.

Two patterns, every case under both:
  0xFF  NaN as float32 / float64, -1 as int32 / int64, UINT_MAX as an unsigned counter;
  0x7F  finite but huge floats (3.39e38 as float32, 1.39e306 as float64) and huge positive integers - what a
        NaN-ignoring fmin / fmax, or a use as an index or a count, would hide under 0xFF.
0x00 is the control: a result the project documents as order-independent must be bit-identical under it.

What this cannot reach: memory the library allocates itself with hipMalloc (plan internals, twiddle and lane tables,
side-stream scratch) never passes through torch and is not poisoned; tests/test_gpu_call_order.py reaches that state
through the order of calls only.
"""
import contextlib

import pytest

torch = pytest.importorskip("torch")

NAN_BYTES = 0xFF
HUGE_BYTES = 0x7F
ZERO_BYTES = 0x00
PATTERNS = (NAN_BYTES, HUGE_BYTES)
PATTERN_IDS = {NAN_BYTES: "0xFF", HUGE_BYTES: "0x7F", ZERO_BYTES: "0x00"}

#: module-level caches of the package that hold device tensors (or plans that own device memory), as
#: (module path, attribute): replaced by empty dicts for the test, so that their scratch is allocated anew - dirty.
CACHES = (("astrild_amd.device", "_power_scratch"), ("astrild_amd.device", "_geom_cache"),
          ("astrild_amd.lensing", "_lens_plans"), ("astrild_amd.lensing", "_smooth_plans"))


def _bytes_of(t):
    """The whole storage of ``t`` as a flat uint8 tensor (any dtype, any memory format)."""
    storage = t.untyped_storage()
    return torch.tensor([], dtype=torch.uint8, device=t.device).set_(storage, 0, (storage.nbytes(),))


def fill_bytes(t, pattern):
    _bytes_of(t).fill_(int(pattern))
    return t


def all_bytes_are(t, pattern):
    b = _bytes_of(t)
    return b.numel() > 0 and bool((b == int(pattern)).all().item())


def _pinned(t):
    try:
        return t.device.type == "cpu" and t.is_pinned()
    except RuntimeError:                      # no accelerator to ask: not pinned
        return False


class DirtyAllocator:
    """Counts and poisons the fresh tensors of ``device_types`` (the tests on the GPU: ("cuda",); the byte logic itself
    is exercised on ("cpu",) tensors where there is no GPU).  Pinned-host and meta tensors, tensors of other device
    types and empty tensors pass through untouched."""

    def __init__(self, pattern, device_types=("cuda",)):
        self.pattern = int(pattern)
        self.device_types = tuple(device_types)
        self.allocations = 0
        self.bytes = 0
        self.log = []                         # (dtype, shape) of every poisoned tensor, in order

    def poison(self, t):
        if not isinstance(t, torch.Tensor) or t.device.type not in self.device_types or t.numel() == 0 or _pinned(t):
            return t
        fill_bytes(t, self.pattern)
        self.allocations += 1
        self.bytes += t.untyped_storage().nbytes()
        self.log.append((t.dtype, tuple(t.shape)))
        return t

    @contextlib.contextmanager
    def using(self, pattern):
        """Another pattern for a while (the all-zero control of a bit-identity case); counted like the rest."""
        saved, self.pattern = self.pattern, int(pattern)
        try:
            yield self
        finally:
            self.pattern = saved

    def mark(self):
        return self.allocations

    def since(self, mark):
        return self.allocations - mark

    def install(self, monkeypatch):
        import importlib
        real_empty, real_empty_like, real_new_empty = torch.empty, torch.empty_like, torch.Tensor.new_empty
        poison = self.poison

        def empty(*args, **kwargs):
            return poison(real_empty(*args, **kwargs))

        def empty_like(*args, **kwargs):
            return poison(real_empty_like(*args, **kwargs))

        def new_empty(self_, *args, **kwargs):
            return poison(real_new_empty(self_, *args, **kwargs))

        monkeypatch.setattr(torch, "empty", empty)
        monkeypatch.setattr(torch, "empty_like", empty_like)
        monkeypatch.setattr(torch.Tensor, "new_empty", new_empty)
        for module, name in CACHES:
            monkeypatch.setattr(importlib.import_module(module), name, {})
        return self


@contextlib.contextmanager
def dirty(pattern, device_types=("cuda",)):
    """``with dirty(0xFF) as alloc: ...`` - the patches and the emptied caches are undone on exit."""
    mp = pytest.MonkeyPatch()
    try:
        yield DirtyAllocator(pattern, device_types).install(mp)
    finally:
        mp.undo()


@pytest.fixture(params=PATTERNS, ids=[PATTERN_IDS[p] for p in PATTERNS])
def dirty_alloc(request, monkeypatch):
    """The dirty allocator for one test, once per pattern.  Import it into a test module to use it."""
    return DirtyAllocator(request.param).install(monkeypatch)
