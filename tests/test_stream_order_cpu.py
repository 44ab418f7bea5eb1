"""Without a GPU: the registry of tests/stream_order.py is complete, its decoys are valid inputs, and ``late_call`` keeps
its books (producer behind the sleep, ``armed`` taken when the call returns, every output cloned before the wait)."""
import contextlib
import inspect
import re

import numpy as np
import pytest

from tests import stream_order as so

torch = pytest.importorskip("torch")

STREAM_CALL = re.compile(r"(?<![\w.])stream\(\)")


def _modules():
    from astrild_amd import device, lensing
    return (device, ""), (lensing, "lensing.")


def stream_taking_functions():
    """Every public function of device.py and lensing.py - and every public method, or __init__, of their public
    classes - whose source passes ``stream()`` to the library."""
    found = set()
    for module, prefix in _modules():
        for name, obj in vars(module).items():
            if name.startswith("_") or getattr(obj, "__module__", None) != module.__name__:
                continue
            if inspect.isfunction(obj):
                if STREAM_CALL.search(inspect.getsource(obj)):
                    found.add(prefix + name)
            elif inspect.isclass(obj):
                for mname, meth in vars(obj).items():
                    if inspect.isfunction(meth) and (not mname.startswith("_") or mname == "__init__") \
                            and STREAM_CALL.search(inspect.getsource(meth)):
                        found.add(prefix + name + "." + mname)
    return found


def _resolve(name):
    from astrild_amd import device, lensing
    obj = lensing if name.startswith("lensing.") else device
    for part in name.replace("lensing.", "", 1).split("."):
        obj = getattr(obj, part)
    return obj


def test_every_stream_taking_function_has_a_case_or_a_named_exemption():
    found = stream_taking_functions()
    assert len(found) > 40 and "power_sums_fused" in found and "lensing.LensPlan.alphas" in found
    covered = so.covered()
    missing = sorted(found - covered - set(so.EXEMPT))
    assert not missing, f"no case and no exemption: {missing}"
    assert not set(so.EXEMPT) & covered, "an exempted function has a case"
    assert set(so.EXEMPT) <= found, f"exempted, but not (or no longer) a stream-taking function: {sorted(set(so.EXEMPT) - found)}"
    assert all(reason and len(reason) > 10 for reason in so.EXEMPT.values())
    for name in covered:                      # (also what the cases reach through other wrappers: the names must exist)
        assert callable(_resolve(name)), name


def test_cases_are_well_formed():
    names = [c.name for c in so.CASES]
    assert len(set(names)) == len(names)
    for c in so.CASES:
        assert c.compare == "equal" or (len(c.compare) == 2 and 0 <= c.compare[1] <= c.compare[0] + 1e-300 <= 1e-5
                                        and c.tol_from), c.name
        assert c.verify is None or c.compare != "equal"
        assert bool(c.sync_line) == c.host_syncs, f"{c.name}: a host synchronisation is named exactly where one is declared"
        assert c.oracle is None or c.compare != "equal"


@pytest.mark.parametrize("c", so.CASES, ids=[c.name for c in so.CASES])
def test_decoys_are_valid_inputs(c):
    ins, dec = c.make()
    assert len(ins) == len(dec)
    differ = False
    for a, b in zip(ins, dec):
        if isinstance(a, dict):
            assert sorted(a) == sorted(b)
            pairs = [(np.asarray(a[k]), np.asarray(b[k])) for k in a]
        elif a is None:
            assert b is None
            continue
        else:
            pairs = [(a, b)]
        for x, y in pairs:
            tx, ty = torch.as_tensor(x), torch.as_tensor(y)                 # what the probe uploads, as CPU tensors
            assert tx.shape == ty.shape and tx.dtype == ty.dtype
            assert not (tx.is_floating_point() or tx.is_complex()) or bool(torch.isfinite(torch.view_as_real(ty) if ty.is_complex() else ty).all())
            differ = differ or not torch.equal(tx, ty)
    assert differ or not ins, "the decoy equals the input"
    if c.check is not None:
        c.check(*ins)
        c.check(*dec)


# ------------------------------------------------------------------ late_call with a host stand-in for the device
class HostBackend:
    """Streams are queues of closures that run when they are waited for: what is queued behind a sleep has not happened
    when the call under test returns, exactly as on the device."""

    def __init__(self):
        self.queues = {"null": [], "S": []}
        self.current = "null"
        self.log = []

    def stream(self, i=0):
        assert i == 0
        return "S"

    def default_stream(self):
        return "null"

    @contextlib.contextmanager
    def on(self, s):
        saved, self.current = self.current, s
        try:
            yield
        finally:
            self.current = saved

    def _queue(self, what, f):
        self.log.append((self.current, what))
        self.queues[self.current].append(f)

    def sleep(self, s, ms):
        self.log.append((s, f"sleep {ms:g}"))
        self.queues[s].append(lambda: None)

    def upload(self, a):
        if isinstance(a, np.ndarray):
            t = torch.from_numpy(a.copy())
            self.log.append((self.current, "upload"))
            return t
        return a

    def overwrite(self, dst, src):
        if isinstance(dst, torch.Tensor):
            self._queue("produce", lambda: dst.copy_(src))

    def record(self):
        e = {"done": False}
        self._queue("record", lambda: e.update(done=True))
        return e

    def done(self, e):
        self.log.append((self.current, "query"))
        return e["done"]

    def clone(self, t):
        out = torch.empty_like(t)
        self._queue("clone", lambda: out.copy_(t))
        return out

    def wait_all(self, s):
        self.log.append((s, "wait"))
        for q in (self.queues[s], self.queues["null"]):
            while q:
                q.pop(0)()


def test_late_call_bookkeeping_on_the_host():
    be = HostBackend()
    x, decoy = np.arange(6.0), np.arange(6.0)[::-1].copy()
    seen = {}

    def fn(t, flag):
        seen["at_call"] = t.clone()                                          # what an eager read would have got
        seen["flag"] = flag
        out = torch.empty_like(t)
        be._queue("kernel", lambda: out.copy_(t * 2))
        return {"twice": out, "n": 6, "host": np.array([1, 2])}
    out, armed = so.late_call(fn, [x, "plain"], [decoy, "plain"], backend=be)
    assert armed                                                             # nothing waited: the producer had not run
    assert torch.equal(seen["at_call"], torch.from_numpy(decoy)) and seen["flag"] == "plain"
    assert torch.equal(out["twice"], torch.from_numpy(2 * x))                # the stream-ordered result saw the real input
    assert out["n"] == 6 and np.array_equal(out["host"], [1, 2])
    what = [w for _, w in be.log]
    order = [what.index(w) for w in ("sleep 120", "sleep 40", "produce", "record", "kernel", "query", "clone")]
    assert order == sorted(order), be.log
    assert what.index("clone") < len(what) - 1 - what[::-1].index("wait")    # cloned before the last wait, i.e. before return
    assert ("null", "sleep 120") in be.log and ("S", "sleep 40") in be.log and ("S", "clone") in be.log
    assert all(s == "S" for s, w in be.log if w in ("produce", "record", "kernel", "clone"))


def test_late_call_reports_a_call_that_waited_for_the_stream():
    be = HostBackend()

    def syncing(t):
        be.wait_all("S")                                                     # a host read of a device value
        return t * 2
    out, armed = so.late_call(syncing, [np.arange(4.0)], [np.zeros(4)], backend=be)
    assert not armed and torch.equal(out, torch.arange(4.0, dtype=torch.float64) * 2)


def test_late_call_hands_host_inputs_over_as_they_are():
    be = HostBackend()
    x = np.arange(4.0)
    out, armed = so.late_call(lambda a: (a is x, torch.from_numpy(a) + 1), [x], [x[::-1].copy()], host_inputs=True, backend=be)
    assert out[0] is True and torch.equal(out[1], torch.from_numpy(x) + 1)


def test_comparisons():
    a = {"k": np.array([1.0, np.nan]), "n": np.array([3, 4])}
    assert so.same_bits(a, {"n": np.array([3, 4]), "k": np.array([1.0, np.nan])})
    assert not so.same_bits(a, {"k": np.array([1.0, np.nan]), "n": np.array([3, 5])})
    assert so.close(a, {"k": np.array([1.0 + 1e-13, np.nan]), "n": np.array([3, 4])}, 1e-12)
    small = {"k": np.array([1.0, 1e-6]), "n": np.array([3, 4])}
    off = {"k": np.array([1.0, 1e-6 + 1e-13]), "n": np.array([3, 4])}
    assert not so.close(off, small, 1e-12) and so.close(off, small, 1e-12, 1e-12)      # no absolute term unless asked for
    assert not so.close(a, {"k": np.array([1.0 + 1e-9, np.nan]), "n": np.array([3, 4])}, 1e-12)
    assert not so.close(a, {"k": np.array([1.0, np.nan]), "n": np.array([3, 5])}, 1e-3)
    assert not so.close(a, {"k": np.array([1.0, 2.0]), "n": np.array([3, 4])}, 1e-3)
    assert not so.close(np.array([1e300]), np.array([1.0]), 1e-6)
