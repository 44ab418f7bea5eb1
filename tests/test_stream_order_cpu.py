"""Without a GPU: the registry of tests/stream_order.py is complete, its decoys are valid inputs, and ``late_call`` keeps
its books (producer behind the sleep, ``armed`` taken when the call returns, every output cloned before the wait)."""
import ast as pyast
import contextlib
import inspect
import pathlib
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


# ------------------------------------------------------------------ the registry of hidden state
PACKAGE = pathlib.Path(__file__).resolve().parent.parent / "astrild_amd"
MUTATORS = {"clear", "pop", "setdefault", "append", "update"}
CONTAINER_CALLS = {"dict", "list", "set", "OrderedDict"}


def mutated_module_containers(source):
    """The module-level names of ``source`` that are bound to a dict, list, set or OrderedDict and that the source
    itself mutates: an assignment (or ``del``) through a subscript, or a call of clear / pop / setdefault / append /
    update.  A lookup table that is only read is not found."""
    tree = pyast.parse(source)

    def is_container(v):
        if isinstance(v, (pyast.Dict, pyast.List, pyast.Set, pyast.DictComp, pyast.ListComp, pyast.SetComp)):
            return True
        return isinstance(v, pyast.Call) and getattr(v.func, "id", getattr(v.func, "attr", "")) in CONTAINER_CALLS
    bound = set()
    for node in tree.body:
        if isinstance(node, pyast.Assign):
            pairs = []
            for t in node.targets:
                if isinstance(t, pyast.Name):
                    pairs.append((t, node.value))
                elif isinstance(t, pyast.Tuple) and isinstance(node.value, pyast.Tuple) and len(t.elts) == len(node.value.elts):
                    pairs.extend(zip(t.elts, node.value.elts))
        elif isinstance(node, pyast.AnnAssign) and node.value is not None:
            pairs = [(node.target, node.value)]
        else:
            continue
        bound.update(t.id for t, v in pairs if isinstance(t, pyast.Name) and is_container(v))
    found = set()
    for node in pyast.walk(tree):
        if isinstance(node, (pyast.Assign, pyast.AugAssign, pyast.Delete)):
            targets = [node.target] if isinstance(node, pyast.AugAssign) else node.targets
            for t in targets:
                for sub in pyast.walk(t):
                    if isinstance(sub, pyast.Subscript) and isinstance(sub.value, pyast.Name) and sub.value.id in bound:
                        found.add(sub.value.id)
        elif isinstance(node, pyast.Call) and isinstance(node.func, pyast.Attribute) and node.func.attr in MUTATORS \
                and isinstance(node.func.value, pyast.Name) and node.func.value.id in bound:
            found.add(node.func.value.id)
    return found


def test_the_python_scan_sees_what_it_is_for():
    src = ("import collections\nTABLE = {1: 2}\n_a, _b = {}, []\n_c = collections.OrderedDict()\n_d: dict = {}\n_e = set()\n"
           "_f = {}\nN = 3\n"
           "def f(k):\n    _a[k] = TABLE[k]\n    _b.append(k)\n    _c.pop(k, None)\n    del _d[k]\n    return _f.get(k), _e\n")
    assert mutated_module_containers(src) == {"_a", "_b", "_c", "_d"}


def test_every_mutated_module_level_container_is_registered():
    have = {(h.where, h.name) for h in so.HIDDEN_STATE}
    missing, seen = [], 0
    for path in sorted(PACKAGE.rglob("*.py")):
        where = path.relative_to(PACKAGE).as_posix()
        for name in sorted(mutated_module_containers(path.read_text())):
            seen += 1
            if (where, name) not in have:
                missing.append(f"{where}: {name}")
    assert seen >= 6, "the scan found less than device.py and lensing.py are known to hold"
    assert not missing, f"module-level state without an entry in stream_order.HIDDEN_STATE: {missing}"


C_COMMENT = re.compile(r"//[^\n]*|/\*.*?\*/", re.S)
C_GLOBAL = re.compile(r"\bg_\w+\b")
C_LOCAL_STATIC = re.compile(r"^[ \t]+(?:thread_local[ \t]+)?static[ \t]+(?!const\b|constexpr\b)(?:thread_local[ \t]+)?"
                            r"[\w:<>,\*& \t]+?[ \t\*&](\w+)[ \t]*(?:\[[^\]\n]*\])*[ \t]*(?:;|=|\{)", re.M)


def c_state_names(text):
    """Names of the objects of a HIP source that outlive a call: everything called g_*, and every function-local
    ``static`` object that is not const / constexpr (a static member FUNCTION has a parenthesis after its name)."""
    code = C_COMMENT.sub("", text)
    return set(C_GLOBAL.findall(code)) | set(C_LOCAL_STATIC.findall(code))


def test_the_c_scan_sees_what_it_is_for():
    text = ("struct A { int x; } g_a;   // g_comment\nstatic thread_local char g_err[8] = \"\";\n"
            "int f() {\n    static std::mutex mu;\n    static SidePipe pipes[64];\n    static const int depth = 3;\n"
            "    static constexpr int K = 2;\n    static ast::PerDeviceOnce attr_once;\n    return 0;\n}\n"
            "struct S {\n    static int or_default(int v, int d) { return v; }\n    static constexpr size_t per = 4;\n};\n")
    assert c_state_names(text) == {"g_a", "g_err", "mu", "pipes", "attr_once"}


def _c_sources():
    files = sorted((PACKAGE / "csrc").glob("*.hip")) + sorted((PACKAGE / "csrc").glob("*.h"))
    assert len(files) > 20
    return files


def test_every_c_object_that_outlives_a_call_is_registered():
    have = {(h.where, h.name) for h in so.HIDDEN_STATE}
    missing, seen = [], set()
    for path in _c_sources():
        where = path.relative_to(PACKAGE).as_posix()
        for name in sorted(c_state_names(path.read_text())):
            seen.add(name)
            if (where, name) not in have:
                missing.append(f"{where}: {name}")
    assert {"g_tw", "g_edge", "g_side", "pipes", "attr_once", "g_err"} <= seen
    assert not missing, f"file-scope or static state without an entry in stream_order.HIDDEN_STATE: {missing}"
    # ... and the table cannot rot: every entry's name still occurs in the file it names
    keys = [(h.where, h.name) for h in so.HIDDEN_STATE]
    assert len(set(keys)) == len(keys)
    for h in so.HIDDEN_STATE:
        path = PACKAGE / h.where
        assert path.is_file(), f"{h.where} (entry {h.name}) does not exist"
        text = path.read_text()
        names = c_state_names(text) if h.where.startswith("csrc/") else mutated_module_containers(text)
        assert h.name in names, f"{h.where} no longer holds {h.name}"


def _function_source(where, name):
    import importlib
    module = importlib.import_module("astrild_amd." + where[:-3].replace("/", "."))
    return inspect.getsource(getattr(module, name))


def _c_struct_get(text, struct):
    """The body of ``struct <name> { ... get(...) { ... } }`` from the ``get`` on, up to the closing ``} g_...;``."""
    m = re.search(r"\bstruct\s+" + re.escape(struct) + r"\s*\{", text)
    assert m, f"struct {struct} not found"
    body = text[m.end():]
    end = re.search(r"^\}\s*g_\w+;", body, re.M)
    assert end, f"struct {struct} does not end in an object called g_*"
    body = body[:end.start()]
    g = re.search(r"\bget\s*\(", body)
    assert g, f"struct {struct} has no get()"
    return body[g.start():]


HAND_OVER = {"event": re.compile(r"\.wait_event\("), "per_stream": re.compile(r"\bstream_key\(\)")}
C_COMPLETE = re.compile(r"\bhipMemcpy\(|\bhipStreamSynchronize\(")


def test_every_entry_says_how_it_is_handed_over_and_the_source_agrees():
    for h in so.HIDDEN_STATE:
        assert h.kind in so.KINDS, (h.name, h.kind)
        assert len(h.holds) > 10, h.name
        assert (h.clear is None) == bool(h.no_clear), f"{h.name}: a clear(), or the reason there is none"
        python = not h.where.startswith("csrc/")
        if python and h.kind in HAND_OVER:
            assert h.filled_by, f"{h.name}: which function fills it?"
            src = _function_source(h.where, h.filled_by)
            assert re.search(r"\b" + re.escape(h.name) + r"\b", src), f"{h.filled_by} does not touch {h.name}"
            assert HAND_OVER[h.kind].search(src), f"{h.where}: {h.filled_by} fills {h.name} ({h.kind}) without the hand-over"
        if python:
            assert h.clear is not None, f"{h.name}: a Python cache can be swapped for an empty one"
        if not python and h.kind == "built_synchronously":
            text = C_COMMENT.sub("", (PACKAGE / h.where).read_text())
            get = _c_struct_get(text, h.filled_by)
            done, published = C_COMPLETE.search(get), get.rfind("push_back(")
            assert published >= 0, f"{h.where}: {h.filled_by}::get publishes nothing"
            assert done and done.start() < published, \
                f"{h.where}: {h.filled_by}::get caches {h.name} before hipMemcpy / hipStreamSynchronize completed it"
            assert re.search(r"^\}\s*" + re.escape(h.name) + r";", text[text.index("struct " + h.filled_by):], re.M)


def test_the_kind_check_has_power():
    """Planted: a get() that publishes before it waits, and a filler without its hand-over."""
    good = "struct T {\n  int* get(int n) {\n    k<<<1, 1, 0, s>>>(d);\n    hipStreamSynchronize(s);\n    tabs.push_back(d);\n  }\n} g_t;\n"
    bad = good.replace("    hipStreamSynchronize(s);\n    tabs.push_back(d);\n", "    tabs.push_back(d);\n    hipStreamSynchronize(s);\n")
    for text, ok in ((good, True), (bad, False)):
        get = _c_struct_get(text, "T")
        done = C_COMPLETE.search(get)
        assert (done is not None and done.start() < get.rfind("push_back(")) == ok
    assert HAND_OVER["event"].search("cur.wait_event(hit[2])") and not HAND_OVER["event"].search("hit = _geom_cache.get(key)")
    assert HAND_OVER["per_stream"].search("key = (*stream_key(), n)") and not HAND_OVER["per_stream"].search("key = (dev, n)")


def test_a_case_shares_its_outputs_only_by_the_words_of_a_docstring():
    for c in so.CASES:
        if not c.shares:
            assert not c.shares_doc, c.name
            continue
        doc = " ".join((inspect.getdoc(_resolve(c.shares_doc)) or "").split())
        reason = " ".join(c.shares.split())
        assert len(reason) > 20 and reason in doc, f"{c.name}: {c.shares_doc}'s docstring does not say: {reason}"
        assert re.search(r"\b(shared|owned by)\b", reason), f"{c.name}: the sentence does not say shared or owned by a plan"
        assert "." in c.shares_doc, f"{c.name}: only an explicit plan object's method may share its result"
    # the geometry leaves are declared only where the comparison is bitwise (elsewhere the case's tolerance covers them)
    assert all(c.compare == "equal" for c in so.CASES if c.geometry_leaves)
