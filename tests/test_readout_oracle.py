"""CPU: the readout oracle (tests/readout_oracle.py) against the paint oracle it is the adjoint of, and the host-side
argument checks of astrild_amd.particles.hutils.readout.  No GPU work."""
import importlib

import numpy as np
import pytest

from oracle import mesh as omesh
from tests import readout_oracle as orc

pytest.importorskip("torch")
# (the package exports the function ``readout`` under the module's own name: the module itself comes from importlib)
ro = importlib.import_module("astrild_amd.particles.hutils.readout")

L = 100.0
WINDOWS = ("ngp", "cic", "tsc")


def renormalised_readout(field, pos, boxsize, window):
    """The field at ``pos`` with the weights of oracle.mesh.window_1d (float64, renormalised by their sum)."""
    n = field.shape[0]
    f4 = field.reshape(n, n, n, -1).astype(np.float64)
    ax = [omesh.window_1d(np.asarray(pos[:, d], dtype=np.float64) * (n / float(boxsize)), window) for d in range(3)]
    out = np.zeros((len(pos), f4.shape[3]))
    support = ax[0][1].shape[0]
    for a in range(support):
        for b in range(support):
            for c in range(support):
                w = ax[0][1][a] * ax[1][1][b] * ax[2][1][c]
                out += w[:, None] * f4[np.mod(ax[0][0] + a, n), np.mod(ax[1][0] + b, n), np.mod(ax[2][0] + c, n)]
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n", [5, 8])
def test_against_the_renormalised_weights(n, window, dtype):
    """|contract - renormalised| <= 16 eps_R A: at most 3 roundings per weight on 3 axes (9), 2 ulp of renormalisation
    per axis (6) and the final cast (1).  Largest ratio on these inputs: 6.2 eps_R A (CIC, float32, n = 5)."""
    field = orc.field(n, 3, dtype, seed=n)
    pos = orc.positions(n, L, 2000, seed=7 * n)
    got, A = orc.readout(field, pos, L, window)
    ref = renormalised_readout(field, pos, L, window)
    eps = np.finfo(dtype).eps
    assert got.dtype == np.dtype(dtype) and got.shape == (len(pos), 3)
    ratio = np.abs(got.astype(np.float64) - ref) / (eps * A)
    print(f"READOUT_ORACLE n={n} {window} {np.dtype(dtype).name}: max |diff| / (eps A) = {ratio.max():.2f}")
    assert np.all(np.abs(got.astype(np.float64) - ref) <= 16 * eps * A)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n", [5, 8])
def test_adjoint_of_the_oracle_paint(n, window):
    """sum paint(m, pos) f = sum m readout(f, pos) within (k_max + 16) eps sum_p |m_p| A_p: 16 eps A_p per read-out
    value as above, and the k_max - 1 additions into the fullest cell on the paint's side."""
    rng = np.random.default_rng(n)
    pos = orc.positions(n, L, 500, seed=3 * n)
    mass = rng.uniform(-1.0, 2.0, size=len(pos))
    field = orc.field(n, 0, np.float64, seed=n + 1)
    val, A = orc.readout(field, pos, L, window)
    idx, _, finite = orc.stencil(pos, n, L, window, 0.0, np.float64)
    assert finite.all()
    W = idx[0].shape[0]
    flat = np.concatenate([((idx[0][a] * n + idx[1][b]) * n + idx[2][c]) for a in range(W) for b in range(W) for c in range(W)])
    k_max = int(np.bincount(flat, minlength=n ** 3).max())
    lhs = float(np.sum(omesh.paint(pos, mass, n, L, window) * field))
    rhs = float(np.sum(mass * val))
    bound = (k_max + 16) * np.finfo(np.float64).eps * float(np.sum(np.abs(mass) * A))
    print(f"READOUT_ORACLE adjoint n={n} {window}: k_max={k_max} |lhs - rhs| / bound = {abs(lhs - rhs) / bound:.3f}")
    assert abs(lhs - rhs) <= bound


def test_sparse_table_gives_the_dense_result():
    n = 6
    field = orc.field(n, 2, np.float32, seed=3)
    pos = orc.positions(n, L, 50, seed=4)
    cells = {(i, j, k): field[i, j, k] for i in range(n) for j in range(n) for k in range(n)}
    for window in WINDOWS:
        dense, A = orc.readout(field, pos, L, window)
        sparse, As, touched = orc.readout_sparse(cells, n, 2, np.float32, pos, L, window)
        assert dense.tobytes() == sparse.tobytes() and np.array_equal(A, As) and touched <= set(cells)


def test_non_finite_coordinates_give_nan():
    n = 4
    field = orc.field(n, 0, np.float64, seed=1)
    pos = np.full((4, 3), 10.0)
    pos[0, 0], pos[1, 1], pos[2, 2] = np.nan, np.inf, -np.inf
    for window in WINDOWS:
        out, _ = orc.readout(field, pos, L, window)
        assert np.isnan(out[:3]).all() and np.isfinite(out[3])


# ------------------------------------------------------------------ argument checks
GOOD = dict(field_shape=(8, 8, 8), field_dtype=np.float32, pos_shape=(10, 3), pos_dtype=np.float64, boxsize=L)


def test_check_accepts_the_valid_shapes():
    import torch
    assert ro.check_readout_args(**GOOD) == (8, 1, 1, L, 0.0)
    for c in (1, 2, 3, 4):
        assert ro.check_readout_args(**{**GOOD, "field_shape": (5, 5, 5, c)})[:2] == (5, c)
    assert ro.check_readout_args(**{**GOOD, "field_shape": (1, 1, 1), "pos_shape": (0, 3)})[0] == 1
    assert ro.check_readout_args(**{**GOOD, "field_dtype": torch.float64, "pos_dtype": torch.float32})[0] == 8
    assert ro.check_readout_args(**{**GOOD, "field_dtype": "float64", "pos_dtype": np.dtype("<f4")})[0] == 8
    for name, code in (("ngp", 0), ("NGP", 0), ("nearest", 0), ("nnb", 0), ("CiC", 1), ("tsc", 2), ("TSC", 2)):
        assert ro.check_readout_args(**GOOD, resampler=name)[2] == code
    assert ro.check_readout_args(**GOOD, shift=0.5)[4] == 0.5


@pytest.mark.parametrize("change, error, says", [
    (dict(field_shape=(8, 8)), ValueError, "(8, 8)"),
    (dict(field_shape=(8, 8, 7)), ValueError, "(8, 8, 7)"),
    (dict(field_shape=(8, 7, 8, 3)), ValueError, "(8, 7, 8, 3)"),
    (dict(field_shape=(0, 0, 0)), ValueError, "(0, 0, 0)"),
    (dict(field_shape=(8, 8, 8, 5)), ValueError, "5"),
    (dict(field_shape=(8, 8, 8, 0)), ValueError, "0"),
    (dict(field_shape=(8, 8, 8, 3, 1)), ValueError, "(8, 8, 8, 3, 1)"),
    (dict(pos_shape=(10,)), ValueError, "(10,)"),
    (dict(pos_shape=(10, 2)), ValueError, "(10, 2)"),
    (dict(pos_shape=(3, 10)), ValueError, "(3, 10)"),
    (dict(field_dtype=np.float16), TypeError, "float16"),
    (dict(field_dtype=np.int32), TypeError, "int32"),
    (dict(pos_dtype=np.int64), TypeError, "int64"),
    (dict(pos_dtype=np.complex64), TypeError, "complex64"),
    (dict(resampler="pcs"), ValueError, "'pcs'"),
    (dict(resampler=None), ValueError, "None"),
    (dict(resampler=2), ValueError, "2"),
    (dict(boxsize=0.0), ValueError, "0.0"),
    (dict(boxsize=-1.0), ValueError, "-1.0"),
    (dict(boxsize=float("inf")), ValueError, "inf"),
    (dict(boxsize=float("nan")), ValueError, "nan"),
    (dict(boxsize=None), ValueError, "None"),
    (dict(boxsize="100"), ValueError, "'100'"),
    (dict(shift=float("nan")), ValueError, "nan"),
    (dict(shift=float("inf")), ValueError, "inf"),
])
def test_check_refuses_by_name(change, error, says):
    with pytest.raises(error) as e:
        ro.check_readout_args(**{**GOOD, **change})
    assert says in str(e.value)


def test_check_refuses_torch_dtypes_by_name():
    import torch
    with pytest.raises(TypeError, match="float16"):
        ro.check_readout_args(**{**GOOD, "field_dtype": torch.float16})
    with pytest.raises(TypeError, match="int32"):
        ro.check_readout_args(**{**GOOD, "pos_dtype": torch.int32})


# ------------------------------------------------------------------ the C entry's own checks (host only: no launch)
def test_entry_refuses_bad_arguments_and_accepts_no_particles(hip):
    import ctypes as ct
    from astrild_amd import _lib
    buf = (ct.c_double * 8)()
    p = ct.cast(buf, ct.c_void_p)
    ok = dict(window=1, fdt=_lib.F32, pdt=_lib.F64, field=p, n=8, c=3, pos=p, np_=0, box=L, shift=0.0, out=p)

    def call(**kw):
        a = {**ok, **kw}
        return hip.ast_readout(a["window"], a["fdt"], a["pdt"], a["field"], a["n"], a["c"], a["pos"], a["np_"], a["box"],
                               a["shift"], a["out"], None)
    assert call() == 0                                            # np == 0: AST_OK, nothing is launched
    assert call(field=None, pos=None, out=None) == 0              # ... and no pointer is looked at
    for bad in (dict(window=3), dict(window=-1), dict(fdt=2), dict(pdt=-1), dict(n=0), dict(n=-4), dict(c=0), dict(c=5),
                dict(n=2 ** 31 - 1, c=4), dict(box=0.0), dict(box=-1.0), dict(box=float("inf")), dict(box=float("nan")),
                dict(shift=float("nan")), dict(shift=float("-inf")),
                dict(np_=1, field=None), dict(np_=1, pos=None), dict(np_=1, out=None)):
        assert call(**bad) == -1, bad                             # AST_ERR_ARG
        assert b"ast_readout: bad argument" in hip.ast_last_error()
