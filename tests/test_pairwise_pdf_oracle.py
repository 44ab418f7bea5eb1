"""CPU: the numpy restatement of the pairwise-velocity histograms (tests/pairwise_pdf_oracle.py) against the recorded
results of the reference's mean_pv_z_sign (tests/golden/pairwise_pdf_known_answers.json), its chunking, and the
argument handling of device.pairwise_velocity_pdf, all without a GPU."""
import numpy as np
import numpy.testing as npt
import pytest

from tests import pairwise_pdf_oracle as orc


def oracle_of(case, **kw):
    args = dict(ffirst=case["ffirst"], ssecond=case["ssecond"])
    args.update(kw)
    return orc.pair_pdf(case["pos"], case["vel"], case["r"], case["dist_bin"], case["vel_bin"], "z_sign", **args)


def test_product_module_imports_without_a_gpu():
    from astrild_amd.particles.hutils import mean_pairwise_velocity as mod
    from astrild_amd.particles.hutils import mean_pv_radial, mean_pv_z_sign  # noqa: F401
    assert callable(mod.mean_pv_z_sign) and callable(mod.mean_pv_radial)


def test_oracle_reproduces_the_reference_catalogue():
    cat, _ = orc.load_golden()
    assert len(cat["pos"]) <= 200 and cat["r"] < cat["dist_bin"]
    ref = orc.dense(cat["entries"], cat["dist_bin"], cat["vel_bin"])
    got = oracle_of(cat)
    npt.assert_array_equal(got["hist"], ref)
    assert ref.sum() > 1000 and got["outside"] > 0
    # the catalogue does what it was mixed for: separations on bin edges, equal z, v12 on velocity-bin edges
    pos, vel = cat["pos"], cat["vel"]
    i, j = np.triu_indices(len(pos), 1)
    dr, dv = pos[j] - pos[i], vel[j] - vel[i]
    d = np.sqrt((dr[:, 0] * dr[:, 0] + dr[:, 1] * dr[:, 1]) + dr[:, 2] * dr[:, 2])
    seen = d <= np.float64(np.float32(cat["r"]))
    assert np.any(seen & (d == np.round(d)) & (d > 0))
    assert np.any(seen & (dr[:, 2] == 0))
    v12 = dv[:, 2] * np.sign(dr[:, 2])
    assert np.any(seen & (v12 == np.round(v12)) & (dr[:, 2] != 0))
    chunk = cat["chunk"]
    npt.assert_array_equal(oracle_of(cat, ffirst=chunk["ffirst"], ssecond=chunk["ssecond"])["hist"],
                           orc.dense(chunk["entries"], cat["dist_bin"], cat["vel_bin"]))


def test_oracle_reproduces_the_reference_edge_cases():
    _, edges = orc.load_golden()
    assert len(edges) >= 10
    for case in edges:
        got = oracle_of(case)
        npt.assert_array_equal(got["hist"], orc.dense(case["entries"], case["dist_bin"], case["vel_bin"]), case["note"])
        assert got["hist"].sum() + got["outside"] <= 1


@pytest.mark.parametrize("kind", ["z_sign", "radial"])
def test_chunks_sum_to_the_whole(kind):
    pos = orc.compact(400, seed=3)
    vel = orc.coherent_velocities(pos, 5)
    whole = orc.pair_pdf(pos, vel, 30.0, 9, 40, kind, dist_width=4.0)
    parts = [orc.pair_pdf(pos, vel, 30.0, 9, 40, kind, dist_width=4.0, ffirst=a, ssecond=b)
             for a, b in ((0, 1), (1, 130), (130, 130), (130, 399), (399, 400))]
    npt.assert_array_equal(sum(p["hist"] for p in parts), whole["hist"])
    assert sum(p["outside"] for p in parts) == whole["outside"] > 0
    npt.assert_array_equal(sum(p["count"] for p in parts), whole["count"])
    npt.assert_allclose(sum(p["s1"] for p in parts), whole["s1"], rtol=1e-12, atol=1e-9)
    assert whole["hist"].sum() + whole["outside"] > 10000


def test_coincident_pair_in_radial_goes_outside():
    pos = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.0, 2.0, 5.0]])
    vel = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 2.0], [0.0, 0.0, 4.0]])
    got = orc.pair_pdf(pos, vel, 4.0, 5, 10, "radial")
    assert got["outside"] == 1 and got["hist"].sum() == 2
    assert got["count"].tolist() == [0, 0, 2, 0, 0] and np.all(np.isfinite(got["s1"]))
    assert got["hist"][2, 5 + 3] == 1 and got["hist"][2, 5 + 2] == 1


def _no_library(monkeypatch):
    from astrild_amd import _lib

    def refuse():
        raise AssertionError("library call before the argument checks")

    monkeypatch.setattr(_lib, "lib", refuse)


@pytest.mark.parametrize("kwargs", [
    dict(pos=np.zeros((5, 2))),
    dict(pos=np.zeros(15)),
    dict(vel=np.zeros((4, 3))),
    dict(r=0.0), dict(r=-1.0), dict(r=np.inf), dict(r=np.nan), dict(r=1e-60),
    dict(dist_bin=0), dict(vel_bin=0), dict(vel_bin=-3),
    dict(dist_bin=1 << 11, vel_bin=(1 << 11) + 1),
    dict(dist_width=0.0), dict(dist_width=np.nan), dict(vel_width=-1.0), dict(vel_width=np.inf),
    dict(kind="transverse"),
    dict(ffirst=-1), dict(ffirst=3, ssecond=2), dict(ssecond=6), dict(ffirst=6),
    dict(dist_bin=481, vel_bin=4, moments=True),
    dict(r="wide"), dict(r=None), dict(dist_width=[1.0, 2.0]), dict(vel_width="1"),
    dict(ffirst=1.5), dict(ssecond=4.0), dict(ssecond="4"), dict(dist_bin=5.5), dict(vel_bin=10.0),
])
def test_value_errors_before_any_library_call(kwargs, monkeypatch):
    from astrild_amd import device as dev
    _no_library(monkeypatch)
    args = dict(pos=np.zeros((5, 3)), vel=np.zeros((5, 3)), r=4.0, dist_bin=5, vel_bin=10, kind="z_sign")
    args.update(kwargs)
    with pytest.raises(ValueError):
        dev.pairwise_velocity_pdf(**args)


def test_good_arguments_reach_the_library(monkeypatch):
    from astrild_amd import _lib, device as dev
    _no_library(monkeypatch)
    for kwargs in (dict(), dict(ffirst=5, ssecond=5), dict(ffirst=np.int64(1), ssecond=np.int32(4), r=np.float32(4)), dict(dist_bin=100, vel_bin=4096), dict(dist_bin=480, moments=True)):
        args = dict(pos=np.zeros((5, 3)), vel=np.zeros((5, 3)), r=4.0, dist_bin=5, vel_bin=10, kind="radial")
        args.update(kwargs)
        with pytest.raises(AssertionError, match="library call"):
            dev.pairwise_velocity_pdf(**args)
    assert _lib.PVPDF_MAX_BINS >= 1 << 22


def test_python_limits_match_the_library():
    """The limits that device.pairwise_velocity_pdf checks without a library call are the library's (host-only calls)."""
    import re
    import os
    from astrild_amd import _lib
    lib = _lib.lib()
    assert lib.ast_pairwise_pdf_max_bins() == _lib.PVPDF_MAX_BINS
    header = open(os.path.join(os.path.dirname(_lib._HERE), "include", "astrild_hip.h")).read()
    assert int(re.search(r"#define AST_PVPDF_MAX_MOMENT_ROWS (\d+)", header).group(1)) == _lib.PVPDF_MAX_MOMENT_ROWS
    assert [int(re.search(rf"#define AST_PVPDF_{k.upper()} (\d+)", header).group(1)) for k in ("z_sign", "radial")] == \
        [_lib.PVPDF_KIND["z_sign"], _lib.PVPDF_KIND["radial"]]
    assert lib.ast_pairwise_pdf_workspace_bytes(1000, 100, 4096, 0) > 0
    assert lib.ast_pairwise_pdf_workspace_bytes(1000, 480, 4, 1) > lib.ast_pairwise_pdf_workspace_bytes(1000, 480, 4, 0)
    assert lib.ast_pairwise_pdf_workspace_bytes(1000, 481, 4, 1) == 0
    assert lib.ast_pairwise_pdf_workspace_bytes(1000, 1 << 11, (1 << 11) + 1, 0) == 0
    assert 40 * 40 <= lib.ast_pairwise_pdf_lds_bins(40, 1) < lib.ast_pairwise_pdf_lds_bins(40, 0) < 40 * 4096
