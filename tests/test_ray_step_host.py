"""The per-ray arithmetic of the ray tracer (astrild_amd/csrc/ray_step.h: ``step_ray``, ``emit_ray``) in a stand-alone
host program under AddressSanitizer and UBSan, float-cast-overflow included: tests/host/ray_step_test.cpp.  What it writes
is compared byte for byte with tests/ray_trace_oracle.py, so the C++ source that the kernels are built from is tied to
the oracle without a device, and every index it forms - for 1e300, Inf and NaN displacements too - is watched."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import ray_trace_cases as cases, ray_trace_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    rocm_clang = "/opt/rocm/lib/llvm/bin/clang++"              # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler: neither g++ / clang++ / c++ on PATH nor " + rocm_clang
    exe = tmp_path_factory.mktemp("ray_step_host") / "ray_step_test"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                    "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "astrild_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "ray_step_test.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def run(program, tmp_path, psi, st, h, chi_prev, chi_k, chi_s, born):
    """The program's state after the step and its six maps."""
    m, npix = psi.shape[0], st.shape[1]
    case, out = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(case, "wb") as f:
        f.write(np.array([m, npix, int(born)], dtype=np.int64).tobytes())
        f.write(np.array([h, chi_prev, chi_k, chi_s], dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(psi, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(st, dtype=np.float64).tobytes())
    res = subprocess.run([program, str(case), str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"{npix * npix} rays stepped and emitted" in res.stdout
    got = np.fromfile(out, dtype=np.float64)
    assert got.size == 18 * npix * npix
    return got[:12 * npix * npix].reshape(12, npix, npix), got[12 * npix * npix:].reshape(6, npix, npix)


def check_bytes(program, tmp_path, psi, st, h, chi_prev, chi_k, chi_s, born):
    state, maps = run(program, tmp_path, psi, st, h, chi_prev, chi_k, chi_s, born)
    want = orc.step(psi, st, h, chi_prev, chi_k, born)
    assert np.isfinite(want).all()
    assert state.tobytes() == want.tobytes()
    assert maps.tobytes() == orc.emit(want, chi_k, chi_s).tobytes()
    return want


@pytest.mark.parametrize("born", [0, 1], ids=["full", "born"])
@pytest.mark.parametrize("npix,m", [(16, 16), (8, 16)])
def test_preset_states(program, tmp_path, npix, m, born):
    h = cases.H
    psi, st = cases.random_psi(m, h, 5 + npix), cases.preset_state(npix, m, h, 11)
    p1, p2 = cases.landing(st, h, 512.0, 1024.0)
    assert (p1 < 0).any() and (p2 < 0).any() and (p1 >= m).any() and (p2 >= m).any()
    want = check_bytes(program, tmp_path, psi, st, h, 512.0, 1024.0, 1711.3, born)
    check_bytes(program, tmp_path, cases.random_psi(m, h, 6 + npix), want, h, 1024.0, 1711.3, 2950.7, born)


@pytest.mark.parametrize("born", [0, 1], ids=["full", "born"])
def test_wild_states_stay_inside_the_potential(program, tmp_path, born):
    """1e300, 2^31, 2^40 and +-(2^30 +- 1) pixels, Inf, NaN, -0.0, a subnormal: no report from the sanitizers (no
    conversion out of int's range, no read outside psi), the oracle's bytes wherever the input is finite, NaN where it
    is not."""
    m, h = 16, cases.H
    psi = cases.random_psi(m, h, 3)
    st, finite = cases.wild_state(h)
    assert not finite[6, :3].any() and finite.sum() == finite.size - 3
    p1, _ = cases.landing(np.where(np.isfinite(st), st, 0.0), h, 512.0, 1024.0)
    assert {2.0 ** 30 + 1, 2.0 ** 30 - 1, -(2.0 ** 30 + 1), -(2.0 ** 30 - 1)} <= set((p1[7] - 7.0).tolist())
    state, maps = run(program, tmp_path, psi, st, h, 512.0, 1024.0, 1711.3, born)
    want = orc.step(psi, np.where(np.isfinite(st), st, 0.0), h, 512.0, 1024.0, born)
    assert state[:, finite].tobytes() == want[:, finite].tobytes()
    assert maps[:, finite].tobytes() == orc.emit(want, 1024.0, 1711.3)[:, finite].tobytes()
    if not born:                                         # fy = Inf - Inf: the deflection along axis 2 is NaN
        assert np.isnan(state[3, 6, :3]).all()
    assert np.isnan(state[1, 6, 2]) and np.isinf(state[1, 6, :2]).all() and not np.isfinite(maps[5, 6, :3]).any()


@pytest.mark.parametrize("born", [0, 1], ids=["full", "born"])
def test_the_smallest_grids(program, tmp_path, born):
    """Every 1 <= npix <= m <= 4: the 4 x 4 stencil wraps onto itself (m = 2: rows a - 1 and a + 1 are one row)."""
    h = cases.H
    for npix, m in cases.TINY_SHAPES:
        psi, st = cases.random_psi(m, h, 70 + m), cases.tiny_state(npix, m, h, 80 + 4 * m + npix)
        p1, p2 = cases.landing(st, h, 512.0, 1024.0)
        assert p1[0, 0] == 2 * m and p2[0, 0] == -3 * m
        if npix > 1:
            assert np.abs(p1).max() > m and np.abs(p2).max() > m and p1.min() < 0 and p2.min() < 0
        want = check_bytes(program, tmp_path, psi, st, h, 512.0, 1024.0, 1711.3, born)
        check_bytes(program, tmp_path, cases.random_psi(m, h, 90 + m), want, h, 1024.0, 1711.3, 2950.7, born)


@pytest.mark.parametrize("born", [0, 1], ids=["full", "born"])
@pytest.mark.parametrize("npix,m", [(65, 65), (67, 134)])
def test_states_that_cover_every_workgroup(program, tmp_path, npix, m, born):
    h, chi = cases.H, cases.CHI
    st = cases.geometry_state(npix, m, h, chi[0], chi[1], 200 + npix)
    assert cases.landing_classes(*cases.landing(st, h, chi[0], chi[1]), m) == []
    want = check_bytes(program, tmp_path, cases.random_psi(m, h, 300 + m), st, h, chi[0], chi[1], chi[2], born)
    check_bytes(program, tmp_path, cases.random_psi(m, h, 301 + m), want, h, chi[1], chi[2], chi[3], born)
