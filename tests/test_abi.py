"""CPU-only: the C-ABI library loads and exports exactly what include/astrild_hip.h
declares, and the ctypes table in astrild_amd/_lib.py covers every declaration.
No compute calls (there is no GPU here)."""
import ctypes as ct
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "astrild_hip.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"^\s*(?:const\s+)?[A-Za-z_][A-Za-z0-9_\s\*]*?\b([a-z][A-Za-z0-9_]*)\s*\(", src, flags=re.M)
    return sorted({n for n in names if n.startswith("ast_") or n.startswith("kappa0_")})


def test_header_declares_the_expected_surface():
    names = declared_functions()
    for required in ("ast_paint", "ast_paint_tiled", "ast_ngp_assign", "ast_fft_exec", "ast_power_bin_1d",
                     "ast_kappa_stack", "ast_kappa_to_alphas", "kappa0_to_alphas", "kappa0_to_phi",
                     "ast_gaussian_smooth", "ast_histogram", "ast_shell_filter", "ast_slab_pack"):
        assert required in names


def test_library_exports_every_declared_symbol():
    from astrild_amd import _lib
    assert os.path.isfile(_lib.LIB_PATH), "build the HIP library first (__graft_entry__.build())"
    handle = ct.CDLL(_lib.LIB_PATH)
    for name in declared_functions():
        assert hasattr(handle, name), f"{name} is declared in the header but not exported"


def test_ctypes_table_matches_header():
    from astrild_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_functions()
    lib = _lib.lib()                      # sets argtypes/restype for all of them
    assert lib.ast_version() >= 100       # host-only call, no GPU needed


def test_paint_flag_and_stage_constants_match_header():
    """The AST_PAINT_* flag bits and AST_PAINT_STAGE_* codes of the header, under the same names without the prefix in _lib."""
    from astrild_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    defines = {name: int(value) for name, value in re.findall(r"^#define\s+AST_(PAINT_[A-Z_]+)\s+\(?(-?\d+)\)?\s*$", src, flags=re.M)}
    assert sorted(defines) == sorted(["PAINT_TWO_PASS", "PAINT_OVERWRITE", "PAINT_DEFER_FOLD", "PAINT_SCATTERED", "PAINT_XSORTED",
                                      "PAINT_STAGE_ALL", "PAINT_STAGE_GROUP", "PAINT_STAGE_WALK", "PAINT_STAGE_FOLD",
                                      "PAINT_STAGE_GROUP_PART", "PAINT_STAGE_RESET", "PAINT_STAGE_LATE"])
    for name, value in defines.items():
        assert getattr(_lib, name) == value, name
    assert sorted(n for n in vars(_lib) if n.startswith("PAINT_")) == sorted(defines)
    assert defines["PAINT_STAGE_ALL"] == -1 and defines["PAINT_XSORTED"] == 16


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "astrild_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f"{f} imports the oracle"


def test_missing_library_fails_loudly(monkeypatch):
    from astrild_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libastrild_hip.so")
    with pytest.raises(_lib.AstrildHipError):
        _lib.lib()


def test_no_gpu_means_error_not_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from astrild_amd import device, _lib
    with pytest.raises(_lib.AstrildHipError):
        device.device()


def test_order_probe_sample_stays_inside_the_particle_array():
    """device.sample_is_unordered reads 32 particles from each start: every start is a multiple of 32 and leaves room for
    its run at every particle count - in particular at 2^30, where a float32 linspace of the starts rounds past the end -
    and on CPU tensors the probe tells lattice order from shuffled order."""
    import numpy as np
    import torch
    from astrild_amd import device as dev
    for npart in (32, 33, 64, 65, 1000, 1 << 20, (1 << 30) - 1, 1 << 30, (1 << 30) + 31, (1 << 32) - 66):
        st = dev.sample_run_starts(npart)
        assert len(st) == 256 and st[0] == 0 and all(s % 32 == 0 or s == npart - 32 for s in st)
        assert all(0 <= s <= npart - 32 for s in st) and st == sorted(st)
    n, L = 64, 100.0
    ijk = np.stack(np.meshgrid(*(np.arange(n),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(3)
    nat = torch.from_numpy((((ijk + 0.5 + 0.5 * rng.standard_normal(ijk.shape)) * (L / n)) % L).astype(np.float32))
    assert not dev.sample_is_unordered(nat, n, L)
    assert dev.sample_is_unordered(nat[torch.from_numpy(rng.permutation(len(nat)))].contiguous(), n, L)


def test_scatter_probe_limit_stays_under_the_late_capacity():
    """device.paint takes the bucket scatter up to an estimated overflow of scatter_overflow_limit: for every particle count
    the tiled paint accepts (up to 2^32 - 66) and both dtypes that is below what the late list holds - the records
    {x, y, z, m} that fit the single pass's overflow list of npart x 4 bytes - and, at float32, never above npart / 5, the
    rule it replaced.  Host-only library calls."""
    import numpy as np
    import torch
    from astrild_amd import _lib, device as dev
    lib = _lib.lib()
    counts = {1 << 20, (1 << 20) + 1, (1 << 20) + 7, 3 * 2 ** 20 + 5, 1 << 21, 1 << 24, (1 << 30) - 1, 1 << 30, 1 << 31,
              (1 << 32) - 67, (1 << 32) - 66}
    counts |= {int(v) for v in np.geomspace(1 << 20, (1 << 32) - 66, 97)}
    counts |= {int(v) for v in np.random.default_rng(5).integers(1 << 20, (1 << 32) - 65, 200)}
    for dtype, esz in ((torch.float32, 4), (torch.float64, 8)):
        for npart in sorted(counts):
            cap = dev.scatter_late_capacity(dtype, npart)
            limit = dev.scatter_overflow_limit(dtype, npart)
            assert cap == int(lib.ast_paint_scatter_late_capacity(_lib.F32 if esz == 4 else _lib.F64, npart))
            assert cap * 4 * esz <= npart * 4 < (cap + 1) * 4 * esz, (dtype, npart, cap)
            assert 0 < limit < cap and limit >= cap * 4 // 5, (dtype, npart, limit, cap)
            if esz == 4:
                assert limit <= npart // 5
    assert lib.ast_paint_scatter_late_capacity(7, 1 << 20) == 0
