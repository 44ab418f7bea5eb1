"""Without a GPU: tests/ray_trace_oracle.py, whose bytes the device and the host build of csrc/ray_step.h must give,
against tests/ray_trace_reference.py - the same step and emit in np.longdouble, built field by field instead of ray by
ray.  A mistake made the same way in the kernel and in the oracle (a transposed node in one bilinear call, a sign of the
cross stencil, A12 for A21 in the coupling) passes every byte comparison; it does not pass this one, and the power test
shows that by making each such mistake in a restatement of the oracle."""
import math

import numpy as np
import pytest

from tests import ray_trace_cases as cases, ray_trace_oracle as orc, ray_trace_reference as ref

pytestmark = pytest.mark.skipif(np.finfo(np.longdouble).eps > 2.0 ** -63,
                                reason="np.longdouble is no wider than float64 here: it cannot referee float64 roundings")

EPS = float(np.finfo(np.float64).eps)          # the oracle's rounding; the reference's own is 2^-11 of it
K = 32                                         # 4 x the measured 4.48, rounded up to a power of two (test_agreement)
H = math.radians(2.0) / 16                     # no power of two: d / h rounds
CHI_PREV, CHI_K, CHI_S = 733.1, 1711.3, 2950.7
SHAPES = [(16, 16), (8, 16), (65, 65), (67, 134)]
CHANGED = (2, 3, 8, 9, 10, 11)                 # the planes that the deflection changes: s and B
ADVANCED = (0, 1, 4, 5, 6, 7)                  # d and A: two products, a sum and a quotient


def inputs(npix, m):
    return cases.random_psi(m, H, 400 + m), cases.reference_state(npix, m, H, 500 + npix)


_reference = {}


def reference(npix, m, born):
    """The longdouble step of one shape and mode, computed once and left unchanged."""
    key = (npix, m, bool(born))
    if key not in _reference:
        out, M = ref.step(*inputs(npix, m), H, CHI_PREV, CHI_K, born)
        out.setflags(write=False)
        _reference[key] = (out, M)
    return _reference[key]


def ratios(got, npix, m, born):
    """Per changed plane, |got - reference| / (eps M) over the rays."""
    want, M = reference(npix, m, born)
    return {q: (np.abs(got[q] - want[q]) / (EPS * M[q])).astype(np.float64) for q in CHANGED}


def test_agreement():
    """Largest |oracle - reference| / (eps M) over the four shapes and both modes: measured 4.48 (plane s2 of (65, 65),
    full mode, a ray 195 pixels out; the other shapes and the Born mode stay under 1.6), eps = 2^-52.  M bounds the
    terms, not the order of their roundings, hence K = 4 x 4.48 rounded up to a power of two = 32; the longest chain of
    the contract has about 16 roundings, so a K beyond 64 would not be a bound on rounding any more.  d and A, which
    are two products, a sum and a quotient of the inputs, agree to under 1 eps of the plane's largest value (0.88)."""
    worst = 0.0
    for npix, m in SHAPES:
        psi, st = inputs(npix, m)
        for born in (False, True):
            got = orc.step(psi, st, H, CHI_PREV, CHI_K, born)
            r = {q: float(v.max()) for q, v in ratios(got, npix, m, born).items()}
            want = reference(npix, m, born)[0]
            adv = max(float(np.abs(got[q] - want[q]).max() / (EPS * np.abs(want[q]).max())) for q in ADVANCED)
            print(f"npix {npix} m {m} {'born' if born else 'full'}: |oracle - reference| / (eps M) per plane "
                  f"{ {q: round(v, 3) for q, v in r.items()} }, d and A {adv:.3f} eps of the plane's maximum")
            worst = max(worst, *r.values())
            assert adv < 1.0
    print(f"largest ratio {worst:.3f}, K = {K}")
    assert K <= 64
    assert worst <= K


# ------------------------------------------------------------------ power: single mistakes in a restatement of the oracle
BILINEAR_CALLS = ("al1", "al2", "U11", "U22", "U12")
MUTATIONS = ([f"swap w10 and w01 in {c}" for c in BILINEAR_CALLS] + [f"flip sign {k} of the u12 stencil" for k in range(4)]
             + ["U12 A12 for U12 A21 in B11", "rows a - 1 and a + 1 exchanged in a1"])


def restated_step(psi, st, h, chi_prev, chi_k, born=False, mutation=None):
    """``orc.step`` once more, operation for operation (``mutation=None`` gives its bytes: asserted), with one switch per
    mistake."""
    assert mutation is None or mutation in MUTATIONS
    psi = np.asarray(psi, dtype=np.float64)
    m, npix = psi.shape[0], st.shape[1]
    v = [np.array(p, dtype=np.float64) for p in st]
    dchi = chi_k - chi_prev
    d1, d2 = (chi_prev * v[0] + dchi * v[2]) / chi_k, (chi_prev * v[1] + dchi * v[3]) / chi_k
    A11, A12 = (chi_prev * v[4] + dchi * v[8]) / chi_k, (chi_prev * v[5] + dchi * v[9]) / chi_k
    A21, A22 = (chi_prev * v[6] + dchi * v[10]) / chi_k, (chi_prev * v[7] + dchi * v[11]) / chi_k
    i = np.arange(npix, dtype=np.float64)[:, None] + np.zeros((npix, npix))
    j = np.arange(npix, dtype=np.float64)[None, :] + np.zeros((npix, npix))
    p1, p2 = (i, j) if born else (i + d1 / h, j + d2 / h)
    f1, f2 = np.floor(p1), np.floor(p2)
    fx, fy = p1 - f1, p2 - f2
    a = np.mod(np.clip(f1, -orc.INDEX_CLAMP, orc.INDEX_CLAMP).astype(np.int64), m)
    b = np.mod(np.clip(f2, -orc.INDEX_CLAMP, orc.INDEX_CLAMP).astype(np.int64), m)

    def at(da, db):
        return psi[np.mod(a + da, m), np.mod(b + db, m)]
    sign = [-1.0 if mutation == f"flip sign {k} of the u12 stencil" else 1.0 for k in range(4)]
    lo, hi = (1, -1) if mutation == "rows a - 1 and a + 1 exchanged in a1" else (-1, 1)
    h2, hh = 2.0 * h, h * h
    hh4 = 4.0 * hh
    a1, a2, u11, u22, u12 = ([[None, None], [None, None]] for _ in range(5))
    for x in range(2):
        for y in range(2):
            a1[x][y] = (at(x + hi, y) - at(x + lo, y)) / h2
            a2[x][y] = (at(x, y + 1) - at(x, y - 1)) / h2
            u11[x][y] = ((at(x + 1, y) - 2.0 * at(x, y)) + at(x - 1, y)) / hh
            u22[x][y] = ((at(x, y + 1) - 2.0 * at(x, y)) + at(x, y - 1)) / hh
            u12[x][y] = (((sign[0] * at(x + 1, y + 1) - sign[1] * at(x + 1, y - 1)) - sign[2] * at(x - 1, y + 1))
                         + sign[3] * at(x - 1, y - 1)) / hh4
    w00, w10, w01, w11 = (1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy

    def bilinear(name, q):
        s10, s01 = (w01, w10) if mutation == f"swap w10 and w01 in {name}" else (w10, w01)
        return ((w00 * q[0][0] + s10 * q[1][0]) + s01 * q[0][1]) + w11 * q[1][1]
    al1, al2 = bilinear("al1", a1), bilinear("al2", a2)
    U11, U22, U12 = bilinear("U11", u11), bilinear("U22", u22), bilinear("U12", u12)
    out = np.empty_like(st, dtype=np.float64)
    out[0], out[1], out[2], out[3] = d1, d2, v[2] - al1, v[3] - al2
    out[4], out[5], out[6], out[7] = A11, A12, A21, A22
    if born:
        out[8], out[9], out[10], out[11] = v[8] - U11, v[9] - U12, v[10] - U12, v[11] - U22
    else:
        out[8] = v[8] - (U11 * (1.0 + A11) + U12 * (A12 if mutation == "U12 A12 for U12 A21 in B11" else A21))
        out[9] = v[9] - (U11 * A12 + U12 * (1.0 + A22))
        out[10] = v[10] - (U12 * (1.0 + A11) + U22 * A21)
        out[11] = v[11] - (U12 * A12 + U22 * (1.0 + A22))
    return out


@pytest.mark.parametrize("npix,m", SHAPES)
def test_power(npix, m):
    """Each single mistake misses the reference by more than 1000 K eps M on some ray: all of them in full mode; in Born
    mode, where the rays sit on the nodes (w10 = w01 = 0) and nothing couples, the stencil's signs and rows.  The inputs
    can tell the nodes apart: no ray has fx == fy, and the cross derivative differs from cell to cell."""
    psi, st = inputs(npix, m)
    p1, p2 = cases.landing(st, H, CHI_PREV, CHI_K)
    fx, fy = p1 - np.floor(p1), p2 - np.floor(p2)
    assert (fx != fy).all() and (fx != 0).all() and (fy != 0).all()
    H12 = np.asarray(ref.fields(psi, H)[0][4], dtype=np.float64)
    assert np.unique(H12).size == m * m and H12.std() > 0.1 * np.abs(H12).max()
    for born in (False, True):
        assert restated_step(psi, st, H, CHI_PREV, CHI_K, born).tobytes() == orc.step(psi, st, H, CHI_PREV, CHI_K, born).tobytes()
        for mutation in MUTATIONS:
            if born and ("B11" in mutation or "swap" in mutation):      # no coupling; w10 = w01 = 0 on the nodes
                continue
            r = ratios(restated_step(psi, st, H, CHI_PREV, CHI_K, born, mutation), npix, m, born)
            worst = max(float(v.max()) for v in r.values())
            print(f"npix {npix} m {m} {'born' if born else 'full'}: {mutation}: {worst:.3g} eps M")
            assert worst > 1000 * K, mutation


def test_emit():
    """The oracle's emit against the longdouble one, from the state after the step: within 4 eps of each map's largest
    value (measured: 0.3 .. 3.2, the largest for omega, a difference of two larger numbers)."""
    for npix, m in SHAPES:
        psi, st = inputs(npix, m)
        for born in (False, True):
            after = orc.step(psi, st, H, CHI_PREV, CHI_K, born)
            got, want = orc.emit(after, CHI_K, CHI_S), ref.emit(after, CHI_K, CHI_S)
            err = (np.abs(got - want).max(axis=(1, 2)) / (EPS * np.abs(want).max(axis=(1, 2)))).astype(np.float64)
            print(f"npix {npix} m {m} {'born' if born else 'full'}: emit off by {np.round(err, 3)} eps of each map's maximum")
            assert (err <= 4.0).all()
            # one switched pair of the emit shows at once: omega changes sign, gamma2 does not
            swapped = after.copy()
            swapped[[5, 6, 9, 10]] = after[[6, 5, 10, 9]]
            other = ref.emit(swapped, CHI_K, CHI_S)
            assert np.abs(got[3] - other[3]).max() > 1000 * 4 * EPS * np.abs(want[3]).max()
            assert (np.abs(got[2] - other[2]) <= 4 * EPS * np.abs(want[2]).max()).all()
