"""numpy restatement of ``FFTPower(mode="2d", Nmu, los, poles)`` on the half spectrum, with the rules astrild_amd fixes
for it (include/astrild_hip.h, ast_power_bin_2d):

* lattice, k shell, dropped modes (DC, |m| >= n/2), Hermitian weight (2 for 0 < i2 < n/2, else 1) and ``binning`` are
  those of ``oracle.fftpower.project_1d``; ``binning`` only touches the k shell;
* mu = |m_los| / |m| folded onto [0, 1]; Nmu uniform left-closed bins, mu = 1 in the last; membership in exact integer
  arithmetic, ``j = min(Nmu - 1, max{j : j^2 |m|^2 <= Nmu^2 m_los^2})``;
* wedges: sums of w|k|, w mu, w P and w per (shell, mu bin); multipoles: sums of w P L_l(mu) over ALL modes of the 1-D
  shell, mu = m_los / sqrt(|m|^2) in float64, L_l from the three-term recurrence, ``P_l = (2l + 1) sum / sum w``.

``project_2d`` finds the mu bin with an integer square root; ``full_lattice_counts`` walks the FULL lattice without
Hermitian weights and compares ``a^2 Nmu^2`` against ``j^2 |m|^2`` bin by bin - it shares no index formula with it."""
import numpy as np

from oracle import fftpower as offt


def legendre(l, mu):
    """L_l(mu) by (k + 1) L_{k+1} = (2k + 1) mu L_k - k L_{k-1}."""
    mu = np.asarray(mu, dtype=np.float64)
    prev, cur = np.ones_like(mu), mu.copy()
    if l == 0:
        return prev
    for k in range(1, l):
        prev, cur = cur, ((2 * k + 1) * mu * cur - k * prev) / (k + 1)
    return cur


def mu_bin_index(m2, a, Nmu):
    """max{j : j^2 m2 <= Nmu^2 a^2} capped at Nmu - 1, for int64 arrays m2 > 0 and a >= 0: j = floor(sqrt(q)) with
    q = floor(Nmu^2 a^2 / m2) (j^2 <= Nmu^2 a^2 / m2 <=> j^2 <= q for integer j)."""
    q = (np.int64(Nmu) * Nmu * a * a) // m2
    return np.minimum(offt.isqrt_array(q), Nmu - 1)


_block_cache = {}


def _block(n, boxsize, los, binning, i0, i1):
    """(|m|^2, w, |m_los|, shell) of a block's modes; the last few are kept (auto and cross, or several sets of poles,
    share them; the callers do not modify them)."""
    i0 = (0, n) if i0 is None else tuple(i0)
    i1 = (0, n) if i1 is None else tuple(i1)
    key = (n, float(boxsize), los, binning or offt.DEFAULT_BINNING, i0, i1)
    if key not in _block_cache:
        while len(_block_cache) >= 4:
            _block_cache.pop(next(iter(_block_cache)))
        _block_cache[key] = _block_uncached(n, boxsize, los, binning, i0, i1)
    return _block_cache[key]


def _block_uncached(n, boxsize, los, binning, i0, i1):
    f = offt._freq_int(n)
    m0 = f[i0[0]:i0[0] + i0[1]]
    m1 = f[i1[0]:i1[0] + i1[1]]
    mz = np.arange(n // 2 + 1)
    shape = (len(m0), len(m1), len(mz))
    m2 = (m0[:, None, None] ** 2 + m1[None, :, None] ** 2 + mz[None, None, :] ** 2).astype(np.int64)
    w = np.broadcast_to(np.where((mz > 0) & (mz < n // 2), 2, 1)[None, None, :], shape)
    a = np.broadcast_to(np.abs((m0[:, None, None], m1[None, :, None], mz[None, None, :])[los]), shape).astype(np.int64)
    sh = offt.shell_index(m0, m1, mz, m2, n, boxsize, binning)
    return m2, w, a, sh


def project_2d(p3d_half, n, boxsize, Nmu, los, poles=(0, 2, 4), binning=None, i0=None, i1=None):
    """Raw sums of a block ``(i0 count, i1 count, n//2+1)`` of P3D values (real; None: geometry only):
    dict(ksum, musum, psum, modes: (n//2-1, Nmu); polesum: (len(poles), n//2-1), without 2l + 1)."""
    nb = n // 2 - 1
    kf = 2.0 * np.pi / boxsize
    m2, w, a, sh = _block(n, boxsize, los, binning, i0, i1)
    ok = (sh >= 0) & (sh < nb)
    m2, w, a, sh = m2[ok], w[ok].astype(np.float64), a[ok], sh[ok]
    norm = np.sqrt(m2.astype(np.float64))
    mu = a.astype(np.float64) / norm
    cell = sh * Nmu + mu_bin_index(m2, a, Nmu)
    hist = lambda idx, weights, size: np.bincount(idx, weights=weights, minlength=size)
    out = {"ksum": hist(cell, w * kf * norm, nb * Nmu).reshape(nb, Nmu),
           "musum": hist(cell, w * mu, nb * Nmu).reshape(nb, Nmu),
           "modes": hist(cell, w, nb * Nmu).astype(np.int64).reshape(nb, Nmu)}
    if p3d_half is not None:
        p = np.asarray(p3d_half).real[ok]
        out["psum"] = hist(cell, w * p, nb * Nmu).reshape(nb, Nmu)
        out["abs_psum"] = hist(cell, w * np.abs(p), nb * Nmu).reshape(nb, Nmu)     # the size of the sums, for tolerances
        out["polesum"] = np.stack([hist(sh, w * p * legendre(l, mu), nb) for l in poles]).reshape(len(poles), nb)
    return out


def finish(sums, poles=(0, 2, 4), shotnoise=0.0):
    """The dict device.finish_power_2d returns, from project_2d's sums."""
    nm = sums["modes"]
    nm1 = nm.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        res = {"k": sums["ksum"] / nm, "mu": sums["musum"] / nm, "power": sums["psum"] / nm, "modes": nm,
               "shotnoise": shotnoise, "poles": {"k": sums["ksum"].sum(axis=1) / nm1, "modes": nm1}}
        for q, l in enumerate(poles):
            res["poles"]["power_%d" % l] = (2 * l + 1) * sums["polesum"][q] / nm1
    return res


def p3d(c1, c2, boxsize):
    """Re(c1 conj(c2)) L^3 of two half spectra (c2 None: auto)."""
    c1 = np.asarray(c1, dtype=np.complex128)
    c2 = c1 if c2 is None else np.asarray(c2, dtype=np.complex128)
    return (c1.real * c2.real + c1.imag * c2.imag) * float(boxsize) ** 3


def full_lattice_counts(n, Nmu, los):
    """Modes per (shell, mu bin) over the FULL lattice (every index 0 .. n-1 of all three axes, no Hermitian weights),
    integer binning.  The mu bin is found by comparing a^2 Nmu^2 with j^2 |m|^2 for one j after the other."""
    nb = n // 2 - 1
    f = offt._freq_int(n).astype(np.int64)
    m = (f[:, None, None], f[None, :, None], f[None, None, :])
    m2 = m[0] ** 2 + m[1] ** 2 + m[2] ** 2
    a2 = np.broadcast_to(m[los] ** 2, m2.shape) * np.int64(Nmu) ** 2
    counts = np.zeros((nb, Nmu), dtype=np.int64)
    for s in range(nb):
        in_shell = (m2 >= (s + 1) ** 2) & (m2 < (s + 2) ** 2)
        for j in range(Nmu):
            lower = a2 >= np.int64(j) ** 2 * m2
            upper = (a2 < np.int64(j + 1) ** 2 * m2) if j < Nmu - 1 else np.ones_like(lower)
            counts[s, j] = np.count_nonzero(in_shell & lower & upper)
    return counts


def on_edge_modes(n, Nmu, los):
    """Kept lattice vectors (full lattice, integer binning) with 0 < mu < 1 exactly on a bin edge: j^2 |m|^2 = Nmu^2 a^2
    for some 0 < j < Nmu.  Returns (count, array of (m0, m1, m2, j))."""
    nb = n // 2 - 1
    f = offt._freq_int(n).astype(np.int64)
    g = np.stack(np.meshgrid(f, f, f, indexing="ij"), axis=-1).reshape(-1, 3)
    m2 = (g ** 2).sum(axis=1)
    keep = (m2 >= 1) & (m2 < (nb + 1) ** 2)
    g, m2 = g[keep], m2[keep]
    a2 = g[:, los] ** 2 * np.int64(Nmu) ** 2
    rows = []
    for j in range(1, Nmu):
        hit = a2 == np.int64(j) ** 2 * m2
        rows.append(np.concatenate([g[hit], np.full((hit.sum(), 1), j)], axis=1))
    rows = np.concatenate(rows)
    return len(rows), rows
