"""numpy restatement of the two-sample pair counts of the two-point correlation function (device.tpcf_cross_counts,
astrild_amd.particles.hutils.tpcf with sample2 / randoms): every pair (i of a, j of b) with the arithmetic and the bins
of tests/tpcf_oracle.py (_setup / _bin, imported), the minimum image with a boxsize and plain separations without one.
cross_counts_brute visits all pairs in row chunks, cross_counts applies the same arithmetic to the candidate pairs of two
cKDTrees (fast at N ~ 10^5); auto_counts_open_brute is the open-boundary twin of tpcf_oracle.pair_counts_brute.  The five
estimators are written out here from the formulas, independently of the package."""
import numpy as np

from tests.tpcf_oracle import _bin, _setup


def _sep(x, y, boxsize):
    d = np.abs(x - y)
    return d if boxsize is None else np.minimum(d, float(boxsize) - d)


def cross_counts_brute(a, b, s_edges, mu_edges=None, los=2, boxsize=None, chunk=256):
    """Counts of all pairs (i of a, j of b), (ns, nmu) or (ns,) int64; fp64 positions (inside [0, boxsize] with one)."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
    s2, mu_e, nmu, counts = _setup(s_edges, mu_edges)
    if len(b):
        for i0 in range(0, len(a), chunk):
            _bin([_sep(a[i0:i0 + chunk, ax, None], b[None, :, ax], boxsize).ravel() for ax in range(3)], s2, mu_e, los,
                 counts)
    return counts.reshape(-1, nmu) if nmu else counts


def auto_counts_open_brute(pos, s_edges, mu_edges=None, los=2, chunk=256):
    """Unordered pairs i < j of one set with plain separations (no box)."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    s2, mu_e, nmu, counts = _setup(s_edges, mu_edges)
    n = len(pos)
    cols = np.arange(n)
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        upper = cols[None, i0:] > cols[i0:i1, None]
        _bin([np.abs(pos[i0:i1, ax, None] - pos[None, i0:, ax])[upper] for ax in range(3)], s2, mu_e, los, counts)
    return counts.reshape(-1, nmu) if nmu else counts


def cross_counts(a, b, s_edges, mu_edges=None, los=2, boxsize=None):
    """cross_counts_brute's counts from the candidate pairs of two cKDTrees (periodic with a boxsize) within the top edge
    plus a relative margin of 1e-6 and an absolute one for coordinates far from the origin."""
    from scipy.spatial import cKDTree
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
    s2, mu_e, nmu, counts = _setup(s_edges, mu_edges)
    if len(a) and len(b):
        if boxsize is None:
            ta, tb = cKDTree(a), cKDTree(b)
            amax = max(np.abs(a).max(), np.abs(b).max())
        else:
            top = np.nextafter(float(boxsize), 0.0)                      # cKDTree wants [0, L)
            ta, tb = cKDTree(np.minimum(a, top), boxsize=float(boxsize)), cKDTree(np.minimum(b, top), boxsize=float(boxsize))
            amax = float(boxsize)
        near = ta.query_ball_tree(tb, float(np.sqrt(s2[-1])) * (1.0 + 1e-6) + amax * 1e-12)
        i = np.repeat(np.arange(len(a)), [len(x) for x in near])
        j = np.fromiter((y for x in near for y in x), dtype=np.int64, count=len(i))
        for c0 in range(0, len(i), 1 << 22):
            ii, jj = i[c0:c0 + (1 << 22)], j[c0:c0 + (1 << 22)]
            _bin([_sep(a[ii, ax], b[jj, ax], boxsize) for ax in range(3)], s2, mu_e, los, counts)
    return counts.reshape(-1, nmu) if nmu else counts


def auto_counts(pos, s_edges, mu_edges=None, los=2, boxsize=None):
    """Unordered pairs of one set from the ordered cross counts with itself: the d = 0 self pairs are in no bin (as are
    coincident points), so every unordered pair is there twice."""
    c = cross_counts(pos, pos, s_edges, mu_edges, los, boxsize)
    assert not (c % 2).any()
    return c // 2


ESTIMATORS = ("Natural", "Davis-Peebles", "Hewett", "Hamilton", "Landy-Szalay")


def estimator_terms(name, dd, dr, rr, na, nb, nr):
    """The additive terms of the estimator, from ORDERED pair counts as fp64 arrays (dd: data-data, 2 x unordered for an
    auto term; dr: all data-random pairs; rr: 2 x unordered random pairs): xi is their sum, in this order."""
    dd, na, nb, nr = np.asarray(dd, dtype=np.float64), float(na), float(nb), float(nr)
    dr = None if dr is None else np.asarray(dr, dtype=np.float64)
    rr = None if rr is None else np.asarray(rr, dtype=np.float64)
    one = np.ones_like(dd)
    with np.errstate(divide="ignore", invalid="ignore"):
        if name == "Natural":
            return [nr * nr / (na * nb) * dd / rr, -one]
        if name == "Davis-Peebles":
            return [nr / nb * dd / dr, -one]
        if name == "Hewett":
            return [nr * nr / (na * nb) * dd / rr, -(nr / na * dr / rr)]
        if name == "Hamilton":
            return [dd * rr / (dr * dr), -one]
        if name == "Landy-Szalay":
            return [nr * nr / (na * nb) * dd / rr, -(nr / na * 2.0 * dr / rr), one]
    raise ValueError(name)


def estimator(name, dd, dr, rr, na, nb, nr):
    t = estimator_terms(name, dd, dr, rr, na, nb, nr)
    out = t[0]
    with np.errstate(invalid="ignore"):                                 # inf - inf in an empty RR bin
        for x in t[1:]:
            out = out + x
    return out


def analytic_cross_xi(d1d2, n1, n2, boxsize, s_edges, mu_edges=None):
    """D1D2 / (N1 N2 v / L^3) - 1, v = shell volume x dmu."""
    s = np.asarray(s_edges, dtype=np.float64)
    v = (4.0 * np.pi / 3.0) * (s[1:] ** 3 - s[:-1] ** 3)
    if mu_edges is not None:
        v = np.outer(v, np.diff(np.asarray(mu_edges, dtype=np.float64)))
    return np.asarray(d1d2, dtype=np.float64) / (float(n1) * float(n2) * v / float(boxsize) ** 3) - 1.0


def parity_lattice(m=8):
    """The sites of the m^3 unit lattice split by the parity of their coordinate sum: (even, odd)."""
    from tests.tpcf_oracle import lattice
    lat = lattice(m)
    odd = (lat.sum(axis=1).astype(np.int64) % 2).astype(bool)
    return lat[~odd], lat[odd]


def parity_lattice_expected(m, s_edges, mu_edges, los):
    """Cross counts of the parity-split lattice in a box of side m (m even, top edge < m / 2): every even site has one
    odd partner per integer vector v with |v|^2 odd: m^3 / 2 x #{v : |v|^2 odd and in the bin}."""
    s2 = np.asarray(s_edges, dtype=np.float64) ** 2
    mu_e = np.asarray(mu_edges, dtype=np.float64)
    out = np.zeros((len(s2) - 1, len(mu_e) - 1), dtype=np.int64)
    r = int(np.ceil(np.sqrt(s2[-1])))
    for vx in range(-r, r + 1):
        for vy in range(-r, r + 1):
            for vz in range(-r, r + 1):
                q = vx * vx + vy * vy + vz * vz
                if q % 2 == 0 or not (s2[0] < q <= s2[-1]):
                    continue
                mu = abs((vx, vy, vz)[los]) / np.sqrt(q)
                if not (mu_e[0] < mu <= mu_e[-1]):
                    continue
                out[int(np.searchsorted(s2, q, side="left")) - 1, int(np.searchsorted(mu_e, mu, side="left")) - 1] += 1
    return out * (m ** 3 // 2)
