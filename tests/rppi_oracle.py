"""numpy restatement of the (r_p, pi) pair counts (device.rp_pi_pair_counts / rp_pi_cross_counts /
rp_pi_jackknife_counts, astrild_amd.particles.hutils.tpcf.rp_pi_tpcf / wp), written from the definition: with ``los`` the
line of sight and a < b the two other axes, p_c = |x_i - x_j| per axis (``_sep`` of tests/tpcf_cross_oracle.py: the
minimum image with a boxsize), rp2 = p_a p_a + p_b p_b, pi = p_los, and a pair in bin (k, l) when
rp_k^2 < rp2 <= rp_{k+1}^2 and pi_l < pi <= pi_{l+1} (np.searchsorted, side="left", on the squared r_p edges and on the
pi edges as given).  Brute force over all pairs; the estimators are those of tests/tpcf_cross_oracle.py."""
import numpy as np

from tests.tpcf_cross_oracle import ESTIMATORS, _sep, estimator, estimator_terms       # noqa: F401  (re-exported)


def _edges(rp_edges, pi_edges):
    rp = np.asarray(rp_edges, dtype=np.float64).reshape(-1)
    return rp * rp, np.asarray(pi_edges, dtype=np.float64).reshape(-1)


def _axes(los):
    a, b = [c for c in range(3) if c != los]
    return a, b


def bin_pairs(pa, pb, pl, rp2_e, pi_e, weights=None):
    """(n_rp, n_pi) int64 counts of pairs given by their separations across (pa, pb) and along (pl) the line of sight;
    ``weights``: an integer per pair instead of 1."""
    rp2 = pa * pa + pb * pb
    k = np.searchsorted(rp2_e, rp2, side="left") - 1
    l = np.searchsorted(pi_e, pl, side="left") - 1
    nrp, npi = len(rp2_e) - 1, len(pi_e) - 1
    ok = (k >= 0) & (k < nrp) & (l >= 0) & (l < npi)
    flat = k[ok] * npi + l[ok]
    w = None if weights is None else np.asarray(weights)[ok].astype(np.float64)
    out = np.bincount(flat, weights=w, minlength=nrp * npi)
    return np.rint(out).astype(np.int64).reshape(nrp, npi)


def rppi_cross_brute(a, b, rp_edges, pi_edges, los=2, boxsize=None, chunk=256):
    """Counts of all pairs (i of a, j of b), (n_rp, n_pi) int64; fp64 positions (inside [0, boxsize] with one)."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
    rp2_e, pi_e = _edges(rp_edges, pi_edges)
    la, lb = _axes(los)
    out = np.zeros((len(rp2_e) - 1, len(pi_e) - 1), dtype=np.int64)
    if len(b):
        for i0 in range(0, len(a), chunk):
            p = [_sep(a[i0:i0 + chunk, ax, None], b[None, :, ax], boxsize).ravel() for ax in (la, lb, los)]
            out += bin_pairs(p[0], p[1], p[2], rp2_e, pi_e)
    return out


def rppi_auto_brute(pos, rp_edges, pi_edges, los=2, boxsize=None, chunk=256):
    """Unordered pairs i < j of one set."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    rp2_e, pi_e = _edges(rp_edges, pi_edges)
    la, lb = _axes(los)
    out = np.zeros((len(rp2_e) - 1, len(pi_e) - 1), dtype=np.int64)
    n = len(pos)
    cols = np.arange(n)
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        upper = cols[None, i0:] > cols[i0:i1, None]
        p = [_sep(pos[i0:i1, ax, None], pos[None, i0:, ax], boxsize)[upper] for ax in (la, lb, los)]
        out += bin_pairs(p[0], p[1], p[2], rp2_e, pi_e)
    return out


def rp_counts_brute(a, b, rp_edges, los=2, boxsize=None):
    """Counts of all pairs (i of a, j of b) per r_p bin alone, whatever pi is: a direct count, without pi edges."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
    rp = np.asarray(rp_edges, dtype=np.float64)
    la, lb = _axes(los)
    pa, pb = _sep(a[:, la, None], b[None, :, la], boxsize), _sep(a[:, lb, None], b[None, :, lb], boxsize)
    rp2 = (pa * pa + pb * pb).ravel()
    return np.array([np.count_nonzero((rp2 > lo * lo) & (rp2 <= hi * hi)) for lo, hi in zip(rp[:-1], rp[1:])],
                    dtype=np.int64)


def bin_volume(rp_edges, pi_edges):
    """pi (rp_{k+1}^2 - rp_k^2) x 2 (pi_{l+1} - pi_l): what a bin offers the second object of an ordered pair."""
    rp, pi = np.asarray(rp_edges, dtype=np.float64), np.asarray(pi_edges, dtype=np.float64)
    return np.outer(np.pi * (rp[1:] ** 2 - rp[:-1] ** 2), 2.0 * np.diff(pi))


def analytic_xi(dd_ordered, na, nb, boxsize, rp_edges, pi_edges):
    """DD / (Na Nb v / L^3) - 1 from ORDERED pair counts (2 x unordered for an auto term)."""
    rr = float(na) * float(nb) * bin_volume(rp_edges, pi_edges) / float(boxsize) ** 3
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(dd_ordered, dtype=np.float64) / rr - 1.0


def wp_from_xi(xi, pi_edges):
    """w_p = 2 sum_l xi(r_p, pi_l) dpi_l."""
    xi = np.asarray(xi, dtype=np.float64)
    dpi = np.diff(np.asarray(pi_edges, dtype=np.float64))
    out = np.zeros(xi.shape[:-1])
    for l in range(len(dpi)):
        out = out + xi[..., l] * dpi[l]
    return 2.0 * out


def wp_matrix(nrp, pi_edges):
    """A of w_p = A xi.ravel(): (n_rp, n_rp n_pi)."""
    dpi = np.diff(np.asarray(pi_edges, dtype=np.float64))
    a = np.zeros((nrp, nrp * len(dpi)))
    for k in range(nrp):
        a[k, k * len(dpi):(k + 1) * len(dpi)] = 2.0 * dpi
    return a


def jackknife_brute(a, ta, b, tb, ntot, rp_edges, pi_edges, los=2, boxsize=None):
    """``(counts, w2)`` of the pairs (i of a, j of b), or with ``b`` None the unordered pairs of ``a``.  ``w2[k]`` is
    TWICE the weighted count with region k left out, pair by pair from the weights: 1 when neither end lies in k, 1/2
    when exactly one does, 0 when both do (twice them: 2 / 1 / 0, integers).  (n_rp, n_pi) and (ntot, n_rp, n_pi)."""
    a, ta = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(ta, dtype=np.int64)
    auto = b is None
    b, tb = (a, ta) if auto else (np.asarray(b, dtype=np.float64).reshape(-1, 3), np.asarray(tb, dtype=np.int64))
    rp2_e, pi_e = _edges(rp_edges, pi_edges)
    la, lb = _axes(los)
    shape = (len(rp2_e) - 1, len(pi_e) - 1)
    if not len(a) or not len(b):
        return np.zeros(shape, dtype=np.int64), np.zeros((ntot,) + shape, dtype=np.int64)
    i, j = np.meshgrid(np.arange(len(a)), np.arange(len(b)), indexing="ij")
    keep = (j > i) if auto else np.ones_like(i, dtype=bool)
    i, j = i[keep], j[keep]
    p = [_sep(a[i, ax], b[j, ax], boxsize) for ax in (la, lb, los)]
    near = (p[0] * p[0] + p[1] * p[1] <= rp2_e[-1]) & (p[2] <= pi_e[-1])
    i, j, p = i[near], j[near], [x[near] for x in p]
    counts = bin_pairs(p[0], p[1], p[2], rp2_e, pi_e)
    w2 = np.zeros((ntot,) + shape, dtype=np.int64)
    for k in range(ntot):
        twice_weight = 2 - (ta[i] == k).astype(np.int64) - (tb[j] == k).astype(np.int64)
        w2[k] = bin_pairs(p[0], p[1], p[2], rp2_e, pi_e, weights=twice_weight)
    return counts, w2


def lattice_expected(m, rp_edges, pi_edges, los):
    """Unordered pair counts of the m^3 unit lattice in a periodic box of side m, for top edges < m / 2: every site
    has one partner per integer vector v != 0 (the minimum image is |v| itself), so m^3 / 2 x #{v in the bin}."""
    rp2_e, pi_e = _edges(rp_edges, pi_edges)
    la, lb = _axes(los)
    assert np.sqrt(rp2_e[-1]) < m / 2 and pi_e[-1] < m / 2
    r = int(np.ceil(max(np.sqrt(rp2_e[-1]), pi_e[-1])))
    out = np.zeros((len(rp2_e) - 1, len(pi_e) - 1), dtype=np.int64)
    for vx in range(-r, r + 1):
        for vy in range(-r, r + 1):
            for vz in range(-r, r + 1):
                v = (vx, vy, vz)
                if v == (0, 0, 0):
                    continue
                rp2, pl = v[la] * v[la] + v[lb] * v[lb], abs(v[los])
                if not (rp2_e[0] < rp2 <= rp2_e[-1]) or not (pi_e[0] < pl <= pi_e[-1]):
                    continue
                out[int(np.searchsorted(rp2_e, rp2, side="left")) - 1,
                    int(np.searchsorted(pi_e, pl, side="left")) - 1] += 1
    assert not ((out * m ** 3) % 2).any()
    return out * m ** 3 // 2
