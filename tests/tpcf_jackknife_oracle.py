"""numpy oracle of the jackknife two-point correlation function (device.tpcf_jackknife_counts,
astrild_amd.particles.hutils.tpcf.tpcf_jackknife), written from the WEIGHT definition of halotools' tpcf_jackknife as
the package recalls it: with region k left out a pair weighs 1 when neither end lies in k, 1/2 when exactly one does and
0 when both do.  Brute force over all pairs with the arithmetic and the bins of tests/tpcf_oracle.py (_setup / _bin).
The endpoint identity the kernel rests on (2 W_k == 2 counts - E_k) is NOT used here: weighted_counts forms 2 W_k pair
by pair from the weights, endpoint_table counts pair ends, and the tests compare the two."""
import numpy as np

from tests.tpcf_cross_oracle import estimator
from tests.tpcf_oracle import _bin, _setup


def region_tags(pos, nsub, lo, hi):
    """Region of every object: per axis floor((x - lo) / dL), dL = (hi - lo) / nsub in fp64, clamped into the grid; C
    order over (x, y, z).  One axis at a time, in plain Python integers at the end."""
    pos = np.asarray(pos).astype(np.float64).reshape(-1, 3)
    idx = []
    for ax in range(3):
        dl = (float(hi[ax]) - float(lo[ax])) / float(nsub[ax])
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.floor((pos[:, ax] - float(lo[ax])) / dl)
        q[~(q >= 0)] = 0
        q[q > nsub[ax] - 1] = nsub[ax] - 1
        idx.append(q.astype(np.int64))
    return np.ravel_multi_index(idx, tuple(int(v) for v in nsub)) if len(pos) else np.zeros(0, dtype=np.int64)


def _near_pairs(a, b, s2top, boxsize, chunk=256):
    """Index arrays (i, j) of the pairs within the top edge (plus a margin; the bin tests are _bin's): i < j of ``a``
    when ``b`` is None, else every (i of a, j of b)."""
    auto = b is None
    b = a if auto else b
    ii, jj = [], []
    reach = s2top * (1.0 + 1e-9)
    for i0 in range(0, len(a), chunk):
        d2 = np.zeros((len(a[i0:i0 + chunk]), len(b)))
        for ax in range(3):
            d = np.abs(a[i0:i0 + chunk, ax, None] - b[None, :, ax])
            if boxsize is not None:
                d = np.minimum(d, float(boxsize) - d)
            d2 += d * d
        i, j = np.nonzero(d2 <= reach)
        i += i0
        if auto:
            keep = j > i
            i, j = i[keep], j[keep]
        ii.append(i)
        jj.append(j)
    cat = lambda x: np.concatenate(x) if x else np.zeros(0, dtype=np.int64)
    return cat(ii), cat(jj)


def _count(a, b, i, j, s2, mu_e, los, boxsize, nbins):
    out = np.zeros(nbins, dtype=np.int64)
    if len(i):
        sep = []
        for ax in range(3):
            d = np.abs(a[i, ax] - b[j, ax])
            sep.append(d if boxsize is None else np.minimum(d, float(boxsize) - d))
        _bin(sep, s2, mu_e, los, out)
    return out


def jackknife_counts_brute(a, ta, b, tb, ntot, s_edges, mu_edges=None, los=2, boxsize=None):
    """``(counts, w2, ends)`` of the pairs (i of a, j of b), or with ``b`` None the unordered pairs of ``a``: ``counts``
    as the plain oracles; ``w2[k]`` = 2 x the weighted count with region k left out, from the weights 1 / 1/2 / 0 per
    pair (twice them: 2 / 1 / 0, integers); ``ends[k]`` = the pair ends in region k, one selection per end.  Shapes
    (ns[, nmu]) and (ntot, ns[, nmu]), int64."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    ta = np.asarray(ta, dtype=np.int64)
    if b is not None:
        b, tb = np.asarray(b, dtype=np.float64).reshape(-1, 3), np.asarray(tb, dtype=np.int64)
    s2, mu_e, nmu, zero = _setup(s_edges, mu_edges)
    nbins = len(zero)
    bb, tbb = (a, ta) if b is None else (b, tb)
    i, j = _near_pairs(a, b, s2[-1], boxsize) if len(a) and len(bb) else (np.zeros(0, dtype=np.int64),) * 2
    cnt = lambda sel: _count(a, bb, i[sel], j[sel], s2, mu_e, los, boxsize, nbins)
    counts = cnt(slice(None))
    w2 = np.zeros((ntot, nbins), dtype=np.int64)
    ends = np.zeros((ntot, nbins), dtype=np.int64)
    for k in range(ntot):
        in_i, in_j = ta[i] == k, tbb[j] == k
        twice_weight = 2 - in_i.astype(np.int64) - in_j.astype(np.int64)
        w2[k] = 2 * cnt(twice_weight == 2) + cnt(twice_weight == 1)
        ends[k] = cnt(in_i) + cnt(in_j)
    shape = (-1, nmu) if nmu else (-1,)
    return counts.reshape(shape), w2.reshape((ntot,) + counts.reshape(shape).shape), \
        ends.reshape((ntot,) + counts.reshape(shape).shape)


def xi_and_cov(name, w2, counts, sizes, occupancy, a, b):
    """Full-sample xi and the jackknife covariance for the term (a, b) in "1", "2": a loop over the regions, every xi_k
    from the WEIGHTED counts (tests.tpcf_cross_oracle.estimator), the covariance by np.cov over the xi_k.
    ``w2`` / ``counts``: dicts under D1D1, D1D2, D2D2, D1R, D2R, RR; ``sizes`` / ``occupancy``: dicts under "1", "2",
    "R" of N and of the objects per region."""
    dd, dr = ("D1D2" if a != b else f"D{a}D{a}"), f"D{a}R"
    f = lambda x: np.asarray(x, dtype=np.float64)
    # ordered pairs: an auto term's are twice its unordered (weighted) count, i.e. w2 itself; the others w2 / 2
    ordered_full = lambda t: None if t not in counts else (2.0 if t in ("D1D1", "D2D2", "RR") else 1.0) * f(counts[t])
    ordered_k = lambda t, k: None if t not in w2 else f(w2[t][k]) * (1.0 if t in ("D1D1", "D2D2", "RR") else 0.5)
    xi = estimator(name, ordered_full(dd), ordered_full(dr), ordered_full("RR"), sizes[a], sizes[b], sizes["R"])
    n = len(occupancy["R"])
    xik = []
    for k in range(n):
        left = {s: sizes[s] - int(occupancy[s][k]) for s in occupancy}
        xik.append(estimator(name, ordered_k(dd, k), ordered_k(dr, k), ordered_k("RR", k), left[a], left[b],
                             left["R"]).reshape(-1))
    xik = np.array(xik)
    cov = (n - 1.0) * np.atleast_2d(np.cov(xik, rowvar=False, bias=True)) if n > 1 else np.zeros((xik.shape[1],) * 2)
    return xi, cov, xik
