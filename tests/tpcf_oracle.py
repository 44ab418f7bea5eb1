"""numpy restatement of the periodic two-point correlation function of particles/hutils/tpcf.py (halotools' s_mu_tpcf
and tpcf with analytic randoms), op for op as astrild_amd.particles.hutils.tpcf documents it: the redshift-space shift
and wrap in the input dtypes, the minimum image per axis, d^2 = (a_x^2 + a_y^2) + a_z^2, mu = a_los / sqrt(d^2), and
half-open bins s_k^2 < d^2 <= s_{k+1}^2, mu_l < mu <= mu_{l+1}.  pair_counts_brute visits all pairs in row chunks;
pair_counts applies the same arithmetic to a periodic cKDTree's candidate pairs (fast at N ~ 10^5)."""
import numpy as np


def shift_and_wrap(pos, vel, boxsize, los=2):
    """tpcf.py:74-97 in the input dtypes: pos[:, los] += vel[:, los] / 100. (vel / 100 in vel's dtype, the add in the
    wider dtype and stored as pos's dtype), then > L -> - L and < 0 -> + L in pos's dtype.  Returns fp64 (N, 3)."""
    pos = np.array(pos, copy=True)
    if vel is not None:
        vel = np.asarray(vel)
        t = pos.dtype.type
        box = t(boxsize)
        pos[:, los] += vel[:, los] / vel.dtype.type(100.0)
        c = pos[:, los]
        pos[:, los] = np.where(c > box, c - box, c)
        c = pos[:, los]
        pos[:, los] = np.where(c < t(0.0), c + box, c)
    return pos.astype(np.float64)


def _bin(a, s2, mu_e, los, counts):
    """Add the pairs with per-axis minimum-image separations a[0..2] (arrays of equal shape) to counts."""
    nmu = 0 if mu_e is None else len(mu_e) - 1
    d2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    sel = (d2 > s2[0]) & (d2 <= s2[-1])
    d2s = d2[sel]
    k = np.searchsorted(s2, d2s, side="left") - 1                 # s2[k] < d2 <= s2[k + 1]
    if nmu:
        mu = a[los][sel] / np.sqrt(d2s)
        ok = (mu > mu_e[0]) & (mu <= mu_e[-1])
        l = np.searchsorted(mu_e, mu[ok], side="left") - 1        # mu_e[l] < mu <= mu_e[l + 1]
        idx = k[ok] * nmu + l
    else:
        idx = k
    counts += np.bincount(idx, minlength=len(counts))


def _setup(s_edges, mu_edges):
    s2 = np.asarray(s_edges, dtype=np.float64) ** 2
    mu_e = None if mu_edges is None else np.asarray(mu_edges, dtype=np.float64)
    nmu = 0 if mu_e is None else len(mu_e) - 1
    return s2, mu_e, nmu, np.zeros((len(s2) - 1) * max(nmu, 1), dtype=np.int64)


def pair_counts_brute(pos64, boxsize, s_edges, mu_edges=None, los=2, chunk=256):
    """Unordered pair counts, (ns, nmu) or (ns,) int64, of fp64 positions already in [0, boxsize]: every pair i < j."""
    pos = np.asarray(pos64, dtype=np.float64)
    L = float(boxsize)
    s2, mu_e, nmu, counts = _setup(s_edges, mu_edges)
    n = len(pos)
    cols = np.arange(n)
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        upper = cols[None, i0:] > cols[i0:i1, None]               # j > i
        a = []
        for ax in range(3):
            d = np.abs(pos[i0:i1, ax, None] - pos[None, i0:, ax])[upper]
            a.append(np.minimum(d, L - d))
        _bin(a, s2, mu_e, los, counts)
    return counts.reshape(-1, nmu) if nmu else counts


def pair_counts(pos64, boxsize, s_edges, mu_edges=None, los=2):
    """The same counts with the same arithmetic, on the candidate pairs of a periodic cKDTree within the top edge
    plus a relative margin of 1e-6 (a superset of the pairs in reach; the bin tests are pair_counts_brute's)."""
    from scipy.spatial import cKDTree
    pos = np.asarray(pos64, dtype=np.float64)
    L = float(boxsize)
    s2, mu_e, nmu, counts = _setup(s_edges, mu_edges)
    if len(pos) > 1:
        tree = cKDTree(np.minimum(pos, np.nextafter(L, 0.0)), boxsize=L)   # cKDTree wants [0, L)
        ij = tree.query_pairs(float(np.sqrt(s2[-1])) * (1.0 + 1e-6), output_type="ndarray")
        for c0 in range(0, len(ij), 1 << 22):
            i, j = ij[c0:c0 + (1 << 22), 0], ij[c0:c0 + (1 << 22), 1]
            a = []
            for ax in range(3):
                d = np.abs(pos[i, ax] - pos[j, ax])
                a.append(np.minimum(d, L - d))
            _bin(a, s2, mu_e, los, counts)
    return counts.reshape(-1, nmu) if nmu else counts


def rr(n, boxsize, s_edges, mu_edges=None):
    """Analytic RR of a periodic box: N^2 (4 pi / 3)(s_{k+1}^3 - s_k^3)(mu_{l+1} - mu_l) / L^3."""
    s = np.asarray(s_edges, dtype=np.float64)
    shell = (4.0 * np.pi / 3.0) * (s[1:] ** 3 - s[:-1] ** 3)
    if mu_edges is not None:
        shell = np.outer(shell, np.diff(np.asarray(mu_edges, dtype=np.float64)))
    return float(n) * float(n) * shell / float(boxsize) ** 3


def xi(counts, n, boxsize, s_edges, mu_edges=None):
    """2 DD / RR - 1 (DD = ordered pairs = 2 x the unordered counts)."""
    return 2.0 * counts.astype(np.float64) / rr(n, boxsize, s_edges, mu_edges) - 1.0


def multipole(xi_s_mu, mu_edges, order):
    """(2 l + 1) / 2 * sum_mu xi * dmu * (P_l(mu_c) + P_l(-mu_c)), P_l written out for l <= 4."""
    mu = np.asarray(mu_edges, dtype=np.float64)
    c = (mu[:-1] + mu[1:]) / 2.0
    p = {0: lambda x: np.ones_like(x), 1: lambda x: x, 2: lambda x: (3.0 * x * x - 1.0) / 2.0,
         3: lambda x: (5.0 * x ** 3 - 3.0 * x) / 2.0, 4: lambda x: (35.0 * x ** 4 - 30.0 * x * x + 3.0) / 8.0}[order]
    return (2.0 * order + 1.0) / 2.0 * np.sum(np.asarray(xi_s_mu) * np.diff(mu) * (p(c) + p(-c)), axis=1)


def uniform(n, boxsize, seed, dtype=np.float64):
    return np.random.default_rng(seed).uniform(0.0, boxsize, (n, 3)).astype(dtype)


def clustered(n, boxsize, seed, blobs=50, sigma=5.0, dtype=np.float64):
    """Gaussian blobs around uniform centres, wrapped periodically into [0, boxsize)."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0.0, boxsize, (blobs, 3))
    pos = centres[rng.integers(0, blobs, n)] + rng.normal(0.0, sigma, (n, 3))
    return np.mod(pos, boxsize).astype(dtype)


def lattice(m, spacing=1.0):
    """m^3 simple-cubic lattice with integer coordinates 0 .. m - 1 (times spacing)."""
    g = np.arange(m, dtype=np.float64) * spacing
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def lattice_expected(m, s_edges, mu_edges, los, reach):
    """Unordered counts of an m^3 lattice with unit spacing in a box of side m, from the integer vectors v with
    |v| <= reach: N / 2 x #{v : |v|^2 in the s bin, |v_los| / |v| in the mu bin} (needs reach < m / 2)."""
    s2 = np.asarray(s_edges, dtype=np.float64) ** 2
    mu_e = np.asarray(mu_edges, dtype=np.float64)
    out = np.zeros((len(s2) - 1, len(mu_e) - 1), dtype=np.int64)
    r = int(np.ceil(reach))
    for vx in range(-r, r + 1):
        for vy in range(-r, r + 1):
            for vz in range(-r, r + 1):
                q = vx * vx + vy * vy + vz * vz
                if q == 0 or not (s2[0] < q <= s2[-1]):
                    continue
                k = int(np.searchsorted(s2, q, side="left")) - 1
                mu = abs((vx, vy, vz)[los]) / np.sqrt(q)
                if not (mu_e[0] < mu <= mu_e[-1]):
                    continue
                out[k, int(np.searchsorted(mu_e, mu, side="left")) - 1] += 1
    n = m ** 3
    return out * n // 2
