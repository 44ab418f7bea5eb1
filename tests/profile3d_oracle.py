"""numpy restatement of the spherical profiles of particles around centres (astrild_amd.profiles.profile_3d,
ast_profile3d_*), op for op as the package documents them: a loop over centres; per centre the signed separation
s = p - c in float64, wrapped once per axis in a periodic box (s > L/2 -> s - L, else s < -L/2 -> s + L),
x = np.sqrt((sx^2 + sy^2) + sz^2) / R, np.histogram for the counts and np.bincount with weights for the moments
sum w, sum w v_r, sum w v_r^2, sum w |u|^2 (u = v - centre velocity, v_r = ((ux sx + uy sy) + uz sz) / d, 0 at d = 0).
Also returns sum |term| per bin and moment, the scale of the tests' tolerances."""
import numpy as np


def separations(pos64, c, boxsize=None):
    """(N, 3) signed separations of fp64 positions from one centre, wrapped once per axis when ``boxsize`` is given."""
    s = pos64 - np.asarray(c, dtype=np.float64)
    if boxsize is not None:
        L = float(boxsize)
        s = np.where(s > L / 2, s - L, np.where(s < -L / 2, s + L, s))
    return s


def scaled_distance(s, R):
    return np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]) / R


def bin_index(x, edges):
    """np.histogram's bin of each x (e_k <= x < e_{k+1}, the last bin closed), -1 outside."""
    k = np.searchsorted(edges, x, side="right") - 1
    k = np.where(x == edges[-1], len(edges) - 2, k)
    return np.where((x >= edges[0]) & (x <= edges[-1]), k, -1)


def profiles(pos, centres, radii, edges, boxsize=None, weights=None, vel=None, centre_vel=None, segments=None):
    """``(counts, moments, scale)``: (Nc, nbins) int64, (Nc, nbins, M) float64 and the sums of |term| in the shape of
    ``moments``; M = 4 with ``vel``, else 1.  ``segments`` (Nc, 2) (offset, count): centre i sees only that slice."""
    pos64 = np.asarray(pos).astype(np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    centres = np.asarray(centres).astype(np.float64).reshape(-1, 3)
    radii = np.asarray(radii).astype(np.float64).reshape(-1)
    nc, nbins, M = len(radii), len(edges) - 1, 4 if vel is not None else 1
    w_all = np.ones(len(pos64)) if weights is None else np.asarray(weights).astype(np.float64)
    v_all = None if vel is None else np.asarray(vel).astype(np.float64)
    counts = np.zeros((nc, nbins), dtype=np.int64)
    moments = np.zeros((nc, nbins, M))
    scale = np.zeros((nc, nbins, M))
    for i in range(nc):
        sl = slice(None) if segments is None else slice(int(segments[i][0]), int(segments[i][0]) + int(segments[i][1]))
        s = separations(pos64[sl], centres[i], boxsize)
        x = scaled_distance(s, radii[i])
        counts[i] = np.histogram(x, bins=edges)[0]
        k = bin_index(x, edges)
        ok = k >= 0
        k, w = k[ok], w_all[sl][ok]
        terms = [w]
        if M == 4:
            s = s[ok]
            u = v_all[sl][ok] - (0.0 if centre_vel is None else np.asarray(centre_vel, dtype=np.float64)[i])
            d = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
            dot = (u[:, 0] * s[:, 0] + u[:, 1] * s[:, 1]) + u[:, 2] * s[:, 2]
            vr = np.divide(dot, d, out=np.zeros_like(d), where=d > 0)
            terms += [w * vr, w * (vr * vr), w * ((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])]
        for m, t in enumerate(terms):
            moments[i, :, m] = np.bincount(k, weights=t, minlength=nbins)
            scale[i, :, m] = np.bincount(k, weights=np.abs(t), minlength=nbins)
        assert np.array_equal(np.bincount(k, minlength=nbins), counts[i])
    return counts, moments, scale


def unit_lattice(m=8):
    """arange(m)^3: the m^3 integer points, (m^3, 3) float64."""
    g = np.arange(m, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


#: (centres, edges, counts per centre) on unit_lattice(8) in a periodic box of 8 with R = 1: values on edges, the
#: closed last edge, the particle at the centre, wraps through faces and the corner.
LATTICE_CASES = (
    ([(0, 0, 0), (3, 4, 7), (7, 0, 4)], [0.5, 1.0, np.sqrt(2.0), np.sqrt(3.0), 2.0, 3.0], [0, 6, 12, 8, 96]),
    ([(0, 0, 0)], [0.0, 1.0, 2.0], [1, 32]),
    ([(7.5, 7.5, 7.5)], np.sqrt([0.0, 0.75, 2.75, 4.75, 6.75]), [0, 8, 24, 56]),
)
