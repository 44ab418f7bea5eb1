"""Radial profiles of objects (voids, peaks) on 2D maps: the reference's ``astrild.profiles.profile_2d``.

``from_map`` / ``profiling`` put every pixel of an object's (2R)^2 square, R = ceil(r * extend), into annulus
eta = int(sqrt(a^2 + b^2) / r / delta_eta) and average each annulus (profile_2d.py:10-59, :92-153).  Here the pixel loop
runs on the GPU (``device.annulus_profiles``, ``ast_profile2d``) and the host decides every bin exactly:

* eta never decreases as d2 = a^2 + b^2 grows (int64 -> float64 is exact below 2^53; sqrt and the two divisions are
  correctly rounded and monotone), so ``annulus_thresholds`` finds T_k = min{d2 : eta(d2) >= k} by binary search with
  numpy's own expression.  Pixel (a, b) is in bin k when T_k <= d2 < T_{k+1} and is read when d2 < T_nbins; the device
  compares integers only.
* The read reach m = max{t <= R : t^2 < T_nbins} decides the rows and columns read, [-m, min(m, R - 1)].  numpy wraps an
  index in [-n, 0) and raises IndexError beyond; that is checked here before any GPU work.
* The reference divides the annulus sums by counts that list the counts of the annuli present, in ascending order,
  then zeros (profile_2d.py:126-129): an empty annulus in the middle shifts the counts left.  ``from_map`` keeps that.

``interpolate``, ``mean_and_interpolate`` and ``bootstrapping`` run on the host with the reference's loop structure,
so that in-place changes feed later steps as they do there.  Deliberate differences: r < 1, extend <= 0, nbins < 1 and
an empty catalogue raise ValueError (the reference divides by zero or fails with UnboundLocalError), and nothing is
printed.
"""
import math

import numpy as np

__all__ = ["from_map", "profiling", "interpolate", "mean_and_interpolate", "bootstrapping", "annulus_thresholds",
           "annulus_geometry", "radii_of"]


def _eta(d2, r, delta_eta):
    """The reference's annulus index of squared distance(s) d2 (int64) for radius r (profile_2d.py:118-121)."""
    return (np.sqrt(np.asarray(d2, dtype=np.int64)) / r / delta_eta).astype(int)


def annulus_thresholds(r, extend, nbins, delta_eta=None):
    """(R, T, m) for an integer radius r >= 1: R = ceil(r * extend), T[k - 1] = min{d2 in [0, 2R^2] : eta(d2) >= k} for
    k = 1..nbins (2R^2 + 1 when no d2 of the square reaches bin k), int64, and the read reach m."""
    de = extend / nbins if delta_eta is None else delta_eta
    R = int(np.ceil(r * extend))
    top = 2 * R * R
    want = np.arange(1, nbins + 1, dtype=np.int64)
    lo = np.zeros(nbins, dtype=np.int64)
    hi = np.full(nbins, top + 1, dtype=np.int64)          # hi = top + 1 stands for "no d2 of the square"
    while True:
        open_ = lo < hi
        if not open_.any():
            break
        mid = (lo + hi) // 2
        ok = _eta(np.minimum(mid, top), r, de) >= want
        hi = np.where(open_ & ok, mid, hi)
        lo = np.where(open_ & ~ok, mid + 1, lo)
    T = lo
    m = min(R, math.isqrt(int(T[-1]) - 1))
    return R, T, m


def radii_of(extend, nbins):
    """Midpoints of linspace(0, extend, nbins + 1) (profile_2d.py:139-140)."""
    edges = np.linspace(0, extend, nbins + 1)
    return 0.5 * (edges[1:] + edges[:-1])


def _as_index(v, name):
    """int() of each value, truncating toward zero, as the reference's int(row[...])."""
    a = np.asarray(v)
    if a.dtype.kind in "iub":
        return a.astype(np.int64)
    a = a.astype(np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name} must be finite")
    return np.trunc(a).astype(np.int64)


def annulus_geometry(shape, x_pix, y_pix, rad_pix, extend, nbins, delta_eta=None):
    """Per object (y, x, R, m, T): the truncated centre, the square's half width, the read reach and the bin thresholds
    ((n, nbins) int64).  ValueError for an empty catalogue, r < 1, extend <= 0 or nbins < 1; IndexError, as numpy would
    raise it, when a read pixel lies outside [-n, n) on either axis."""
    extend = float(extend)
    if int(nbins) != nbins or nbins < 1:
        raise ValueError(f"nbins must be a positive integer, got {nbins}")
    nbins = int(nbins)
    if not (extend > 0 and math.isfinite(extend)):
        raise ValueError(f"extend must be positive and finite, got {extend}")
    if delta_eta is not None and not (delta_eta > 0 and math.isfinite(delta_eta)):
        raise ValueError(f"delta_eta must be positive and finite, got {delta_eta}")
    r = _as_index(rad_pix, "rad_pix").reshape(-1)
    x = _as_index(x_pix, "x_pix").reshape(-1)
    y = _as_index(y_pix, "y_pix").reshape(-1)
    if len(r) == 0:
        raise ValueError("the catalogue is empty")
    if not (len(x) == len(r) == len(y)):
        raise ValueError("x_pix, y_pix and rad_pix must have the same length")
    if r.min() < 1:
        raise ValueError(f"rad_pix must be >= 1 after truncation, got {int(r.min())}")
    ny, nx = int(shape[0]), int(shape[1])
    uniq, inv = np.unique(r, return_inverse=True)
    Rs = np.empty(len(uniq), dtype=np.int64)
    ms = np.empty(len(uniq), dtype=np.int64)
    Ts = np.empty((len(uniq), nbins), dtype=np.int64)
    for i, rr in enumerate(uniq.tolist()):
        Rs[i], Ts[i], ms[i] = annulus_thresholds(rr, extend, nbins, delta_eta)
    R, m = Rs[inv], ms[inv]
    up = np.minimum(m, R - 1)
    for c, n, axis in ((y, ny, 0), (x, nx, 1)):
        bad = (c - m < -n) | (c + up >= n)
        if bad.any():
            i = int(np.argmax(bad))
            idx = int(c[i] - m[i]) if c[i] - m[i] < -n else int(c[i] + up[i])
            raise IndexError(f"index {idx} is out of bounds for axis {axis} with size {n} "
                             f"(object {i}: x {int(x[i])}, y {int(y[i])}, rad_pix {int(r[i])})")
    return y, x, R, m, Ts[inv]


def _columns(objects):
    return objects["x_pix"].values, objects["y_pix"].values, objects["rad_pix"].values


def aligned_values(sums, counts):
    """The reference's annulus values: sums / counts with each row's nonzero counts packed to the front in bin order and
    zeros after (profile_2d.py:126-143); 0/0 gives nan and x/0 gives +-inf, as in numpy."""
    sums = np.asarray(sums, dtype=np.float64)
    counts = np.asarray(counts)
    nz = counts != 0
    order = np.argsort(~nz, axis=1, kind="stable")
    packed = np.take_along_axis(np.where(nz, counts, 0), order, axis=1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return sums / packed


def from_map(objects, skymap, extend, nr_profile_bins, return_counts=False):
    """Profiles of every object of ``objects`` (columns x_pix, y_pix, rad_pix) on ``skymap``: {"values": (N, nbins)
    float64, "radii": (nbins,)} (profile_2d.py:10-59).  ``skymap`` is a 2D numpy array or a device tensor, float32 or
    float64 (e.g. ``SkyArray.data.device("orig")``).  ``return_counts=True`` adds the true per-annulus "sums" and
    "counts"."""
    from .. import device as dev
    x, y, r = _columns(objects)
    sums, counts = dev.annulus_profiles(skymap, x, y, r, extend, nr_profile_bins)
    sums, counts = dev.to_numpy(sums), dev.to_numpy(counts)
    out = {"values": aligned_values(sums, counts), "radii": radii_of(extend, nr_profile_bins)}
    if return_counts:
        out["sums"], out["counts"] = sums, counts
    return out


def profiling(obj_radius, obj_pos, mapp, delta_eta, extend, nr_profile_bins):
    """Profile of one object at ``obj_pos`` = (x, y) pixels (profile_2d.py:92-153): {"radii", "values"}."""
    from .. import device as dev
    sums, counts = dev.annulus_profiles(mapp, [obj_pos[0]], [obj_pos[1]], [obj_radius], extend, nr_profile_bins,
                                        delta_eta=delta_eta)
    values = aligned_values(dev.to_numpy(sums), dev.to_numpy(counts))[0]
    return {"radii": radii_of(extend, nr_profile_bins), "values": values}


def _fill_rows(profile, r):
    """The reference's clean-up of a stack of profiles, in place (profile_2d.py:205-222 / :237-256): every nan becomes 0,
    then each nan entry's row is interpolated over its nonzero entries, once per nan entry; without nans, the rows of
    the first len(profile) - (row of the first zero) zero entries, in np.where order, are interpolated the same way."""
    where_nan = np.argwhere(np.isnan(profile))
    if len(where_nan):
        for row, col in where_nan:
            profile[row, col] = 0
        for row, _ in where_nan:
            keep = profile[row] != 0
            profile[row] = np.interp(r, r[keep], profile[row][keep])
        return profile
    where_zero = np.argwhere(profile == 0)
    if len(where_zero):
        first_row = where_zero[0, 0]
        for i in range(len(profile) - first_row):
            row = where_zero[i, 0]                    # IndexError when there are fewer zeros, as in the reference
            keep = profile[row] != 0
            profile[row] = np.interp(r, r[keep], profile[row][keep])
    return profile


def interpolate(profile, objects_rad, extend, nr_rad_bins):
    """Fill nan (or zero) entries of a (N, nbins) stack in place by linear interpolation over r = linspace(0, extend,
    nbins) (profile_2d.py:196-224); returns it."""
    return _fill_rows(profile, np.linspace(0, extend, nr_rad_bins))


def mean_and_interpolate(profile, objects_rad, extend, nr_rad_bins):
    """``interpolate``, then the average of the rows weighted by objects_rad ** 2 (profile_2d.py:227-259)."""
    _fill_rows(profile, np.linspace(0, extend, nr_rad_bins))
    return np.average(profile, axis=0, weights=objects_rad ** 2)


BLOCK = 256          # bootstrap block side in pixels (profile_2d.py:302)
REALISATIONS = 100   # bootstrap realisations (profile_2d.py:313)


def _blocks(mask, w):
    h, _ = mask.shape
    return mask.reshape(h // w, w, -1, w).swapaxes(1, 2).reshape(-1, w, w)


def bootstrapping(profiles, mean_profile, objects, npix, extend, nr_rad_bins):
    """Block-bootstrap errors of the weighted mean profile (profile_2d.py:278-359).  Each object tags pixel
    [x_pix, y_pix] of an npix^2 mask with its index + 1 (a later object overwrites an earlier one); the mask is cut into
    256^2 blocks; each of 100 realisations draws one block per block with np.random.randint (numpy's global state,
    realisation outer, block inner), stacks the tagged profiles, orders them by np.flip(np.argsort(radii)) and takes
    ``mean_and_interpolate``.  Returns the std (ddof 0) over realisations per bin, twice: np.squeeze of a (2, nbins)
    array."""
    npix = int(npix)
    if npix % BLOCK:
        raise ValueError(f"npix must be a multiple of {BLOCK}, got {npix}")
    xs, ys = objects["x_pix"].values, objects["y_pix"].values
    rad = objects["rad_pix"].values
    mask = np.zeros((npix, npix))
    for i in range(len(profiles)):
        mask[xs[i], ys[i]] = i + 1
    blocks = _blocks(mask, BLOCK)
    tags = [b[b != 0] for b in blocks]
    nblocks = len(blocks)
    draws = [[tags[np.random.randint(0, nblocks)] for _ in range(nblocks)] for _ in range(REALISATIONS)]
    means = np.zeros((REALISATIONS, nr_rad_bins))
    for j in range(REALISATIONS):
        idx = [int(t) for t in np.concatenate(draws[j]) - 1]
        stack = np.array([profiles[k] for k in idx])
        radii = np.array([rad[k] for k in idx])
        order = np.flip(np.argsort(radii), 0)
        if len(order) > 0:
            means[j] = mean_and_interpolate(stack[order], radii[order], extend, nr_rad_bins)
    std = np.array([np.std(means.T[i]) for i in range(nr_rad_bins)])
    return np.squeeze(np.array([std, std]))
