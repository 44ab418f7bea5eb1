"""numpy oracle of the 2D radial profiles (the reference's profiles/profile_2d.py), written independently of the product:
every pixel's annulus index comes from numpy's own per-pixel expression, not from the product's integer thresholds.

Rules restated (from_map, :10-59 / profiling, :92-153), per object with r = int(rad_pix), x = int(x_pix), y = int(y_pix):
  1. R = int(ceil(r * extend)); offsets a, b in [-R, R) on both axes.
  2. eta = (sqrt(a^2 + b^2) / r / (extend / nbins)).astype(int) with int64 d2, float64 sqrt and divisions; only
     eta < nbins is read.
  3. pixel (a, b) adds map[y + a, x + b] (widened to float64) to annulus eta; an index i in [-n, 0) reads i + n, one
     outside [-n, n) raises IndexError.
  4. values = sums / counts, where counts lists the counts of the annuli present in ascending order, then zeros.
  5. radii = midpoints of linspace(0, extend, nbins + 1).
The host statistics (interpolate, mean_and_interpolate, bootstrapping) follow the reference's loop structure.
"""
import numpy as np


def annulus_index(d2, r, extend, nbins):
    return (np.sqrt(np.asarray(d2, dtype=np.int64)) / r / (extend / nbins)).astype(int)


def object_sums(skymap, x, y, r, extend, nbins):
    """True per-annulus (sums, counts) of one object; sums added with np.bincount (float64)."""
    R = int(np.ceil(r * extend))
    off = np.arange(-R, R, dtype=np.int64)
    a, b = np.meshgrid(off, off, indexing="ij")
    eta = annulus_index(a * a + b * b, r, extend, nbins)
    sel = eta < nbins
    rows, cols = y + a[sel], x + b[sel]
    ny, nx = skymap.shape
    for idx, n, axis in ((rows, ny, 0), (cols, nx, 1)):
        if len(idx) and (idx.min() < -n or idx.max() >= n):
            raise IndexError(f"index out of bounds for axis {axis} with size {n}")
    vals = np.asarray(skymap)[rows, cols].astype(np.float64)
    sums = np.bincount(eta[sel], weights=vals, minlength=nbins)[:nbins]
    counts = np.bincount(eta[sel], minlength=nbins)[:nbins].astype(np.int64)
    return sums, counts


def aligned(sums, counts):
    """Rule 4: nonzero counts packed to the front, then numpy's division (nan for 0/0, inf for x/0)."""
    present = counts[counts != 0].astype(np.float64)
    packed = np.concatenate([present, np.zeros(len(counts) - len(present))])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(sums, dtype=np.float64) / packed


def radii(extend, nbins):
    e = np.linspace(0, extend, nbins + 1)
    return 0.5 * (e[1:] + e[:-1])


def from_map(x_pix, y_pix, rad_pix, skymap, extend, nbins):
    """(values, sums, counts, radii) of a catalogue; int() truncation of x, y, r as in the reference."""
    S, C, V = [], [], []
    for x, y, r in zip(x_pix, y_pix, rad_pix):
        s, c = object_sums(skymap, int(x), int(y), int(r), extend, nbins)
        S.append(s)
        C.append(c)
        V.append(aligned(s, c))
    return np.array(V), np.array(S), np.array(C), radii(extend, nbins)


def fill(profile, extend, nbins):
    r = np.linspace(0, extend, nbins)
    nans = np.argwhere(np.isnan(profile))
    if len(nans) > 0:
        for i in range(len(nans)):
            profile[nans[i, 0], nans[i, 1]] = 0
        for i in range(len(nans)):
            row = profile[nans[i, 0]]
            profile[nans[i, 0]] = np.interp(r, r[row != 0], row[row != 0])
    elif len(np.argwhere(profile == 0)):
        zeros = np.argwhere(profile == 0)
        for i in range(len(profile) - zeros[0, 0]):
            row = profile[zeros[i, 0]]
            profile[zeros[i, 0]] = np.interp(r, r[row != 0], row[row != 0])
    return profile


def mean_and_interpolate(profile, rad, extend, nbins):
    fill(profile, extend, nbins)
    return np.average(profile, axis=0, weights=rad ** 2)


def bootstrapping(profiles, x_pix, y_pix, rad_pix, npix, extend, nbins):
    mask = np.zeros((npix, npix))
    for i in range(len(profiles)):
        mask[x_pix[i], y_pix[i]] = i + 1
    w = 256
    blocks = mask.reshape(npix // w, w, -1, w).swapaxes(1, 2).reshape(-1, w, w)
    tags = [blk[np.nonzero(blk)] for blk in blocks]
    picks = []
    for _ in range(100):
        picks.append([tags[np.random.randint(0, len(blocks))] for _ in range(len(blocks))])
    means = np.zeros((100, nbins))
    for j in range(100):
        k = (np.concatenate(picks[j]) - 1).astype(int)
        if len(k) == 0:
            continue
        prof = np.array([profiles[i] for i in k])
        rad = np.array([rad_pix[i] for i in k])
        order = np.flip(np.argsort(rad), 0)
        means[j] = mean_and_interpolate(prof[order], rad[order], extend, nbins)
    sd = np.array([np.std(means.T[i]) for i in range(nbins)])
    return np.squeeze(np.array([sd, sd]))
