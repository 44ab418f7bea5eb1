"""Mean pairwise velocity from transverse velocities with astrild's API
(src/astrild/particles/hutils/mean_pairwise_velocity.py), the pair loop on the GPU.

``mean_pv_from_tv`` keeps the reference's semantics, quirks included:

* ``binnr = len(bins)`` (not ``len(bins) - 1``) and ``binwidth = bins[1] - bins[0]``; a pair goes to bin
  ``int(|r_i - r_j| / binwidth)`` when that is below ``binnr``, so the reach is ``binnr * binwidth`` and uneven edges
  are ignored beyond the first width.
* Without angles, ``theta1 = arctan(x / z)`` and ``theta2 = arctan(y / z)`` plus 10 degrees; given angles are degrees
  when ``max(theta1) > 2 pi``, radians otherwise.
* Empty bins are dropped from the estimate: ``pest = nom[denom > 0] / denom[denom > 0]``, so ``len(pest)`` can be
  below ``len(rsep)``.  Coincident objects add NaN to bin 0, which then drops out the same way.

There is no object cap (the reference refuses more than 50 000).  ``multithreading`` and ``Nthreads`` are accepted
and ignored.

``mean_pv_z_sign`` and ``mean_pv_radial`` are the pairwise-velocity histograms of the reference's
particles/utils_cython/pairwise_velocity.pyx: the pair counts per (separation bin, velocity bin), from which the mean
streaming velocity v12(r) and the pairwise dispersion sigma12(r) follow.  All pair arithmetic is float64, op by op.
For the unordered pair i < j of original indices:

* Differences are ``x_j - x_i`` per axis and ``d = sqrt((dx dx + dy dy) + dz dz)``.
* The pair is seen iff ``d <= float64(float32(r))`` (the reference declares ``float r``: with ``r = 4.1`` a pair at
  exactly 4.1 is out) and ``ffirst <= i < ssecond``, the reference's chunking of its i loop; chunks over a partition of
  [0, N) sum to the whole.  ``ValueError`` unless ``0 <= ffirst <= ssecond <= N``.
* ``z_sign``: ``v12 = (vz_j - vz_i) * sign(z_j - z_i)`` with sign -1, 0 or +1 (equal z gives ``v12 = +-0``);
  ``radial``: ``v12 = (((vx_j - vx_i) dx + (vy_j - vy_i) dy) + (vz_j - vz_i) dz) / d``.  The reference's
  ``mean_pv_radial`` does not run as shipped (it hands a 1-D point to ``BallTree.query_radius``), so it is defined here
  as ``mean_pv_z_sign`` with the radial velocity in place of the line-of-sight one.
* The binned quantities are rounded to float32 like the reference's ``cdef float diff, dist``:
  ``ds = float32(d / dist_width)`` and ``vs = float32(v12 / vel_width + vel_bin // 2)``.  The pair is counted in
  ``counter[int(ds), int(vs)]`` iff ``int(ds) < dist_bin`` and ``0 <= vs < vel_bin``; every other seen pair (a NaN
  from coincident objects in ``radial`` included) adds 1 to ``outside``, the reference's ``rubbish_counter``.  The
  reference raises ``IndexError`` for ``vs == vel_bin`` and ``int(ds) == dist_bin``; counting those pairs in ``outside``
  is the one deliberate difference.  ``dist_width`` and ``vel_width`` are extensions; at their default 1.0 the rule is
  the reference's own.
* Moments (``return_moments``, an extension): per row ``a < dist_bin`` over the seen pairs with finite v12, whatever
  ``vs`` is, ``count``, ``mean = sum(v12) / count`` and ``sigma = sqrt(sum(v12^2) / count - mean^2)`` of the float64
  v12, neither scaled nor rounded; NaN for empty rows.

Nothing is printed (the reference prints every counted pair), ``tree`` is accepted and ignored, fewer than two objects
give zeros, and the problem is non-periodic, as in the reference.
"""
from typing import Optional

import numpy as np


def mean_pv_from_tv(
    pos_cart: np.ndarray,
    vel_ang: np.ndarray,
    bins: np.ndarray,
    theta1: Optional[np.ndarray] = None,
    theta2: Optional[np.ndarray] = None,
    multithreading: bool = True,
    Nthreads=None,
    return_counts: bool = False,
):
    """Mean pairwise velocity estimated from the transverse velocity components (Yasini et al. 2018,
    arxiv:1812.04241).

    Args:
        pos_cart: (N, 3) cartesian positions [Mpc/h]; numpy array or device tensor.
        vel_ang: (N, 2) RA and DEC velocities [km/s].
        bins: distances [Mpc/h] of the histogram edges.
        theta1, theta2: RA and DEC of the objects [deg or rad], or None.
        return_counts: also return the pairs per bin (all ``len(bins)`` bins).

    Returns:
        rsep: bin centres [Mpc/h]; pest: the estimate of the bins with pairs (numpy float64);
        with ``return_counts``, the int64 pair counts as a third element.
    """
    from ... import device as dev

    bins = np.asarray(bins)
    binnr = len(bins)
    binwidth = float(np.diff(bins)[0])
    nom, denom, counts = dev.pairwise_tv(pos_cart, vel_ang, binnr, binwidth, theta1=theta1, theta2=theta2)
    nom, denom, counts = dev.to_numpy(nom), dev.to_numpy(denom), dev.to_numpy(counts)
    keep = denom > 0
    pest = nom[keep] / denom[keep]
    rsep = make_rsep(binnr, binwidth)
    if return_counts:
        return rsep, pest, counts
    return rsep, pest


def _mean_pv_pdf(kind, ppos, vvel, ffirst, ssecond, r, dist_bin, vel_bin, dist_width, vel_width, return_outside,
                 return_moments):
    from ... import device as dev

    res = dev.pairwise_velocity_pdf(ppos, vvel, r, dist_bin, vel_bin, kind, dist_width=dist_width, vel_width=vel_width,
                                    ffirst=ffirst, ssecond=ssecond, moments=return_moments)
    counter = dev.to_numpy(res[0]).astype(np.float64).reshape(-1)
    out = [counter]
    if return_outside:
        out.append(int(res[1].item()))
    if return_moments:
        count, s1, s2 = (dev.to_numpy(t) for t in res[2])
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = s1 / count
            sigma = np.sqrt(s2 / count - mean * mean)
        out.append({"count": count, "mean": mean, "sigma": sigma, "s1": s1, "s2": s2})
    return out[0] if len(out) == 1 else tuple(out)


def mean_pv_z_sign(tree, ppos, vvel, ffirst, ssecond, r, dist_bin, vel_bin, *, dist_width=1.0, vel_width=1.0,
                   return_outside=False, return_moments=False):
    """Pairwise-velocity histogram along the z axis, the line of sight:
    ``v12 = (vz_j - vz_i) * sign(z_j - z_i)`` (pairwise_velocity.pyx: mean_pv_z_sign).

    Args:
        tree: accepted and ignored (the reference's BallTree); may be None.
        ppos, vvel: (N, 3) positions and velocities; numpy arrays or device tensors.
        ffirst, ssecond: the rows i of the pair loop, ``ffirst <= i < ssecond``.
        r: reach of the pair search, rounded to float32 as in the reference.
        dist_bin, vel_bin: number of separation and velocity bins; velocities run from ``-(vel_bin // 2)``.
        dist_width, vel_width: bin widths (the reference's are 1).
        return_outside: also return the number of seen pairs that fell outside the histogram.
        return_moments: also return ``{"count", "mean", "sigma", "s1", "s2"}`` per separation bin.

    Returns:
        counter: the flattened float64 array of ``dist_bin * vel_bin`` pair counts, as the reference returns it;
        then ``outside`` and the moments when asked for.
    """
    return _mean_pv_pdf("z_sign", ppos, vvel, ffirst, ssecond, r, dist_bin, vel_bin, dist_width, vel_width,
                        return_outside, return_moments)


def mean_pv_radial(tree, ppos, vvel, ffirst, ssecond, r, dist_bin, vel_bin, *, dist_width=1.0, vel_width=1.0,
                   return_outside=False, return_moments=False):
    """Pairwise-velocity histogram along the separation vector: ``v12 = (v_j - v_i) . (r_j - r_i) / |r_j - r_i|``
    (pairwise_velocity.pyx: mean_pv_radial).  Arguments and returns as ``mean_pv_z_sign``."""
    return _mean_pv_pdf("radial", ppos, vvel, ffirst, ssecond, r, dist_bin, vel_bin, dist_width, vel_width,
                        return_outside, return_moments)


def make_rsep(binnr: int, binwidth: float) -> np.ndarray:
    """Bin centres ``(i + 1/2) binwidth``, i < binnr, of the histogram of ``mean_pv_from_tv``."""
    half = binwidth / 2.0
    return np.linspace(0.0, binwidth * (binnr - 1), binnr) + half


def make_rsep_uneven_bins(bin_edges: np.ndarray) -> np.ndarray:
    """Bin centres of arbitrary edges: the midpoints of consecutive edges."""
    e = np.asarray(bin_edges)
    return (e[:-1] + e[1:]) / 2.0
