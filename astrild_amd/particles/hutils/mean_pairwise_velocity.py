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


def make_rsep(binnr: int, binwidth: float) -> np.ndarray:
    """Bin centres ``(i + 1/2) binwidth``, i < binnr, of the histogram of ``mean_pv_from_tv``."""
    half = binwidth / 2.0
    return np.linspace(0.0, binwidth * (binnr - 1), binnr) + half


def make_rsep_uneven_bins(bin_edges: np.ndarray) -> np.ndarray:
    """Bin centres of arbitrary edges: the midpoints of consecutive edges."""
    e = np.asarray(bin_edges)
    return (e[:-1] + e[1:]) / 2.0
