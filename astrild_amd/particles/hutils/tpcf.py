"""Two-point correlation function of a periodic box with astrild's API (src/astrild/particles/hutils/tpcf.py), the pair
counts on the GPU.  The reference hands the work to halotools (``s_mu_tpcf``, and ``tpcf`` / ``tpcf_multipole`` in its
commented-out halo code); halotools is not used here, and this module restates its behaviour as far as its published
source fixes it, without a check against the library itself:

* **Redshift-space shift** (``tpcf.py:74-97``): ``pos_s[:, los] += vel[:, los] / 100.``, then one wrap,
  ``> boxsize -> - boxsize`` and ``< 0 -> + boxsize``, in numpy's arithmetic for the input dtypes (float32 positions
  are shifted and wrapped in float32, then widened to float64).  The reference then swaps axis ``los`` with z for
  halotools; in a cubic box that changes no distance, so the pair geometry simply uses axis ``los`` as the line of
  sight.  ``los=None`` (the default of ``compute``) crashes in the reference; here it means 2, halotools' own line of
  sight.  ``space`` is ignored, as in the reference: ``compute`` is always redshift space.
* **Validation, as halotools does it**: after the shift every coordinate must lie in [0, boxsize]; the largest s edge
  must be below boxsize / 3; s edges strictly increasing and >= 0; mu edges strictly increasing within [0, 1].
  Otherwise ``ValueError``.
* **Pair geometry**: minimum image per axis, ``a = min(|x_i - x_j|, L - |x_i - x_j|)``;
  ``d^2 = (a_x^2 + a_y^2) + a_z^2`` and ``mu = a_los / sqrt(d^2)`` = |cos theta_LOS|, all fp64.  This port follows
  the cosine convention (older halotools releases are recalled to have defined mu through sin theta_LOS).
* **Binning**: halotools differences cumulative counts (``d <= s_k``, ``mu <= mu_l``, our reading of its source), so a
  pair lands in bin (k, l) when ``s_k^2 < d^2 <= s_{k+1}^2`` and ``mu_l < mu <= mu_{l+1}``.  A pair with mu exactly
  on the lowest mu edge (mu = 0 when that edge is 0) is in no bin; coincident objects (d = 0) never count.
* **Estimator**: analytic randoms in the periodic box (halotools with ``randoms=None`` and a ``period``):
  ``RR_kl = N^2 (4 pi / 3)(s_{k+1}^3 - s_k^3)(mu_{l+1} - mu_l) / L^3`` and ``DD`` = ordered pairs = 2 x the
  unordered counts.  With DR = RR and N_R = N every halotools estimator (Natural, Davis-Peebles, Hewett, Hamilton,
  Landy-Szalay) reduces to ``xi = DD / RR - 1``; all five names are accepted, anything else is a ``ValueError``.
  This arithmetic runs on the host in fp64 from the int64 counts.

``nthreads`` is accepted and ignored.  Cross-correlations, user randoms and non-periodic samples are not supported.
"""
from typing import Optional, Union

import numpy as np

ESTIMATORS = ("Natural", "Davis-Peebles", "Hewett", "Hamilton", "Landy-Szalay")


def _check_estimator(estimator):
    if estimator not in ESTIMATORS:
        raise ValueError(f"estimator {estimator!r}: one of {', '.join(ESTIMATORS)}")


def _xi(dd_unordered, n, boxsize, s_edges, mu_edges=None):
    """``2 DD / RR - 1`` with the analytic RR of a periodic box; ``mu_edges`` None: per s bin only."""
    s = np.asarray(s_edges, dtype=np.float64)
    shell = (4.0 * np.pi / 3.0) * (s[1:] ** 3 - s[:-1] ** 3)
    if mu_edges is not None:
        shell = np.outer(shell, np.diff(np.asarray(mu_edges, dtype=np.float64)))
    rr = float(n) * float(n) * shell / float(boxsize) ** 3
    with np.errstate(divide="ignore", invalid="ignore"):
        return 2.0 * dd_unordered.astype(np.float64) / rr - 1.0


def _counts(pos, boxsize, s_edges, mu_edges, vel, los):
    from ... import device as dev
    return dev.to_numpy(dev.tpcf_pair_counts(pos, boxsize, s_edges, mu_edges=mu_edges, vel=vel, los=los))


class TPCF:
    """Two Point Correlation Function in redshift space."""

    @staticmethod
    def compute(
        pos: np.ndarray,
        vel: np.ndarray,
        boxsize: float,
        space: str,
        s_range: Union[tuple, np.ndarray],
        mu_range: Union[tuple, np.ndarray],
        nthreads: int = 1,
        los: Optional[int] = None,
        return_counts: bool = False,
    ):
        """xi(s, mu) of a periodic box in redshift space.

        Args:
            pos, vel: (N, 3) positions [Mpc/h] and velocities [km/s]; numpy arrays or device tensors.
            space: ignored (always redshift space, as the reference).
            s_range: s edges, or a tuple (min, max) -> ``linspace(min, max, 40)``.
            mu_range: mu edges, or a tuple (min, max) -> ``sort(1 - geomspace(min, max, 40))``.
            los: line-of-sight axis; None means 2.
            return_counts: also return the int64 unordered pair counts.

        Returns:
            (s bin centres, mu edges, xi of shape (ns, nmu)) [, counts].
        """
        from ... import device as dev

        if type(s_range) == tuple:
            s_range = np.linspace(min(s_range), max(s_range), 40)
        if type(mu_range) == tuple:
            mu_range = np.sort(1.0 - np.geomspace(min(mu_range), max(mu_range), 40))
        if mu_range is None:
            raise ValueError("mu_range is required (redshift-space xi(s, mu))")
        s_range, mu_range = dev.check_tpcf_edges(s_range, mu_range, boxsize)
        out = TPCF.tpcf_s(pos, vel, s_range, mu_range, 2 if los is None else los, boxsize, nthreads,
                          return_counts=return_counts)
        centres = (s_range[1:] + s_range[:-1]) / 2.0
        if return_counts:
            return centres, mu_range, out[0], out[1]
        return centres, mu_range, out

    @staticmethod
    def tpcf_s(
        pos: np.ndarray,
        vel: np.ndarray,
        chi_range: np.ndarray,
        mu_range: np.ndarray,
        los: int = 2,
        boxsize: float = 500.0,
        nthreads: int = 1,
        return_counts: bool = False,
    ):
        """xi(s, mu) in redshift space (Landy-Szalay, analytic randoms): shape (len(chi_range) - 1,
        len(mu_range) - 1); with ``return_counts`` also the int64 unordered pair counts."""
        from ... import device as dev

        s, mu = dev.check_tpcf_edges(chi_range, mu_range, boxsize)
        if mu is None:
            raise ValueError("mu_range is required (redshift-space xi(s, mu))")
        dd = _counts(pos, boxsize, s, mu, vel, los)
        xi = _xi(dd, len(pos), boxsize, s, mu)
        return (xi, dd) if return_counts else xi


def tpcf_r(pos, rbins, period, estimator: str = "Natural", return_counts: bool = False):
    """Real-space xi(r) of a periodic box, the subset of halotools' ``tpcf`` the reference calls
    (``sample1``, ``rbins``, ``period``, ``estimator``; analytic randoms): shape (len(rbins) - 1,); with
    ``return_counts`` also the int64 unordered pair counts."""
    from ... import device as dev

    _check_estimator(estimator)
    r, _ = dev.check_tpcf_edges(rbins, None, period)
    dd = _counts(pos, period, r, None, None, 2)
    xi = _xi(dd, len(pos), period, r)
    return (xi, dd) if return_counts else xi


def tpcf_multipole(xi_s_mu, mu_bins, order: int = 0):
    """Legendre multipole of xi(s, mu) in halotools' form (recalled from its source, not checked against it):
    ``(2 l + 1) / 2 * sum_mu xi * dmu * (P_l(mu_c) + P_l(-mu_c))`` with mu_c the mu bin centres.  Host numpy."""
    xi = np.atleast_2d(np.asarray(xi_s_mu, dtype=np.float64))
    mu = np.atleast_1d(np.asarray(mu_bins, dtype=np.float64))
    order = int(order)
    if xi.shape[-1] != len(mu) - 1:
        raise ValueError(f"xi has {xi.shape[-1]} mu bins, mu_bins gives {len(mu) - 1}")
    centres = (mu[:-1] + mu[1:]) / 2.0
    coef = np.zeros(order + 1)
    coef[order] = 1.0
    leg = np.polynomial.legendre.legval(centres, coef) + np.polynomial.legendre.legval(-centres, coef)
    return (2.0 * order + 1.0) / 2.0 * np.sum(xi * np.diff(mu) * leg, axis=1)
