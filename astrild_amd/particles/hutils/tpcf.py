"""Two-point correlation functions with astrild's API (src/astrild/particles/hutils/tpcf.py): one or two samples, in a
periodic box with analytic or user randoms, or with open boundaries and user randoms; the pair counts on the GPU. The reference hands the work to halotools (``s_mu_tpcf``, and ``tpcf`` / ``tpcf_multipole`` in its
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

* **Two samples** (``sample2=`` of ``tpcf_r`` / ``s_mu_tpcf``, ``pos2=`` / ``vel2=`` of ``TPCF``; the reference's
  halo code splits a catalogue at a mass threshold and correlates the halves this way, ``stats_subfind.py:155-218``):
  as halotools returns them, ``xi_11`` without a second sample; with one, ``(xi_11, xi_12, xi_22)``, or ``xi_12``
  alone with ``do_auto=False``, or ``(xi_11, xi_22)`` with ``do_cross=False``; both flags false is a ``ValueError``.
  The cross counts ``D1D2`` are all pairs (i of sample 1, j of sample 2), with the geometry and bins above; coincident
  points of the two samples (d = 0) never count.  In ``TPCF`` sample 2 is shifted and wrapped like sample 1.
* **Analytic randoms with two samples** (``period`` given, no ``randoms``): the auto terms are the one-sample path
  above, unchanged; the cross term is ``D1D2 / (N1 N2 v / L^3) - 1`` with ``v`` the shell volume times ``dmu``, for
  every estimator name.
* **User randoms** (``randoms=``; they have no velocities and are never shifted): with ``period`` every term is counted
  with the minimum image, with ``period=None`` every term with open boundaries (plain separations; every coordinate
  must be finite, and the top s edge is not bounded by a box).  ``period=None`` without ``randoms`` is a ``ValueError``.
  The estimators, halotools' ``_TP_estimator`` as recalled from its source and not checked against the library: with
  ``DD`` the ordered data pairs (2 x the unordered counts for an auto term, all pairs for the cross term),
  ``RR`` = 2 x the unordered random pairs, ``DR`` all data-random pairs and ``Na, Nb, NR`` the sample sizes,

  - Natural: ``NR NR / (Na Nb) DD / RR - 1``
  - Davis-Peebles: ``NR / Nb DD / DR - 1``
  - Hewett: ``NR NR / (Na Nb) DD / RR - NR / Na DR / RR``
  - Hamilton: ``DD RR / (DR DR) - 1``
  - Landy-Szalay: ``NR NR / (Na Nb) DD / RR - NR / Na 2 DR / RR + 1``

  The auto terms use (a, b) = (1, 1) or (2, 2) with their own ``DaR``; the cross term uses (1, 2) with ``D1R`` only,
  as halotools is recalled to do.  The symmetric cross Landy-Szalay, ``(D1D2 - D1R - D2R + RR) / RR`` with each count
  normalised by its number of pairs, can be formed from ``return_counts``.  Host fp64 arithmetic from the int64 counts;
  an empty ``RR`` or ``DR`` bin gives inf / nan as numpy does, not an exception.
* **``return_counts``**: with a second sample or randoms (and always in ``s_mu_tpcf``) a dict of the raw int64 counts
  that were needed, under ``D1D1, D1D2, D2D2, D1R, D2R, RR`` (unordered pairs for ``D1D1, D2D2, RR``); otherwise, as
  before, the array of unordered ``D1D1`` counts.

* **Jackknife errors** (``tpcf_jackknife``, halotools' function of that name): xi with the covariance matrix of a
  leave-one-subvolume-out resampling, every leave-one-out count of a term from one pass over its pairs; the weights,
  the identity behind the single pass and what is recalled rather than checked are in its docstring.

* **xi(r_p, pi) and w_p(r_p)** (``rp_pi_tpcf``, ``wp``, ``rp_pi_tpcf_jackknife``, ``wp_jackknife``: halotools'
  functions of those names, which the reference never calls): with ``los`` the line of sight and a < b the two other
  axes, ``p_c`` the per-axis separation above (minimum image with a ``period``), ``rp^2 = p_a^2 + p_b^2`` and
  ``pi = p_los``, fp64.  **Binning**: halotools differences the cumulative counts of ``npairs_xy_z`` (``r_p <= rp_k``
  and ``pi <= pi_l``; recalled from its source, not checked against the library), so a pair lands in bin (k, l) when
  ``rp_k^2 < rp^2 <= rp_{k+1}^2`` and ``pi_l < pi <= pi_{l+1}``, the r_p edges squared once in fp64 and the pi edges
  compared as given.  A pair with pi exactly on the lowest pi edge (pi = 0 when that edge is 0) is in no bin; a pair
  with r_p = 0 is in no bin when the lowest r_p edge is 0; coincident objects never count.  Both sets of edges are
  finite, >= 0 and strictly increasing, and with a ``period`` both top edges are below period / 3.  **Bin volume**
  (analytic randoms): ``RR_kl = N^2 pi (rp_{k+1}^2 - rp_k^2) 2 (pi_{l+1} - pi_l) / L^3``, the two cylinder shells on
  either side of an object, and ``N1 N2`` for the cross term; everything else - the return conventions, user randoms,
  open boundaries, the five estimators and ``return_counts`` - is what is said above for ``s_mu_tpcf``, from the same
  ordered-count conventions.  ``w_p = 2 sum_l xi(r_p, pi_l) dpi_l`` (``wp_from_xi``) over ``pi_bins``, by default
  halotools' single bin ``[0, pi_max]``; that halotools sums xi this way is recalled, not checked.

``nthreads`` / ``num_threads`` and ``seed`` are accepted and ignored.
"""
from typing import Optional, Union

import numpy as np

ESTIMATORS = ("Natural", "Davis-Peebles", "Hewett", "Hamilton", "Landy-Szalay")


def _check_estimator(estimator):
    if estimator not in ESTIMATORS:
        raise ValueError(f"estimator {estimator!r}: one of {', '.join(ESTIMATORS)}")


def _bin_volume(s_edges, mu_edges=None, rppi=False):
    """The volume that a bin offers the second object of an ordered pair: the shell ``(4 pi / 3)(s_{k+1}^3 - s_k^3)``,
    times ``dmu`` with ``mu_edges``; ``rppi``: the two cylinder shells on either side of the first object,
    ``pi (rp_{k+1}^2 - rp_k^2) x 2 (pi_{l+1} - pi_l)``."""
    s = np.asarray(s_edges, dtype=np.float64)
    if rppi:
        return np.outer(np.pi * (s[1:] ** 2 - s[:-1] ** 2), 2.0 * np.diff(np.asarray(mu_edges, dtype=np.float64)))
    shell = (4.0 * np.pi / 3.0) * (s[1:] ** 3 - s[:-1] ** 3)
    if mu_edges is not None:
        shell = np.outer(shell, np.diff(np.asarray(mu_edges, dtype=np.float64)))
    return shell


def _xi(dd_unordered, n, boxsize, s_edges, mu_edges=None, rppi=False):
    """``2 DD / RR - 1`` with the analytic RR of a periodic box over ``_bin_volume``; ``mu_edges`` None: per s bin only."""
    rr = float(n) * float(n) * _bin_volume(s_edges, mu_edges, rppi) / float(boxsize) ** 3
    with np.errstate(divide="ignore", invalid="ignore"):
        return 2.0 * dd_unordered.astype(np.float64) / rr - 1.0


def _counts(pos, boxsize, s_edges, mu_edges, vel, los, rppi=False):
    from ... import device as dev
    if rppi:
        return dev.to_numpy(dev.rp_pi_pair_counts(pos, boxsize, s_edges, mu_edges, vel=vel, los=los))
    return dev.to_numpy(dev.tpcf_pair_counts(pos, boxsize, s_edges, mu_edges=mu_edges, vel=vel, los=los))


def _cross(pos1, pos2, boxsize, s_edges, mu_edges, vel1=None, vel2=None, los=2, rppi=False):
    from ... import device as dev
    count = dev.rp_pi_cross_counts if rppi else dev.tpcf_cross_counts
    return dev.to_numpy(count(pos1, pos2, s_edges, mu_edges, boxsize=boxsize, vel1=vel1, vel2=vel2, los=los))


def _estimate(estimator, dd, dr, rr, na, nb, nr):
    """halotools' ``_TP_estimator`` from ordered pair counts (module docstring); ``dr`` / ``rr`` None when the
    estimator does not use them."""
    na, nb, nr = np.float64(na), np.float64(nb), np.float64(nr)      # a size of 0 gives inf / nan, not an exception
    with np.errstate(divide="ignore", invalid="ignore"):
        if estimator == "Natural":
            return (nr * nr) / (na * nb) * dd / rr - 1.0
        if estimator == "Davis-Peebles":
            return nr / nb * dd / dr - 1.0
        if estimator == "Hewett":
            return (nr * nr) / (na * nb) * dd / rr - nr / na * dr / rr
        if estimator == "Hamilton":
            return dd * rr / (dr * dr) - 1.0
        return (nr * nr) / (na * nb) * dd / rr - nr / na * 2.0 * dr / rr + 1.0


_USES_DR = ("Davis-Peebles", "Hewett", "Hamilton", "Landy-Szalay")
_USES_RR = ("Natural", "Hewett", "Hamilton", "Landy-Szalay")


def _correlate(pos1, pos2, randoms, s, mu, period, estimator, do_auto, do_cross, vel1=None, vel2=None, los=2,
               rppi=False):
    """The xi terms asked for and the dict of raw counts; ``s`` / ``mu`` are checked edges - with ``rppi`` the r_p / pi
    edges, and the counters and the bin volume are those of (r_p, pi)."""
    _check_estimator(estimator)
    if not (do_auto or do_cross):
        raise ValueError("do_auto and do_cross are both False: nothing to compute")
    if period is None and randoms is None:
        raise ValueError("period=None (open boundaries) needs randoms")
    auto1 = do_auto or pos2 is None
    auto2 = do_auto and pos2 is not None
    cross = do_cross and pos2 is not None
    n1, n2 = len(pos1), 0 if pos2 is None else len(pos2)
    f64 = lambda c: c.astype(np.float64)

    def unordered(pos, vel):
        if period is not None:
            return _counts(pos, period, s, mu, vel, los, rppi)
        return _cross(pos, None, None, s, mu, vel1=vel, los=los, rppi=rppi)

    c = {}
    if auto1:
        c["D1D1"] = unordered(pos1, vel1)
    if cross:
        c["D1D2"] = _cross(pos1, pos2, period, s, mu, vel1=vel1, vel2=vel2, los=los, rppi=rppi)
    if auto2:
        c["D2D2"] = unordered(pos2, vel2)
    xi = {}
    if randoms is None:
        if auto1:
            xi[11] = _xi(c["D1D1"], n1, period, s, mu, rppi)
        if auto2:
            xi[22] = _xi(c["D2D2"], n2, period, s, mu, rppi)
        if cross:
            shell = _bin_volume(s, mu, rppi)
            with np.errstate(divide="ignore", invalid="ignore"):
                xi[12] = f64(c["D1D2"]) / (float(n1) * float(n2) * shell / float(period) ** 3) - 1.0
    else:
        nr = len(randoms)
        dr1 = dr2 = rr = None
        if estimator in _USES_DR:
            c["D1R"] = _cross(pos1, randoms, period, s, mu, vel1=vel1, los=los, rppi=rppi)
            dr1 = f64(c["D1R"])
            if auto2:
                c["D2R"] = _cross(pos2, randoms, period, s, mu, vel1=vel2, los=los, rppi=rppi)
                dr2 = f64(c["D2R"])
        if estimator in _USES_RR:
            c["RR"] = unordered(randoms, None)
            rr = 2.0 * f64(c["RR"])
        if auto1:
            xi[11] = _estimate(estimator, 2.0 * f64(c["D1D1"]), dr1, rr, n1, n1, nr)
        if cross:
            xi[12] = _estimate(estimator, f64(c["D1D2"]), dr1, rr, n1, n2, nr)
        if auto2:
            xi[22] = _estimate(estimator, 2.0 * f64(c["D2D2"]), dr2, rr, n2, n2, nr)
    if pos2 is None:
        out = xi[11]
    elif do_auto and do_cross:
        out = (xi[11], xi[12], xi[22])
    elif do_cross:
        out = xi[12]
    else:
        out = (xi[11], xi[22])
    return out, c


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
        pos2=None,
        vel2=None,
        randoms=None,
        do_auto: bool = True,
        do_cross: bool = True,
        estimator: str = "Landy-Szalay",
    ):
        """xi(s, mu) of a periodic box in redshift space.

        Args:
            pos, vel: (N, 3) positions [Mpc/h] and velocities [km/s]; numpy arrays or device tensors.
            space: ignored (always redshift space, as the reference).
            s_range: s edges, or a tuple (min, max) -> ``linspace(min, max, 40)``.
            mu_range: mu edges, or a tuple (min, max) -> ``sort(1 - geomspace(min, max, 40))``.
            los: line-of-sight axis; None means 2.
            return_counts: also return the int64 unordered pair counts (a dict of counts with ``pos2`` or ``randoms``).
            pos2, vel2: a second sample, shifted and wrapped like the first.
            randoms: (NR, 3) random positions, not shifted; None: analytic randoms.
            do_auto, do_cross, estimator: as ``s_mu_tpcf`` (module docstring).

        Returns:
            (s bin centres, mu edges, xi of shape (ns, nmu)) [, counts]; with ``pos2``, xi is what ``s_mu_tpcf``
            returns for two samples.
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
                          return_counts=return_counts, pos2=pos2, vel2=vel2, randoms=randoms, do_auto=do_auto,
                          do_cross=do_cross, estimator=estimator)
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
        pos2=None,
        vel2=None,
        randoms=None,
        do_auto: bool = True,
        do_cross: bool = True,
        estimator: str = "Landy-Szalay",
    ):
        """xi(s, mu) in redshift space (Landy-Szalay, analytic randoms): shape (len(chi_range) - 1,
        len(mu_range) - 1); with ``return_counts`` also the int64 unordered pair counts.  With ``pos2`` / ``vel2``
        and / or ``randoms``: the terms of ``s_mu_tpcf`` for the shifted samples, and a dict of counts."""
        from ... import device as dev

        _check_estimator(estimator)
        s, mu = dev.check_tpcf_edges(chi_range, mu_range, boxsize)
        if mu is None:
            raise ValueError("mu_range is required (redshift-space xi(s, mu))")
        if pos2 is not None or randoms is not None:
            if pos2 is None and vel2 is not None:
                raise ValueError("vel2 given without pos2")
            xi, c = _correlate(pos, pos2, randoms, s, mu, boxsize, estimator, do_auto, do_cross, vel1=vel, vel2=vel2,
                               los=los)
            return (xi, c) if return_counts else xi
        dd = _counts(pos, boxsize, s, mu, vel, los)
        xi = _xi(dd, len(pos), boxsize, s, mu)
        return (xi, dd) if return_counts else xi


def tpcf_r(pos, rbins, period=None, estimator: str = "Natural", return_counts: bool = False, sample2=None, randoms=None,
           do_auto: bool = True, do_cross: bool = True):
    """Real-space xi(r), halotools' ``tpcf`` (``sample1``, ``rbins``, ``period``, ``estimator``, ``sample2``,
    ``randoms``, ``do_auto``, ``do_cross``; module docstring): each term of shape (len(rbins) - 1,).  With
    ``return_counts`` also the int64 unordered pair counts of ``pos``, or, with ``sample2`` or ``randoms``, the dict of
    raw counts."""
    from ... import device as dev

    _check_estimator(estimator)
    if sample2 is not None or randoms is not None or period is None:
        return s_mu_tpcf(pos, rbins, None, sample2=sample2, randoms=randoms, period=period, do_auto=do_auto,
                         do_cross=do_cross, estimator=estimator, return_counts=return_counts)
    if not (do_auto or do_cross):
        raise ValueError("do_auto and do_cross are both False: nothing to compute")
    r, _ = dev.check_tpcf_edges(rbins, None, period)
    dd = _counts(pos, period, r, None, None, 2)
    xi = _xi(dd, len(pos), period, r)
    return (xi, dd) if return_counts else xi


def s_mu_tpcf(sample1, s_bins, mu_bins, sample2=None, randoms=None, period=None, do_auto: bool = True,
              do_cross: bool = True, estimator: str = "Natural", los: int = 2, return_counts: bool = False):
    """xi(s, mu) with halotools' ``s_mu_tpcf`` arguments (module docstring): each term of shape (len(s_bins) - 1,
    len(mu_bins) - 1), or (len(s_bins) - 1,) with ``mu_bins=None``.  No redshift-space shift: the samples are used as
    given, with axis ``los`` the line of sight.  With ``return_counts`` also the dict of raw int64 counts."""
    from ... import device as dev

    _check_estimator(estimator)
    if not (do_auto or do_cross):
        raise ValueError("do_auto and do_cross are both False: nothing to compute")
    if period is None and randoms is None:
        raise ValueError("period=None (open boundaries) needs randoms")
    s, mu = dev.check_tpcf_edges(s_bins, mu_bins, period, periodic=period is not None)
    xi, c = _correlate(sample1, sample2, randoms, s, mu, period, estimator, do_auto, do_cross, los=los)
    return (xi, c) if return_counts else xi


def jackknife_tags(pos, nsub, lo, hi):
    """The jackknife region of every object, int32 (N,): per axis ``i = floor((x - lo) / ((hi - lo) / nsub))`` in fp64
    with true divisions, clamped to ``[0, nsub - 1]`` on both sides (``x == hi``, a point outside ``[lo, hi]`` and a NaN
    belong to a border region), and ``tag = (i_x nsub_y + i_y) nsub_z + i_z``: numpy's C order, halotools' label
    minus one.  ``nsub``, ``lo``, ``hi``: three values each.  Host numpy; the rule of ``ast_tpcf_jk_prepare``."""
    x = np.asarray(pos).astype(np.float64).reshape(-1, 3)
    nsub = np.asarray(nsub, dtype=np.int64).reshape(3)
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
    with np.errstate(divide="ignore", invalid="ignore"):
        i = np.floor((x - lo) / ((hi - lo) / nsub.astype(np.float64)))
    i = np.minimum(np.where(i >= 0.0, i, 0.0), (nsub - 1).astype(np.float64)).astype(np.int64)
    return ((i[:, 0] * nsub[1] + i[:, 1]) * nsub[2] + i[:, 2]).astype(np.int32)


def jackknife_from_counts(c, n1, m1, nr, mr, n2=None, m2=None, estimator="Natural", do_auto=True, do_cross=True,
                          transform=None):
    """xi of the full sample and its jackknife covariance from integer counts, on the host in fp64 (no GPU).

    ``c``: term -> ``(counts, ends)`` under ``D1D1, D1D2, D2D2, D1R, D2R, RR`` (those the estimator and the flags need),
    ``counts`` of shape B and ``ends`` of (n, *B) as ``device.tpcf_jackknife_counts`` returns them; ``n1, n2, nr`` the
    sample sizes and ``m1, m2, mr`` the objects per region, (n,) each.  Region k left out: sizes ``N - m[k]``; ordered
    auto pairs ``2 counts - ends[k]``; cross and data-random pairs ``(2 counts - ends[k]) / 2``; each xi_k by
    ``_estimate`` as for the full sample.  ``cov = (n - 1) / n sum_k (xi_k - mean)(xi_k - mean)^T`` over all n regions,
    empty ones included, mean the mean of the xi_k, xi flattened per bin.  Returns, in halotools' order, ``(xi, cov)``
    for one sample, ``(xi_11, xi_12, xi_22, cov_11, cov_12, cov_22)`` for two, ``(xi_12, cov_12)`` with ``do_cross``
    only and ``(xi_11, xi_22, cov_11, cov_22)`` with ``do_auto`` only; xi of shape B, cov (prod B, prod B).
    ``transform``: a function applied to the full-sample xi and to every xi_k (each of shape B) before the covariance,
    which is then that of the transformed statistic (``wp_jackknife``: w_p from xi(r_p, pi))."""
    _check_estimator(estimator)
    if not (do_auto or do_cross):
        raise ValueError("do_auto and do_cross are both False: nothing to compute")
    two = n2 is not None
    f64 = lambda a: np.asarray(a).astype(np.float64)
    n = len(np.asarray(mr).reshape(-1))
    left = {key: float(size) - f64(m).reshape(-1) for key, size, m in (("1", n1, m1), ("2", n2, m2), ("R", nr, mr))
            if m is not None}
    full = {"1": n1, "2": n2, "R": nr}

    def ordered(term, k=None):
        """Ordered pairs of a term, or None when it was not counted: auto terms 2 x unordered, the others as counted."""
        if term not in c:
            return None
        counts, ends = f64(c[term][0]), c[term][1]
        auto = term in ("D1D1", "D2D2", "RR")
        if k is None:
            return 2.0 * counts if auto else counts
        loo = 2.0 * counts - f64(ends[k])
        return loo if auto else loo / 2.0

    def term(a, b):
        dd, dr = ("D1D2" if a != b else f"D{a}D{a}"), f"D{a}R"
        stat = transform if transform is not None else (lambda x: x)
        xi = stat(_estimate(estimator, ordered(dd), ordered(dr), ordered("RR"), full[a], full[b], nr))
        xik = np.stack([np.asarray(stat(_estimate(estimator, ordered(dd, k), ordered(dr, k), ordered("RR", k),
                                                  left[a][k], left[b][k], left["R"][k]))).reshape(-1)
                        for k in range(n)])
        with np.errstate(invalid="ignore"):
            d = xik - xik.mean(axis=0)
            return xi, (n - 1.0) / n * (d.T @ d)

    if not two:
        return term("1", "1")
    out = {}
    if do_auto:
        out[11], out[22] = term("1", "1"), term("2", "2")
    if do_cross:
        out[12] = term("1", "2")
    keys = [k for k in (11, 12, 22) if k in out]
    if keys == [12]:
        return out[12]
    return tuple(out[k][0] for k in keys) + tuple(out[k][1] for k in keys)


def tpcf_jackknife(sample1, randoms, rbins, Nsub=[5, 5, 5], sample2=None, period=None, do_auto: bool = True,
                   do_cross: bool = True, estimator: str = "Natural", num_threads: int = 1, seed=None, mu_bins=None,
                   los: int = 2, return_counts: bool = False):
    """xi and its covariance matrix from leave-one-subvolume-out resampling, with halotools' ``tpcf_jackknife``
    arguments; ``mu_bins`` / ``los`` give xi(s, mu) instead of xi(r).  Every pair count with all its leave-one-out
    variants comes from ONE pass over the pairs (``device.tpcf_jackknife_counts``).

    * **Regions**: ``Nsub`` (an int or three) boxes per axis over one volume shared by ``sample1``, ``sample2`` and
      ``randoms``: ``[0, period]``, or with ``period=None`` their joint bounding box; the region of an object is
      ``jackknife_tags``'.  ``randoms`` are required.
    * **Weights** (halotools' rule, recalled from its source, not checked against the library): with region k left out
      a pair weighs 1 when neither end lies in k, 1/2 when exactly one does, 0 when both do.
    * **Endpoint identity** (checked against a brute-force weighted count in the tests): with ``ends[k, b]`` the number
      of pair ends in region k over the pairs of bin b, the weighted ordered auto pairs are ``2 counts - ends[k]`` and
      twice the weighted cross pairs likewise, exact integers; ``ends.sum(0) == 2 counts``.
    * **Estimate** (``jackknife_from_counts``): sample sizes ``N - (objects tagged k)``, each xi_k by the estimator of
      the module docstring, the returned xi the full-sample one, ``cov = (n - 1) / n sum_k (xi_k - mean)(xi_k -
      mean)^T`` over all regions, empty ones included.  Which counts enter the cross term (``D1R`` only) and the
      return order - ``(xi, cov)``; ``(xi_11, xi_12, xi_22, cov_11, cov_12, cov_22)``; ``(xi_12, cov_12)`` with
      ``do_cross`` only; ``(xi_11, xi_22, cov_11, cov_22)`` with ``do_auto`` only - are recalled, not checked.
    * ``return_counts`` appends a dict term -> ``(counts, ends)`` of the raw int64 arrays that were needed, under
      ``D1D1, D1D2, D2D2, D1R, D2R, RR``.  ``num_threads`` and ``seed`` are accepted and ignored."""
    from ... import device as dev

    _check_estimator(estimator)
    if not (do_auto or do_cross):
        raise ValueError("do_auto and do_cross are both False: nothing to compute")
    if randoms is None:
        raise ValueError("tpcf_jackknife needs randoms")
    s, mu = dev.check_tpcf_edges(rbins, mu_bins, period, periodic=period is not None)
    return _jackknife(sample1, randoms, s, mu, Nsub, sample2, period, do_auto, do_cross, estimator, los, return_counts)


def _jackknife(sample1, randoms, s, mu, Nsub, sample2, period, do_auto, do_cross, estimator, los, return_counts,
               rppi=False, transform=None):
    """``tpcf_jackknife`` after its argument checks: the regions, one counting pass per term and
    ``jackknife_from_counts`` (with its ``transform``).  ``s`` / ``mu``: checked edges; ``rppi``: r_p / pi edges and
    ``device.rp_pi_jackknife_counts``."""
    from ... import device as dev

    host = lambda a: dev.to_numpy(a) if hasattr(a, "is_cuda") else np.asarray(a)
    sets = {"1": host(sample1), "R": host(randoms)}
    if sample2 is not None:
        sets["2"] = host(sample2)
    nbins = (len(s) - 1) * (1 if mu is None else len(mu) - 1)
    for p in sets.values():
        nsub3, ntot, lo, hi = dev.check_jackknife_args(Nsub, np.shape(p), boxsize=period, nbins=nbins)
    if lo is None:
        filled = [p.astype(np.float64) for p in sets.values() if len(p)]
        lo = np.min([p.min(axis=0) for p in filled], axis=0) if filled else np.zeros(3)
        hi = np.max([p.max(axis=0) for p in filled], axis=0) if filled else np.zeros(3)
    tags = {k: jackknife_tags(p, nsub3, lo, hi) for k, p in sets.items()}
    m = {k: np.bincount(t, minlength=ntot) for k, t in tags.items()}

    def count(a, b=None):
        counter = dev.rp_pi_jackknife_counts if rppi else dev.tpcf_jackknife_counts
        out = counter(sets[a], ntot, s, mu, pos2=None if b is None else sets[b], boxsize=period, los=los,
                      tags1=tags[a], tags2=None if b is None else tags[b])
        return tuple(dev.to_numpy(x) for x in out)

    two = sample2 is not None
    auto1, auto2, cross = do_auto or not two, do_auto and two, do_cross and two
    c = {}
    if auto1:
        c["D1D1"] = count("1")
    if cross:
        c["D1D2"] = count("1", "2")
    if auto2:
        c["D2D2"] = count("2")
    if estimator in _USES_DR:
        c["D1R"] = count("1", "R")
        if auto2:
            c["D2R"] = count("2", "R")
    if estimator in _USES_RR:
        c["RR"] = count("R")
    out = jackknife_from_counts(c, len(sets["1"]), m["1"], len(sets["R"]), m["R"], len(sets["2"]) if two else None,
                                m.get("2"), estimator, do_auto, do_cross, transform=transform)
    return out + (c,) if return_counts else out


def wp_from_xi(xi, pi_bins):
    """``w_p(r_p) = 2 sum_l xi(r_p, pi_l) dpi_l`` over the pi bins (the last axis of ``xi``), halotools' sum in ``wp``.
    Host numpy, fp64."""
    xi = np.asarray(xi, dtype=np.float64)
    pi = np.asarray(pi_bins, dtype=np.float64).reshape(-1)
    if xi.ndim < 1 or xi.shape[-1] != len(pi) - 1:
        raise ValueError(f"xi has {xi.shape[-1] if xi.ndim else 0} pi bins, pi_bins gives {len(pi) - 1}")
    return 2.0 * np.sum(xi * np.diff(pi), axis=-1)


def _wp_pi_bins(pi_max, pi_bins):
    """The pi edges of ``wp``: halotools' single bin ``[0, pi_max]``, or ``pi_bins``, which must end at ``pi_max``."""
    if pi_bins is None:
        return np.array([0.0, float(pi_max)])
    pi = np.asarray(pi_bins, dtype=np.float64).reshape(-1)
    if len(pi) < 2 or pi[-1] != float(pi_max):
        raise ValueError(f"pi_bins must end at pi_max = {pi_max}, got {pi.tolist()}")
    return pi


def rp_pi_tpcf(sample1, rp_bins, pi_bins, sample2=None, randoms=None, period=None, do_auto: bool = True,
               do_cross: bool = True, estimator: str = "Natural", los: int = 2, return_counts: bool = False,
               num_threads: int = 1):
    """xi(r_p, pi) with halotools' ``rp_pi_tpcf`` arguments (module docstring): each term of shape (len(rp_bins) - 1,
    len(pi_bins) - 1), returned as ``s_mu_tpcf`` returns its terms.  The samples are used as given, with axis ``los``
    the line of sight.  With ``return_counts`` also the dict of raw int64 counts.  ``num_threads`` is ignored."""
    from ... import device as dev

    _check_estimator(estimator)
    if not (do_auto or do_cross):
        raise ValueError("do_auto and do_cross are both False: nothing to compute")
    if period is None and randoms is None:
        raise ValueError("period=None (open boundaries) needs randoms")
    rp, pi = dev.check_rp_pi_edges(rp_bins, pi_bins, period, periodic=period is not None)
    xi, c = _correlate(sample1, sample2, randoms, rp, pi, period, estimator, do_auto, do_cross, los=los, rppi=True)
    return (xi, c) if return_counts else xi


def wp(sample1, rp_bins, pi_max, sample2=None, randoms=None, period=None, do_auto: bool = True, do_cross: bool = True,
       estimator: str = "Natural", los: int = 2, pi_bins=None, return_counts: bool = False, num_threads: int = 1):
    """The projected correlation function ``w_p(r_p) = 2 sum_l xi(r_p, pi_l) dpi_l`` with halotools' ``wp`` arguments:
    each term of shape (len(rp_bins) - 1,), returned as ``rp_pi_tpcf`` returns its terms.  ``pi_bins`` None:
    halotools' single bin ``[0, pi_max]``; given, they must end at ``pi_max``.  With ``return_counts`` also the dict
    of raw int64 (r_p, pi) counts.  ``num_threads`` is ignored."""
    pi = _wp_pi_bins(pi_max, pi_bins)
    xi, c = rp_pi_tpcf(sample1, rp_bins, pi, sample2=sample2, randoms=randoms, period=period, do_auto=do_auto,
                       do_cross=do_cross, estimator=estimator, los=los, return_counts=True)
    out = tuple(wp_from_xi(x, pi) for x in xi) if isinstance(xi, tuple) else wp_from_xi(xi, pi)
    return (out, c) if return_counts else out


def _rp_pi_jackknife(name, sample1, randoms, rp_bins, pi, Nsub, sample2, period, do_auto, do_cross, estimator, los,
                     return_counts, transform=None):
    from ... import device as dev

    _check_estimator(estimator)
    if not (do_auto or do_cross):
        raise ValueError("do_auto and do_cross are both False: nothing to compute")
    if randoms is None:
        raise ValueError(f"{name} needs randoms")
    rp, pi = dev.check_rp_pi_edges(rp_bins, pi, period, periodic=period is not None)
    return _jackknife(sample1, randoms, rp, pi, Nsub, sample2, period, do_auto, do_cross, estimator, los, return_counts,
                      rppi=True, transform=transform)


def rp_pi_tpcf_jackknife(sample1, randoms, rp_bins, pi_bins, Nsub=[5, 5, 5], sample2=None, period=None,
                         do_auto: bool = True, do_cross: bool = True, estimator: str = "Natural", los: int = 2,
                         return_counts: bool = False, num_threads: int = 1, seed=None):
    """xi(r_p, pi) and its covariance matrix from leave-one-subvolume-out resampling, with halotools'
    ``rp_pi_tpcf_jackknife`` arguments: ``tpcf_jackknife`` (regions, weights, estimate, return order, ``return_counts``)
    on the (r_p, pi) counts of ``device.rp_pi_jackknife_counts``; xi of shape (n_rp, n_pi), cov (n_rp n_pi, n_rp n_pi).
    ``num_threads`` and ``seed`` are accepted and ignored."""
    return _rp_pi_jackknife("rp_pi_tpcf_jackknife", sample1, randoms, rp_bins, pi_bins, Nsub, sample2, period, do_auto,
                            do_cross, estimator, los, return_counts)


def wp_jackknife(sample1, randoms, rp_bins, pi_max, Nsub=[5, 5, 5], sample2=None, period=None, do_auto: bool = True,
                 do_cross: bool = True, estimator: str = "Natural", los: int = 2, pi_bins=None,
                 return_counts: bool = False, num_threads: int = 1, seed=None):
    """w_p(r_p) of the full sample and its jackknife covariance, with halotools' ``wp_jackknife`` arguments, in
    ``tpcf_jackknife``'s return order with terms of shape (n_rp,) and cov (n_rp, n_rp).  The covariance is that of the
    per-region ``w_p,k = wp_from_xi(xi_k)``, formed from the xi_k of the one counting pass of
    ``rp_pi_tpcf_jackknife`` (no second pass over the pairs).  ``pi_bins`` as ``wp``; ``return_counts`` appends the
    dict of raw (r_p, pi) ``(counts, ends)``.  ``num_threads`` and ``seed`` are accepted and ignored."""
    pi = _wp_pi_bins(pi_max, pi_bins)
    return _rp_pi_jackknife("wp_jackknife", sample1, randoms, rp_bins, pi, Nsub, sample2, period, do_auto, do_cross,
                            estimator, los, return_counts, transform=lambda xi: wp_from_xi(xi, pi))


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
