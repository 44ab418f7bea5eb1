"""Mean pairwise velocity v12 and pairwise velocity dispersion sigma12 per separation bin, of one or two samples, in a
periodic box or with open boundaries; the pair sums on the GPU (``device.pair_velocity_moments``).  The argument names
are those of halotools' ``mean_radial_velocity_vs_r``, ``radial_pvd_vs_r``, ``mean_los_velocity_vs_rp`` and
``los_pvd_vs_rp``, which the reference's commented-out ``SubFind.mean_pairwise_velocity`` calls
(``stats_subfind.py:155-218``).  halotools is not used here, and parity with it is unpinned: this module restates its
published behaviour as far as we recall it, without a check against the library itself (as ``hutils/tpcf.py``).

The rules, all in fp64 and op by op:

* **Separation**: ``s_a = x_j[a] - x_i[a]`` per axis.  With a ``period`` L, ``s_a > L / 2 -> s_a - L``, else
  ``s_a < -L / 2 -> s_a + L``.  The rule is exactly antisymmetric under i <-> j, and ``|s_a|`` is bit for bit the
  two-point correlation function's ``min(|dx|, L - |dx|)``.  ``period=None``: open boundaries, plain separations.
* **Velocity difference**: ``dv = v_j - v_i``.
* **radial** (``mean_radial_velocity_vs_r``, ``radial_pvd_vs_r``): ``d^2 = (s_x^2 + s_y^2) + s_z^2``; the pair is in
  bin k when ``r_k^2 < d^2 <= r_{k+1}^2`` (the bins of ``tpcf_r``, so the pair counts are its counts; a pair at
  d = 0 is in no bin and no NaN arises); ``v = ((dv_x s_x + dv_y s_y) + dv_z s_z) / sqrt(d^2)``, negative for infall.
* **los** (``mean_los_velocity_vs_rp``, ``los_pvd_vs_rp``; the periodic twin of the reference's ``mean_pv_z_sign``):
  with a, b the two axes other than ``los`` in axis order, ``rp^2 = s_a^2 + s_b^2``; the pair is in bin k when
  ``rp_k^2 < rp^2 <= rp_{k+1}^2`` and ``|s_los| <= pi_max``; ``v = dv_los * sign(s_los)``, sign in {-1, 0, +1}.
* Both v are unchanged bit for bit under i <-> j, so the auto term needs no orientation.
* **Pairs**: without ``sample2`` the unordered pairs i < j of sample 1 (the auto term); with it every pair (i of
  sample 1, j of sample 2) (the 1 x 2 cross term).
* **Result**: ``mean = sum v / count`` and ``sigma = sqrt(max(sum v^2 / count - mean^2, 0))`` on the host in fp64;
  NaN in a bin without pairs.
* **Validation** (``ValueError`` before any pair work): bins finite, >= 0 and strictly increasing; with a ``period``
  the top bin edge, and ``pi_max``, below period / 3 and every coordinate in [0, period]; without one every coordinate
  finite; ``pi_max`` positive and finite; ``los`` 0, 1 or 2; samples (N, 3) with velocities shaped like them; a
  second sample comes with its velocities.

halotools' ``rbins_normalized`` / ``normalize_rbins_by`` (per-object normalised bins), weights, ``num_threads`` and
``approx_cell*_size`` are not taken.  ``return_moments=True`` also returns the dict of raw sums
``{count, sum_v, sum_v2}`` (int64, float64, float64)."""
import numpy as np


def _moments(sample1, velocities1, bins, sample2, velocities2, period, kind, pi_max=None, los=2):
    from ... import device as dev
    count, s1, s2 = dev.pair_velocity_moments(sample1, velocities1, bins, pos2=sample2, vel2=velocities2,
                                              boxsize=period, kind=kind, pi_max=pi_max, los=los)
    count, s1, s2 = (np.array(dev.to_numpy(x)) for x in (count, s1, s2))
    mean, sigma = dev.finish_pair_velocity(count, s1, s2)
    return mean, sigma, dict(count=count, sum_v=s1, sum_v2=s2)


def mean_radial_velocity_vs_r(sample1, velocities1, rbins_absolute, sample2=None, velocities2=None, period=None,
                              return_moments=False):
    """v12(r): the mean radial pairwise velocity per bin of ``rbins_absolute``, shape (len(rbins_absolute) - 1,)
    (module docstring)."""
    mean, _, mom = _moments(sample1, velocities1, rbins_absolute, sample2, velocities2, period, "radial")
    return (mean, mom) if return_moments else mean


def radial_pvd_vs_r(sample1, velocities1, rbins_absolute, sample2=None, velocities2=None, period=None,
                    return_moments=False):
    """sigma12(r): the dispersion of the radial pairwise velocity per bin of ``rbins_absolute`` (module docstring)."""
    _, sigma, mom = _moments(sample1, velocities1, rbins_absolute, sample2, velocities2, period, "radial")
    return (sigma, mom) if return_moments else sigma


def mean_los_velocity_vs_rp(sample1, velocities1, rp_bins, pi_max, sample2=None, velocities2=None, period=None, los=2,
                            return_moments=False):
    """The mean line-of-sight pairwise velocity per bin of projected separation ``rp_bins``, over the pairs within
    ``pi_max`` along axis ``los``, shape (len(rp_bins) - 1,) (module docstring)."""
    mean, _, mom = _moments(sample1, velocities1, rp_bins, sample2, velocities2, period, "los", pi_max, los)
    return (mean, mom) if return_moments else mean


def los_pvd_vs_rp(sample1, velocities1, rp_bins, pi_max, sample2=None, velocities2=None, period=None, los=2,
                  return_moments=False):
    """The dispersion of the line-of-sight pairwise velocity per bin of ``rp_bins`` (module docstring)."""
    _, sigma, mom = _moments(sample1, velocities1, rp_bins, sample2, velocities2, period, "los", pi_max, los)
    return (sigma, mom) if return_moments else sigma
