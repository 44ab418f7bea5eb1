"""Spherical profiles of particles around haloes and voids: the reference's ``astrild.profiles.profile_3d``.

The reference's ``Profiles3D.get_one_profile`` takes the particles of one halo, ``coordinates[cum_N : cum_N + N]``,
divides their distances to the halo centre by r200c and histograms them with ``np.histogram`` in 20 logarithmic bins
from 0.05 to 1; a catalogue is a Python loop over haloes.  Here all centres go through one launch
(``device.sphere_profiles``, ``ast_profile3d_*``): per centre one histogram with edges in units of that centre's own
radius, counts plus the sums of w, w v_r, w v_r^2 and w |u|^2.  ``radial_profiles`` finds the particles in reach itself
(a cell grid, periodic or open); ``Profiles3D`` bins the reference's membership segments.

Bins follow ``np.histogram``: e_k <= x < e_{k+1}, the last bin closed, with x = sqrt((sx^2 + sy^2) + sz^2) / R in
float64, which is bit-equal to the reference's ``np.linalg.norm(d, axis=1) / R`` for float64 input.  A particle at
distance 0 counts when the first edge is 0 (the pair counts of ``tpcf`` never count distance 0).

Deliberate differences from the reference:

* ``get_one_profile`` there calls ``prof.from_particle_data`` with an undefined ``prof`` and fails with NameError;
  here it returns the profile.  It honours ``nbins`` (the reference's ``from_particle_data`` overwrites it with 20;
  the static ``from_particle_data`` here still does, literally).
* Its "velo" branch recomputes the positions as "velocities" and passes a particle mass of 0, so every bin would be 0.
  Here a quantity with "velo" in its name needs ``velocities`` and returns a velocity profile relative to ``halo_vel``:
  "... radial ... dispersion" sigma_r, "... radial ..." the mean v_r, otherwise the 3D dispersion sqrt(<|u|^2>).
* The class has a constructor (the reference's has none and its attributes are never set), ``get_profiles`` for the
  whole catalogue, and an optional ``boxsize`` for haloes that straddle a face of a periodic box.
"""
import numpy as np

__all__ = ["radial_profiles", "Profiles3D", "log_bins", "bin_volumes"]


def log_bins(nbins=20, min_rad=0.05, max_rad=1.0):
    """The reference's radial bins (profile_3d.py:64-67)."""
    return np.logspace(np.log10(min_rad), np.log10(max_rad), nbins + 1, base=10.0)


def bin_volumes(edges):
    """Shell volumes in units of radius^3 (profile_3d.py:71)."""
    edges = np.asarray(edges, dtype=np.float64)
    return 4.0 / 3.0 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3)


def _finish(edges, counts, moments):
    """The profile dict from the device sums; empty bins give 0 density and nan means (numpy's 0 / 0, silently)."""
    out = {"radii": 0.5 * (edges[1:] + edges[:-1]), "counts": counts, "mass": moments[..., 0],
           "density": moments[..., 0] / bin_volumes(edges)}
    if moments.shape[-1] == 4:
        with np.errstate(invalid="ignore", divide="ignore"):
            w = moments[..., 0]
            vr, vr2, u2 = moments[..., 1] / w, moments[..., 2] / w, moments[..., 3] / w
            out["v_r"] = vr
            out["sigma_r"] = np.sqrt(np.maximum(vr2 - vr * vr, 0.0))
            out["sigma_3d"] = np.sqrt(u2)
    return out


def radial_profiles(pos, centres, radii, edges, boxsize=None, weights=None, vel=None, centre_vel=None,
                    return_counts=False):
    """Profiles of all particles ``pos`` (Np, 3) around ``centres`` (Nc, 3), in bins ``edges`` in units of each centre's
    ``radii``; ``boxsize`` given: a periodic cube.  A dict of (Nc, nbins) numpy arrays:

    * ``radii``: the arithmetic midpoints of ``edges`` (nbins,), as the reference;
    * ``counts`` (int64), ``mass``: the sum of ``weights`` (1 each when None);
    * ``density``: mass / (4 pi / 3 (e_{k+1}^3 - e_k^3)), in units of radius^-3 (the reference's ``bin_value``);
    * with ``vel``: ``v_r`` the weighted mean radial velocity relative to ``centre_vel`` (0 when None), ``sigma_r`` =
      sqrt(<v_r^2> - <v_r>^2) and ``sigma_3d`` = sqrt(<|u|^2>); nan in empty bins.

    ``return_counts=True`` returns ``(dict, counts, moments)`` with the raw device sums as numpy arrays.
    Arguments are checked as ``device.sphere_profiles`` documents (ValueError)."""
    return _profiles(pos, centres, radii, edges, boxsize, weights, vel, centre_vel, return_counts, None)


def _profiles(pos, centres, radii, edges, boxsize, weights, vel, centre_vel, return_counts, segments):
    """``radial_profiles``; ``segments`` (Nc, 2) integer (offset, count): centre i looks only at that slice of ``pos``
    (``Profiles3D``'s membership mode)."""
    from .. import device as dev
    counts, moments = dev.sphere_profiles(pos, centres, radii, edges, boxsize=boxsize, weights=weights, vel=vel,
                                          centre_vel=centre_vel, segments=segments)
    counts, moments = dev.to_numpy(counts), dev.to_numpy(moments)
    out = _finish(np.asarray(edges, dtype=np.float64).reshape(-1), counts, moments)
    return (out, counts, moments) if return_counts else out


class Profiles3D:
    """Profiles of haloes from their member particles (the reference's ``Profiles3D``): halo i owns
    ``coordinates[cum_N_particles[i] : cum_N_particles[i] + N_particles[i]]`` and is binned in units of ``r200c[i]``."""

    def __init__(self, coordinates, halo_pos, r200c, N_particles, cum_N_particles=None, Mpart=1.0, velocities=None,
                 halo_vel=None, boxsize=None):
        self.coordinates = coordinates
        self.velocities = velocities
        self.halo_pos = np.asarray(halo_pos, dtype=np.float64).reshape(-1, 3)
        self.halo_vel = None if halo_vel is None else np.asarray(halo_vel, dtype=np.float64).reshape(-1, 3)
        self.r200c = np.asarray(r200c, dtype=np.float64).reshape(-1)
        self.N_particles = np.asarray(N_particles, dtype=np.int64).reshape(-1)
        if cum_N_particles is None:
            cum_N_particles = np.concatenate([[0], np.cumsum(self.N_particles)[:-1]])
        self.cum_N_particles = np.asarray(cum_N_particles, dtype=np.int64).reshape(-1)
        self.Mpart = Mpart
        self.boxsize = boxsize

    def _values(self, idx, quantity, bins):
        velo = "velo" in quantity
        if velo and self.velocities is None:
            raise ValueError(f"quantity {quantity!r} needs velocities")
        seg = np.stack([self.cum_N_particles[idx], self.N_particles[idx]], axis=1)
        prof = _profiles(self.coordinates, self.halo_pos[idx], self.r200c[idx], bins, self.boxsize, None,
                         self.velocities if velo else None,
                         self.halo_vel[idx] if velo and self.halo_vel is not None else None, False, seg)
        if velo:
            if "radial" in quantity:
                return prof["radii"], prof["sigma_r"] if "dispersion" in quantity else prof["v_r"]
            return prof["radii"], prof["sigma_3d"]
        if quantity == "count":
            return prof["radii"], prof["counts"]
        return prof["radii"], prof["counts"] * self.Mpart / bin_volumes(bins)     # profile_3d.py:74-76

    def get_one_profile(self, halo_idx, quantity="mass", nbins=20):
        """(bin_radii, bin_values) of halo ``halo_idx`` in ``nbins`` logarithmic bins from 0.05 to 1 r200c."""
        radii, values = self._values(np.array([int(halo_idx)]), quantity, log_bins(nbins))
        return radii, values[0]

    def get_profiles(self, quantity="mass", nbins=20, min_rad=0.05, max_rad=1.0):
        """(bin_radii (nbins,), values (Nhaloes, nbins)) of every halo, in one launch."""
        return self._values(np.arange(len(self.r200c)), quantity, log_bins(nbins, min_rad, max_rad))

    @staticmethod
    def from_particle_data(pos, vel, Mpart, quantity, nbins):
        """The reference's function, literally (profile_3d.py:55-78): ``pos`` are the particles' distances in units of
        r200c; ``vel``, ``quantity`` and ``nbins`` are ignored (20 bins from 0.05 to 1).  Host numpy, as there."""
        bins = log_bins(20)
        bin_radii = 0.5 * (bins[1:] + bins[:-1])
        number_particles = np.histogram(pos, bins=bins)[0]
        return bin_radii, number_particles * Mpart / bin_volumes(bins)
