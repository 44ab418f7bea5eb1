"""``SubFind.power_spectrum`` with astrild's API
(src/astrild/particles/hutils/stats_subfind.py:109-153): particles -> TSC paint
-> /dx^3 -> FFTPower, on the GPU."""
import numpy as np
import torch

from ... import device as dev


class SubFind:
    dtype = torch.float64

    @staticmethod
    def power_spectrum(snapshot, objects: str = "subhalo", limits: tuple = None, nbins: int = 512,
                       boxsize: float = 500.0):
        """Real-space halo power spectrum.  ``snapshot`` exposes ``.cat[...]`` and
        ``.header.hubble/.boxsize`` like astrild's read_hdf5.snapshot."""
        if boxsize is None:
            boxsize = snapshot.header.boxsize / 1e3  # [Mpc/h]
        if objects != "subhalo":
            raise ValueError(f"objects={objects!r} is not supported")
        # The reference converts units on the host first (pos * h / 1e3 [Mpc/h], mass * h / 1e10: stats_subfind.py:121-122 -
        # two numpy passes over the catalogue, 7.5 ms for 2e6 objects, more than everything the GPU does with it).  Here the
        # catalogue goes to the device as it was read; the position factor rides on the cell lookup (pos_scale), the mass
        # factor on the paint's scale.
        h = float(snapshot.header.hubble)
        dx = boxsize / nbins
        pos = dev.as_device(np.ascontiguousarray(snapshot.cat["SubhaloPos"][:]), SubFind.dtype)
        mass = dev.as_device(np.ascontiguousarray(snapshot.cat["SubhaloMass"][:]), SubFind.dtype)
        # pm.paint(pos, mass=mass, resampler="tsc") / dx**3   (stats_subfind.py:130-132)
        # ... then FFTPower(ArrayMesh(value_map), mode="1d")                 (stats_subfind.py:134-150)
        r = dev.paint_power_1d(pos, mass, nbins, boxsize, "tsc", scale=(h / 1e10) / dx ** 3, pos_scale=h / 1e3)
        k = np.array(r["k"])
        Pk = np.array(r["power"] - r["shotnoise"])
        return k, Pk

    @staticmethod
    def mean_pairwise_velocity(snapshot, limits: tuple = None, nbins: int = None, boxsize: float = None,
                               seperate: dict = None) -> tuple:
        """Mean radial pairwise velocity v12(r) of two groups of haloes in the periodic box, the reference's
        commented-out method (stats_subfind.py:155-218), with ``pair_velocity_box.mean_radial_velocity_vs_r`` in
        halotools' place.  Defaults as there: ``boxsize = header.boxsize / 1e3`` [Mpc/h], ``limits = (0.3, boxsize / 5)``,
        ``nbins = int(2 / 3 * max(limits))``; positions ``GroupPos * header.hubble / 1e3`` [Mpc/h], velocities
        ``GroupVel`` [km/s].  ``seperate = {"Group_M_Crit200": 14, "compare": [1, 2]}`` splits the catalogue at
        10^14 of that field: compare code 1 takes the haloes below the threshold, 2 those above, first entry for group
        one, second for group two (any other code leaves ``<`` for group one and ``>`` for group two); None: all haloes
        in both groups.

        One deliberate difference: ``r = geomspace(min(limits), max(limits), nbins)`` are the bin EDGES and the return
        is ``(r_c, v12)`` with ``r_c`` the ``nbins - 1`` bin centres.  The reference passes the centres as bins and
        returns ``r_c[1:]``, whose length does not match its ``nbins - 2`` values."""
        from .pair_velocity_box import mean_radial_velocity_vs_r

        if boxsize is None:
            boxsize = snapshot.header.boxsize / 1e3  # [Mpc/h]
        if limits is None:
            limits = (0.3, boxsize / 5)
        if nbins is None:
            nbins = int(2 / 3 * max(limits))
        r = np.geomspace(min(limits), max(limits), nbins)
        r_c = 0.5 * (r[1:] + r[:-1])

        if seperate is None:
            idx1 = np.ones(len(snapshot.cat["GroupVel"][:]), dtype=bool)
            idx2 = np.ones(len(snapshot.cat["GroupVel"][:]), dtype=bool)
        else:
            split_quantity = list(seperate.keys())[0]
            below = snapshot.cat[split_quantity][:] < 10 ** seperate[split_quantity]
            above = snapshot.cat[split_quantity][:] > 10 ** seperate[split_quantity]
            idx1 = {1: below, 2: above}.get(seperate["compare"][0], below)
            idx2 = {1: below, 2: above}.get(seperate["compare"][1], above)

        pos1 = snapshot.cat["GroupPos"][idx1, :] * snapshot.header.hubble / 1e3  # [Mpc/h]
        vel1 = snapshot.cat["GroupVel"][idx1, :]  # [km/sec]
        pos2 = snapshot.cat["GroupPos"][idx2, :] * snapshot.header.hubble / 1e3  # [Mpc/h]
        vel2 = snapshot.cat["GroupVel"][idx2, :]  # [km/sec]
        pv12 = mean_radial_velocity_vs_r(pos1, vel1, rbins_absolute=r, sample2=pos2, velocities2=vel2, period=boxsize)
        return r_c, pv12
