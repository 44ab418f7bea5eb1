"""``PowerSpectrum3D`` with astrild's API (src/astrild/power_spectra/power_spectrum_3d.py),
computed on the MI355X: NGP scatter-assign, rocFFT 3D R2C and FFTPower shell
binning all run through libastrild_hip.so.

Differences from the reference, all deliberate:
* ``PowerSpectrumWarning`` is undefined where the reference raises it
  (power_spectrum_3d.py:49,100,127); the intended ``PowerSpectrum3DWarning`` is used.
* nbodykit's ``ArrayMesh`` ignores ``compensated/interlaced/window`` for an
  in-memory array, so the cross-spectrum branch (:197-222) is the plain cross
  power of the two grids, exactly what the reference executes.
"""
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import pandas as pd
import torch

from .. import device as dev
from ..io import IO


class PowerSpectrum3DWarning(BaseException):
    pass


class PowerSpectrum3D:
    """
    Attributes:
        sim_type:
        simulation: object exposing .boxsize, .domain_level, .npar, .dirs, .dir_nrs,
            .get_file_nrs(), .get_file_paths() (astrild.simulation.Simulation)

    Methods:
        compute:
    """

    #: grid / FFT precision on the device: float64 like the reference; set to
    #: torch.float32 for the fp32 fast path of BASELINE.json configs[1]
    dtype = torch.float64

    def __init__(self, sim_type: str, simulation):
        self.sim = simulation
        self.sim.type = sim_type

    def compute(
        self,
        quantities: List[str],
        file_dsc: List[Dict[str, str]],
        snap_nrs: Optional[List[int]] = None,
        dir_out: Optional[str] = None,
        save: bool = True,
        mode: str = "1d",
        Nmu: int = 5,
        los: int = 2,
        poles: Tuple[int, ...] = (0, 2, 4),
    ) -> Union[None, dict]:
        """Power spectrum of particle quantities, same call as power_spectrum_3d.py:33-81: one file
        description -> auto spectra, two -> cross spectra of the paired files; one spectrum per snapshot.
        Returns {"k": {snap_%d: k}, "P": {snap_%d: P}} when ``save`` is False, else writes pk_<quantities>.h5.

        ``mode="2d"`` (no reference counterpart; nbodykit's ``FFTPower(mode="2d", Nmu=, los=, poles=)``): P(k, mu) in
        ``Nmu`` bins of mu about the box axis ``los`` and the multipoles ``poles``.  Returns {snap_%d: the dict of
        :meth:`_power_spectrum_2d`} when ``save`` is False, else writes pkmu_<quantities>.h5."""
        if mode not in ("1d", "2d"):
            raise ValueError(f"mode must be '1d' or '2d', got {mode!r}")
        if mode == "2d":
            Nmu, los, poles = dev.check_fftpower_2d_args(Nmu, los, poles)
        jobs = self._jobs(file_dsc, snap_nrs)
        if mode == "2d":
            pkmu = self._spectra(quantities, jobs, cross=len(file_dsc) > 1,
                                 spectrum=lambda *maps: self._power_spectrum_2d(*maps, Nmu=Nmu, los=los, poles=poles))
            if save:
                self._save_results_2d(quantities, pkmu)
                return None
            return pkmu
        pk = self._spectra(quantities, jobs, cross=len(file_dsc) > 1)
        if save:
            self._save_results(quantities, pk)
            return None
        return pk

    def _jobs(self, file_dsc, snap_nrs):
        """[(snap_nr, (path,) or (path1, path2))] sorted by snapshot: the reference's file resolution
        (:48-71; an explicit snapshot list must be a subset of the simulation's directories, without one
        the file numbers of the first description are used and "path" is popped from the descriptions)."""
        explicit = bool(snap_nrs)
        if explicit and not set(snap_nrs) < set(self.sim.dir_nrs):
            raise PowerSpectrum3DWarning(
                f"Some of the snapshots {snap_nrs} do not exist in:\n{self.sim.dir_nrs}")
        columns = []
        for i, dsc in enumerate(file_dsc[:2]):
            path = dsc["path"] if explicit else dsc.pop("path")
            if i == 0 and not explicit:
                snap_nrs = self.sim.get_file_nrs(dsc, path, "max")
            columns.append(self.sim.get_file_paths(dsc, path, "max"))
        return list(zip(np.sort(snap_nrs), zip(*columns)))

    def _spectra(self, quantity, jobs, cross, spectrum=None) -> dict:
        """One spectrum per job.  Auto: the ``quantity`` column of the file; cross: both files as they are
        (the reference passes quantity=None there, :120-121).  ``spectrum`` (maps -> result): what is computed of a
        snapshot's grids instead of (k, P); the results come back as {snap_%d: result}."""
        pk = {"k": {}, "P": {}} if spectrum is None else {}
        # The reference reads, grids and transforms snapshot after snapshot (power_spectrum_3d.py:83-110).  Here the NEXT
        # snapshot's files are read (and .npy grids staged in page-locked memory) by a loader thread while the current one
        # is uploaded and transformed: a 512^3 float64 grid is 19 ms of PCIe next to ~6 ms of GPU work, and the disk read
        # is longer than both.
        from concurrent.futures import ThreadPoolExecutor
        q = None if cross else quantity
        self._files_per_job = max((len(paths) for _, paths in jobs), default=1)

        def load(tickets):
            return [self._fill_host(t) for t in tickets]

        def submit(pool, paths):
            # the page-locked staging buffers are taken HERE, on the calling thread: the loader thread only reads files and
            # copies bytes - it never enters the GPU runtime (a pinned allocation from a second thread beside the first GPU
            # calls of the process is the one thing this loop did there; the suite once aborted at exactly that point)
            return pool.submit(load, [self._open_host(p, q) for p in paths])
        with ThreadPoolExecutor(max_workers=1) as pool:
            fut = submit(pool, jobs[0][1]) if jobs else None
            for i, (snap_nr, paths) in enumerate(jobs):
                loaded = fut.result()
                fut = submit(pool, jobs[i + 1][1]) if i + 1 < len(jobs) else None
                maps = [self._to_device(item) for item in loaded]
                if maps[0].dim() != 3:
                    raise PowerSpectrum3DWarning(f"{maps[0].dim()}D is not supported :-(")
                if spectrum is not None:
                    pk["snap_%d" % snap_nr] = spectrum(*maps)
                    continue
                pk["k"]["snap_%d" % snap_nr], pk["P"]["snap_%d" % snap_nr] = self._power_spectrum_3d(*maps)
        if spectrum is not None:
            return pk
        ks = list(pk["k"].values())
        if len(ks) > 1:                     # the reference's check that snapshots share their wavenumbers
            assert np.sum(ks[0]) == np.sum(ks[1])
        return pk

    # the reference's two entry points, kept for callers that use them directly
    def _auto_power_spectra(self, quantity, snap_nrs, _file_paths) -> dict:
        return self._spectra(quantity, list(zip(snap_nrs, ((p,) for p in _file_paths))), cross=False)

    def _cross_power_spectra(self, quantity, snap_nrs, _file_paths1, _file_paths2) -> dict:
        return self._spectra(quantity, list(zip(snap_nrs, zip(_file_paths1, _file_paths2))), cross=True)

    def _read_data(self, file_in: str, quantity=None):
        """NGP scatter-assign of a DataFrame column, or a pre-gridded .npy
        (power_spectrum_3d.py:140-153).  Returns a CUDA tensor (npar, npar, npar)."""
        return self._to_device(self._load_host(file_in, quantity))

    def _load_host(self, file_in: str, quantity=None):
        """The disk -> host half of _read_data: the DataFrame columns of an .h5 file, or a .npy grid copied into a page-locked
        buffer (two rotate) so that its upload can run asynchronously."""
        return self._fill_host(self._open_host(file_in, quantity))

    def _open_host(self, file_in: str, quantity=None):
        """What the CALLING thread does of _load_host: the .npy header (a memory map) and the page-locked staging buffer the
        grid will be read into - everything that enters the GPU runtime."""
        if ".h5" in file_in:
            return ("frame", file_in, quantity)
        elif ".npy" in file_in:
            arr = np.load(file_in, mmap_mode="r")
            pinned = self._pinned(arr.shape, arr.dtype) if torch.cuda.is_available() else None
            return ("array", arr, pinned)
        elif file_in.endswith((".a_den", ".a_vel", ".a_velDiv", ".den", ".dtfe")):
            return ("density_file", file_in)
        return ("zeros", None)

    @staticmethod
    def _fill_host(ticket):
        """What the loader thread does: file reads and host copies only (no GPU call of any kind)."""
        if ticket[0] == "frame":
            _, file_in, quantity = ticket
            fields = pd.read_hdf(file_in, key="df")
            column = quantity[0] if isinstance(quantity, (list, tuple)) else quantity
            return ("frame", tuple(np.ascontiguousarray(fields[c].values) for c in ("x", "y", "z", column)))
        if ticket[0] == "array":
            _, arr, pinned = ticket
            if pinned is None:
                return ("array", torch.from_numpy(np.ascontiguousarray(arr)))
            pinned.numpy()[...] = arr                    # the disk read itself, straight into page-locked memory
            return ("array", pinned)
        return ticket

    def _pinned(self, shape, dtype):
        """One of the rotating page-locked staging buffers of this shape: two per file of a job (the loader fills the next
        job's while the current job's upload)."""
        key = (tuple(shape), np.dtype(dtype).str)
        pool = self.__dict__.setdefault("_pinned_pool", {})
        bufs, turn = pool.get(key, ([], 0))
        tdt = torch.from_numpy(np.empty(0, dtype=dtype)).dtype
        slots = 2 * self.__dict__.get("_files_per_job", 1)      # the job being uploaded + the job being read
        if len(bufs) < slots:
            bufs.append(torch.empty(tuple(shape), dtype=tdt, pin_memory=True))
            pool[key] = (bufs, len(bufs) % slots)
            return bufs[-1]
        pool[key] = (bufs, (turn + 1) % slots)
        return bufs[turn]

    def _to_device(self, loaded):
        """The host -> HBM half of _read_data."""
        kind, payload = loaded
        if kind == "frame":
            x, y, z, values = payload
            return dev.ngp_assign(x, y, z, values, self.sim.npar, dtype=self.dtype)
        if kind == "array":
            if payload.is_pinned():
                # asynchronous upload on a copy stream; the compute stream waits for it, and the staging buffer is not
                # refilled before then (the loader is one snapshot ahead, the buffers rotate in pairs)
                copy = self.__dict__.setdefault("_copy_stream", torch.cuda.Stream())
                copy.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(copy):
                    t = payload.to(dev.device(), non_blocking=True)
                    if t.dtype != self.dtype:
                        t = t.to(self.dtype)
                torch.cuda.current_stream().wait_stream(copy)
                t.record_stream(torch.cuda.current_stream())
                return t.contiguous()
            return dev.as_device(payload, self.dtype)
        if kind == "density_file":
            # a DTFE grid binary (what dtfe.py:70-80 / powmes.py:21-23 turn into the .npy above): straight to the device
            from ..formats import read_density_grid
            return read_density_grid(payload, dtype=self.dtype)[1]
        return dev.as_device(np.zeros((self.sim.npar,) * 3), self.dtype)

    def _get_vector_magnitude(self, value_map: np.ndarray) -> np.ndarray:
        """Vector magnitude of a (N, N, N, 3) array (power_spectrum_3d.py:155-162)."""
        value_map = np.sqrt(np.sum(np.square(value_map), axis=3))
        assert len(value_map.shape) == 3
        return value_map

    def _power_spectrum_3d(self, value_map1, value_map2=None) -> Tuple[np.ndarray, np.ndarray]:
        """3D auto / cross power spectrum, FFTPower(mode="1d", kmin=2*pi/L) semantics
        (power_spectrum_3d.py:164-226).  Accepts numpy arrays or CUDA tensors."""
        f1 = dev.as_device(value_map1, self.dtype)
        f2 = None if value_map2 is None else dev.as_device(value_map2, self.dtype)
        n = int(self.sim.domain_level)
        if tuple(f1.shape) != (n, n, n):
            raise PowerSpectrum3DWarning(f"value_map shape {tuple(f1.shape)} does not match Nmesh={n}")
        r = dev.fftpower_1d(f1, self.sim.boxsize, f2)
        k = np.array(r["k"])
        Pk = np.array(r["power"] - r["shotnoise"])
        print("Pk wavenumber ------>", np.nanmin(k), np.nanmax(k))
        return k, Pk

    def _power_spectrum_3d_catalog(self, pos1, mass1=None, pos2=None, mass2=None, window: str = "tsc",
                                   interlaced: bool = True, compensated: bool = True) -> Tuple[np.ndarray, np.ndarray]:
        """The cross (or auto) spectrum of PARTICLE catalogues with the mesh parameters the reference writes in its
        cross branch (power_spectrum_3d.py:197-212: ``compensated=True, interlaced=True, window='TSC'``).  There they
        decorate an ``ArrayMesh`` and do nothing; for a catalogue source they mean: paint with the window, paint again
        half a cell shifted, combine the two spectra and divide by the window.  Positions in box
        units, ``(Np, 3)``; returns ``(k, P - shotnoise)`` like ``_power_spectrum_3d``."""
        as_dev = lambda a: None if a is None else dev.as_device(np.ascontiguousarray(a), self.dtype)
        r = dev.catalog_power_1d(as_dev(pos1), as_dev(mass1), int(self.sim.domain_level), self.sim.boxsize, window,
                                 interlaced, compensated, pos2=as_dev(pos2), mass2=as_dev(mass2))
        return np.array(r["k"]), np.array(r["power"] - r["shotnoise"])

    def _power_spectrum_2d(self, value_map1, value_map2=None, Nmu: int = 5, los: int = 2, poles=(0, 2, 4)) -> dict:
        """P(k, mu) and multipoles of one grid (or the cross spectrum of two), ``FFTPower(mode="2d", Nmu=, los=, poles=,
        kmin=2*pi/L)`` semantics with the line of sight along box axis ``los``: {"k", "mu", "power", "modes":
        (Nmesh/2-1, Nmu); "shotnoise"; "poles": {"k", "modes", "power_<l>"}} (device.fftpower_2d).  Accepts
        numpy arrays or CUDA tensors."""
        f1 = dev.as_device(value_map1, self.dtype)
        f2 = None if value_map2 is None else dev.as_device(value_map2, self.dtype)
        n = int(self.sim.domain_level)
        if tuple(f1.shape) != (n, n, n):
            raise PowerSpectrum3DWarning(f"value_map shape {tuple(f1.shape)} does not match Nmesh={n}")
        return dev.fftpower_2d(f1, self.sim.boxsize, f2, Nmu=Nmu, los=los, poles=poles)

    def _power_spectrum_2d_catalog(self, pos1, mass1=None, pos2=None, mass2=None, vel1=None, vel2=None,
                                   rsd_factor: float = 0.01, window: str = "tsc", interlaced: bool = True,
                                   compensated: bool = True, Nmu: int = 5, los: int = 2, poles=(0, 2, 4)) -> dict:
        """The same for PARTICLE catalogues with the mesh parameters of :meth:`_power_spectrum_3d_catalog`; with
        velocities the catalogue is moved to redshift space first, ``pos[:, los] += rsd_factor * vel[:, los]`` and one
        periodic wrap (TPCF's shift).  The shot noise is reported in the dict, not subtracted."""
        as_dev = lambda a: None if a is None else dev.as_device(np.ascontiguousarray(a), self.dtype)
        return dev.catalog_power_2d(as_dev(pos1), as_dev(mass1), int(self.sim.domain_level), self.sim.boxsize, window,
                                    interlaced, compensated, pos2=as_dev(pos2), mass2=as_dev(mass2), vel1=as_dev(vel1),
                                    vel2=as_dev(vel2), rsd_factor=rsd_factor, Nmu=Nmu, los=los, poles=poles)

    @staticmethod
    def _frames_2d(res: dict):
        """(wedge frame: index k of the shell, one column per mu-bin centre; poles frame: index k, columns P<l>, modes)
        of one snapshot's mode-2d result."""
        nmu = res["power"].shape[1]
        k1 = res["poles"]["k"]
        wedges = pd.DataFrame(res["power"], index=pd.Index(k1, name="k"), columns=(np.arange(nmu) + 0.5) / nmu)
        cols = {"P%s" % key[len("power_"):]: val for key, val in res["poles"].items() if key.startswith("power_")}
        cols["modes"] = res["poles"]["modes"]
        return wedges, pd.DataFrame(cols, index=pd.Index(k1, name="k"))

    def _save_results_2d(self, quantity: List[str], pkmu: dict) -> None:
        """Per snapshot the frames of :meth:`_frames_2d` under the keys snap_%d_pkmu and snap_%d_poles ->
        pkmu_<quantity>.h5."""
        filename = self.sim.dirs["out"] + "pkmu_%s.h5" % (("_").join(quantity))
        IO._remove_existing_file(filename)
        print(f"Saving results to -> {filename}")
        first = True
        for snap, res in pkmu.items():
            for frame, name in zip(self._frames_2d(res), ("pkmu", "poles")):
                frame.to_hdf(filename, key="%s_%s" % (snap, name), mode="w" if first else "a")
                first = False

    def _save_results(self, quantity: List[str], pk: dict) -> None:
        """DataFrame(index=k, columns=snap_%d) -> pk_<quantity>.h5 (power_spectrum_3d.py:228-249)."""
        _columns = list(pk["k"].keys())
        df = pd.DataFrame(data=pk["P"], index=pk["k"][_columns[0]])
        filename = self.sim.dirs["out"] + "pk_%s.h5" % (("_").join(quantity))
        IO._remove_existing_file(filename)
        print(f"Saving results to -> {filename}")
        df.to_hdf(filename, key="df", mode="w")
