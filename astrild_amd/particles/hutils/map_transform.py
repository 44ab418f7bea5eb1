"""``MapTransform`` with astrild's API (src/astrild/particles/hutils/map_transform.py): the divergence of gridded vector
fields, computed on the GPU (``device.divergence``, one streaming stencil kernel) with numpy's arithmetic bit for bit.

What the reference does (map_transform.py:29-118) and what is kept:

* ``divergence`` resolves the files of ``file_dsc`` under ``directory`` (default ``sim.dirs["sim"]``) through the
  simulation object, reads each one, and writes ``div_<file name>`` beside it, or with ``save=False`` returns the first
  snapshot's array.  An explicit ``snap_nrs`` must be a proper subset of ``sim.dir_nrs``: the reference asserts it
  with ``set(snap_nrs) < set(sim.dir_nrs)``, and so does this port, with the same message.
* ``.npy`` files are read as they are; ``.h5`` tables are scatter-assigned to a 3D grid of ``sim.npar`` cells a side.
  Anything that is not 4D raises ``MapTransformWarning(f"{ndim}D is not supported yet.")``.
* ``_compute_divergence`` is ``np.gradient(value_map[:, :, :, a], 1 / sim.boxsize, axis=a, edge_order=2)`` summed over
  a = 0, 1, 2.  **The spacing 1 / boxsize is the reference's**, although a cell is boxsize / N wide: the result is the
  divergence in physical units times the constant boxsize^2 / N.  Parity is the default here too; ``spacing=`` takes
  the true cell width (or any other) from whoever wants physical units.
* Results are written with ``np.save``, which appends ``.npy`` to a name that does not end in it.

Added here: ``.a_vel`` DTFE binaries (``formats.read_density_grid``) go from the file straight to the device;
``periodic=True`` replaces numpy's one-sided edge formulas by central differences with wrapped indices, which is what
a periodic simulation box calls for; ``_compute_divergence`` accepts a device tensor and then returns one, so that a
result can feed ``PowerSpectrum3D._power_spectrum_3d`` without leaving HBM.
"""
from typing import Dict, List, Optional

import numpy as np


class MapTransformWarning(BaseException):
    pass


class MapTransform:
    """
    Attributes:
        sim_type:
        simulation: object exposing .boxsize, .npar, .dirs, .dir_nrs, .get_file_nrs(), .get_file_paths()
            (astrild.simulation.Simulation)

    Methods:
        divergence:
    """

    def __init__(self, sim_type: str, simulation):
        self.sim = simulation
        self.sim.type = sim_type

    def divergence(
        self,
        quantity: Optional[str] = None,
        snap_nrs: Optional[List[int]] = None,
        file_dsc: Dict[str, str] = {"root": "dtfe", "extension": "npy"},
        directory: Optional[str] = None,
        save: bool = True,
        periodic: bool = False,
        spacing: Optional[float] = None,
    ):
        """Divergence of the vector grids in the files of ``file_dsc``, one per snapshot (map_transform.py:29-68).
        ``save``: write ``div_<file name>`` (numpy ``.npy``) beside each input; otherwise return the first snapshot's
        divergence as a numpy array.  ``spacing=None`` is the reference's ``1 / sim.boxsize``."""
        if not directory:
            directory = self.sim.dirs["sim"]
        if snap_nrs:
            assert set(snap_nrs) < set(self.sim.dir_nrs), MapTransformWarning(
                f"Some of the snapshots {snap_nrs} do not exist" + f"in:\n{self.sim.dir_nrs}"
            )
            _file_paths = self.sim.get_file_paths(file_dsc, directory, "max")
        else:
            snap_nrs = self.sim.get_file_nrs(file_dsc, directory, "max")
            _file_paths = self.sim.get_file_paths(file_dsc, directory, "max")

        for snap_nr, file_path in zip(snap_nrs, _file_paths):
            _value_map = self._read_data(file_path, quantity)
            if len(_value_map.shape) == 4:
                _value_map = self._compute_divergence(_value_map, periodic=periodic, spacing=spacing)
            else:
                raise MapTransformWarning(f"{len(_value_map.shape)}D is not supported yet.")
            if not isinstance(_value_map, np.ndarray):
                from ... import device as dev
                _value_map = dev.to_numpy(_value_map)
            if save:
                self._save_results("div_", file_path, _value_map)
            else:
                return _value_map

    def _read_data(self, file_in: str, quantity: Optional[str] = None):
        """A ``.npy`` grid as it is, a ``.h5`` table of astrild.particles.ecosmog.dtfe() as a 3D grid (numpy arrays,
        map_transform.py:71-89), or a DTFE ``.a_vel`` binary as a device tensor ``(gx, gy, gz, 3)``."""
        value_map = np.zeros((self.sim.npar, self.sim.npar, self.sim.npar))
        if ".h5" in file_in:
            import pandas as pd
            fields = pd.read_hdf(file_in, key="df")
            x = (self.sim.npar * fields["x"].values).astype(int)
            y = (self.sim.npar * fields["y"].values).astype(int)
            z = (self.sim.npar * fields["z"].values).astype(int)
            value_map[(x, y, z)] = fields[quantity].values
        elif ".npy" in file_in:
            value_map = np.load(file_in)
        elif file_in.endswith(".a_vel"):
            from ...formats import read_density_grid
            value_map = read_density_grid(file_in)[1]
        return value_map

    def _compute_divergence(self, value_map, periodic: bool = False, spacing: Optional[float] = None):
        """Vector divergence field, nabla^i v_i, of a ``(N0, N1, N2, 3)`` grid: numpy array in, numpy array out; device
        tensor in, device tensor out."""
        from ... import device as dev
        h = 1 / self.sim.boxsize if spacing is None else spacing
        dev.check_divergence_args(value_map.shape, value_map.dtype, h)
        div_v = dev.divergence(value_map, h, periodic=periodic)
        return div_v if hasattr(value_map, "is_cuda") else dev.to_numpy(div_v)

    @staticmethod
    def _result_path(file_tag: str, file_path: str) -> str:
        """``<directory of file_path>/<file_tag><file name>`` (map_transform.py:113-115)."""
        directory = file_path.split("/")[:-1]
        file_name = file_tag + file_path.split("/")[-1]
        return "/".join(directory) + "/" + file_name

    def _save_results(self, file_tag: str, file_path: str, value_map: np.ndarray) -> None:
        file_out = self._result_path(file_tag, file_path)
        print(f"Save result in -> {file_out}")
        np.save(file_out, value_map)
