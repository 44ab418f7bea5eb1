"""The watershed void finder on sky maps: the reference's ``astrild.rays.voids.watershed.WatershedFinder``.

A void is a basin of the map, or a union of basins that shallow passes connect.  Pixels are ordered by (value, flat
index); every pixel links to the smallest of itself and its up-to-8 neighbours inside the map; a basin is the set of
pixels whose links end at the same minimum.  The pass between two basins is the lowest max(f[p], f[q]) over their
8-adjacent pixel pairs.  At a boundary height h the passes are taken in ascending (height, a, b), and two sets merge
when the pass lies less than h above the higher of their two lowest minima; every final set is one void, with the
centroid of its pixels as centre and sqrt(area / pi) as radius.  DESIGN.md 6j has the full definition.

The reference's class only has ``to_file`` and ``_create_filename`` next to file-format helpers for an external
program, and its ``rays/utils/watershed_voids.py`` does not run.  So, as for the tunnels finder, the result is defined
by the sentences above, not by parity with a program.  The basins come from ``device.watershed_basins``
(``ast_watershed_*``) on the resident map, the merge from ``device.watershed_merge`` on the host, the void maps from
``device.watershed_void_map``.

The finder does no smoothing and no down-sampling of its own: call ``SkyArray.filter`` (e.g. ``{"gaussian": {...}}``)
first and pass the filtered map's name as ``on``.

Deliberate differences:

* ``find_voids`` exists (the reference's class cannot find anything); ``boundary_heights`` are in units of the map's
  standard deviation, or of ``snr_sigma`` when that is given.
* no compensated top-hat, no distance transform, no DBSCAN, no skimage: minima on the border and in the corners of
  the map are legal, and plateaus are split by the lower flat index.
* ``x_*`` is the column of the map and ``y_*`` the row, as in ``TunnelsFinder`` and ``profile_2d.from_map``; the
  frame has tunnels' columns (``theta1_pix`` / ``theta2_pix``: the centre before rounding, which
  ``Voids._trim_edges`` reads) and also ``area_pix``, ``edge_pix``, ``kappa_min``, ``kappa_mean``, ``x_min_pix``,
  ``y_min_pix`` (the position of the void's lowest pixel) and ``void_id`` (its value on ``self.void_maps[nu]``).
* ``to_file`` writes the voids only: there are no peaks.
* nothing is printed and no temporary file is written.
"""
from typing import List, Optional

import numpy as np
import pandas as pd

from ... import device as dev
from .._resident import to_host
from ..skyio import SkyIO
from .tunnel import VOID_COLUMNS, _INT_COLUMNS

WATERSHED_COLUMNS = VOID_COLUMNS + ["area_pix", "edge_pix", "kappa_min", "kappa_mean", "x_min_pix", "y_min_pix",
                                    "void_id"]
_WS_INT_COLUMNS = _INT_COLUMNS + ("area_pix", "edge_pix", "x_min_pix", "y_min_pix", "void_id")


class WatershedFinderWarning(BaseException):
    pass


def _empty():
    return pd.DataFrame({c: np.zeros(0, dtype=np.int64 if c in _WS_INT_COLUMNS else np.float64)
                         for c in WATERSHED_COLUMNS})


class WatershedFinder:
    def __init__(self, skymap):
        self.skymap = skymap

    def find_voids(self, on: str, boundary_heights: List[float], snr_sigma: Optional[float] = None,
                   min_rad_pix: float = 0.0, rtn: bool = False):
        """The watershed voids of ``skymap.data[on]`` at every boundary height nu of ``boundary_heights``: the basins
        are found once, then merged at h = nu * std(map) (or nu * ``snr_sigma``).  The frames of all heights,
        concatenated with nu in the column ``sigma``, go to self.voids_df (or are returned with ``rtn``); the int32
        void map of every height to self.void_maps[nu], the basins to self.basins.  Voids with
        sqrt(area / pi) <= ``min_rad_pix`` are left out of the frame (they stay on the void map)."""
        self.on = on
        t = self.skymap.data.device(on)
        unit = float(np.std(np.asarray(to_host(t), dtype=np.float64))) if snr_sigma is None else float(snr_sigma)
        self.basins = dev.watershed_basins(t)
        host = {k: to_host(v) for k, v in self.basins.items() if k != "labels"}
        self.void_maps = {}
        frames = []
        for nu in boundary_heights:
            h = float(nu) if nu == 0 or np.isinf(nu) else float(nu) * unit      # 0 * inf is not a height
            merged = dev.watershed_merge(host, h)
            self.void_maps[nu] = to_host(dev.watershed_void_map(self.basins, merged["void_of_basin"]))
            self.voids = self._merged_to_df(merged, nu, min_rad_pix)
            frames.append(self.voids)
        voids_df_sum = pd.concat(frames, ignore_index=True) if frames else _empty()
        if rtn:
            return voids_df_sum
        self.voids_df = voids_df_sum

    def _merged_to_df(self, merged, sigma, min_rad_pix) -> pd.DataFrame:
        npix, angle = self.skymap.npix, self.skymap.opening_angle
        area = merged["area"].astype(np.float64)
        cx, cy, r = merged["sum_x"] / area, merged["sum_y"] / area, np.sqrt(area / np.pi)
        x_deg, y_deg, rad_deg = cx * (angle / npix), cy * (angle / npix), r * (angle / npix)
        void_df = pd.DataFrame(data={
            "x_deg": x_deg, "x_pix": np.rint(cx).astype(int),
            "y_deg": y_deg, "y_pix": np.rint(cy).astype(int),
            "rad_deg": rad_deg, "rad_pix": np.rint(r).astype(int)})
        void_df["sigma"] = sigma
        void_df["theta1_pix"] = cx
        void_df["theta2_pix"] = cy
        void_df["area_pix"] = merged["area"]
        void_df["edge_pix"] = merged["edge_pix"]
        void_df["kappa_min"] = merged["kappa_min"].astype(np.float64)
        void_df["kappa_mean"] = merged["sum_f"] / area
        void_df["x_min_pix"] = merged["min_index"] % npix
        void_df["y_min_pix"] = merged["min_index"] // npix
        void_df["void_id"] = np.arange(len(area), dtype=np.int64)
        return void_df[r > min_rad_pix].reset_index(drop=True)

    def to_file(self, dir_out: str) -> None:
        """The voids as a pandas HDF5 file (key "df") in ``dir_out``: what ``Voids.from_file("wvf", ...)`` reads."""
        self.voids_df.to_hdf(self._create_filename(obj="voids", dir_out=dir_out, on=self.on), key="df")

    def _create_filename(self, obj: str, dir_out: str, on: str) -> str:
        _filename = SkyIO._create_filename(self.skymap.map_file, self.skymap.quantity, on, extension="_")
        _filename = "".join(_filename.split(".")[:-1])
        return f"{dir_out}/{obj}_{_filename}.h5"
