"""The tunnels void finder on sky maps: the reference's ``astrild.rays.voids.tunnel.TunnelsFinder`` (Cautun et al.,
arXiv:1710.01730).  Tracers are the peaks of a convergence map; a void is a circle through at least three tracers with
no tracer strictly inside, i.e. a circumcircle of the tracers' Delaunay triangulation, each distinct circle once, kept
when its centre lies in the map.

The reference writes the peaks to a text file, converts it to a binary file and runs an external program,
``void_finder_spherical_2D``, whose result it reads back.  Here the peaks come from ``lensing.peak_find`` on the
resident map and the voids from ``device.tunnels_voids`` (``ast_tunnels_find``), in exact integer arithmetic on the
GPU.  Since the external program is not available, the result is defined by the sentence above, not by parity with it.

Deliberate differences:

* ``find_peaks`` takes ``smoothing_length`` (arcmin, default 0: no buffer) for the edge buffer of
  ``_remove_peaks_crossing_edge``; the reference reads ``skymap.smoothing_length``, which its SkyArray never sets.
* ``pos[:, 0]`` is x, the column of the map, and ``pos[:, 1]`` is y, the row, both times ``opening_angle / npix``
  degrees.  This is what ``profile_2d.from_map`` reads as ``x_pix`` / ``y_pix``.
* the voids frame has the reference's columns and also ``theta1_pix`` / ``theta2_pix``, the centre in pixels before
  rounding, which ``Voids._trim_edges`` reads (the reference's trim reads them too, and its tunnels frame lacks them).
* the integer records of each threshold are kept on ``self.void_records``.
* a threshold that leaves fewer than three peaks, or no void, contributes empty frames.
* nothing is printed, no temporary file is written, ``dir_temp`` is accepted and ignored.
* only the overlapping run (``-l 0.``) exists; the file-format helpers (``_txt2bin``, ``_peaks2txt``, ...) are not
  carried over.
"""
from typing import List, Optional, Tuple

import numpy as np
import pandas as pd

from ... import device as dev
from ... import lensing
from .. import peak as Peaks
from .._resident import to_host
from ..skyio import SkyIO

VOID_COLUMNS = ["x_deg", "x_pix", "y_deg", "y_pix", "rad_deg", "rad_pix", "sigma", "theta1_pix", "theta2_pix"]
PEAK_COLUMNS = ["x_deg", "x_pix", "y_deg", "y_pix", "sigma", "rad_deg", "rad_pix"]
_INT_COLUMNS = ("x_pix", "y_pix", "rad_pix")


class TunnelsFinderWarning(BaseException):
    pass


def _empty(columns):
    return pd.DataFrame({c: np.zeros(0, dtype=np.int64 if c in _INT_COLUMNS else np.float64) for c in columns})


class TunnelsFinder:
    def __init__(self, skymap):
        self.skymap = skymap

    def find_peaks(self, on: str, field_conversion: str, thresholds_dsc: dict, snr_sigma: Optional[float] = None,
                   save: bool = False, smoothing_length: float = 0.0) -> None:
        """Peaks of ``skymap.data[on]`` -> self.peaks = {"kappa", "pos", "snr"}: strict 8-neighbour maxima of the interior
        (lenstools' ``locatePeaks``) with thresholds[0] <= height < thresholds[-1], heights of (map - mean) for
        "normalize", those within the edge buffer removed, snr = height / std(map) or / ``snr_sigma``."""
        self.on = on
        self.smoothing_length = smoothing_length
        t = self.skymap.data.device(on)
        host = np.asarray(to_host(t), dtype=np.float64)         # a copy for numpy's mean and std; the map stays resident
        mean = np.mean(host) if field_conversion == "normalize" else 0.0
        thresholds = self._get_convergence_thresholds(**thresholds_dsc)
        heights, index = lensing.peak_find(t)
        heights = np.asarray(heights, dtype=np.float64) - mean if field_conversion == "normalize" else heights
        keep = (heights >= thresholds[0]) & (heights < thresholds[-1])
        heights, index = heights[keep], index[keep]
        npix = self.skymap.npix
        pos = np.stack([index % npix, index // npix], axis=1) * (self.skymap.opening_angle / npix)
        _peaks = {}
        _peaks["kappa"], _peaks["pos"] = self._remove_peaks_crossing_edge(heights, pos)
        assert len(_peaks["kappa"]) != 0, "No peaks"
        _peaks["snr"] = self._signal_to_noise_ratio(_peaks["kappa"], host - mean, snr_sigma)
        self.peaks = _peaks

    def _get_convergence_thresholds(self, on: str = "orig", nbins: int = 100) -> np.ndarray:
        data = to_host(self.skymap.data.device(on))
        lo, hi = np.min(data), np.max(data)
        return np.arange(lo, hi, (hi - lo) / nbins)

    def _signal_to_noise_ratio(self, peak_values: np.ndarray, map_values: np.ndarray,
                               sigma: Optional[float] = None) -> np.ndarray:
        if sigma is None:
            return peak_values / np.std(map_values)
        return peak_values / sigma

    def _remove_peaks_crossing_edge(self, kappa: np.ndarray, pos: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """Drop the peaks within one smoothing length of the map's edges."""
        npix, angle = self.skymap.npix, self.skymap.opening_angle
        pixlen = angle / npix
        bufferlen = np.ceil(getattr(self, "smoothing_length", 0.0) / (60 * pixlen))
        x = pos[:, 0] * npix / angle
        y = pos[:, 1] * npix / angle
        indx = np.logical_and(np.logical_and(x <= npix - 1 - bufferlen, x >= bufferlen),
                              np.logical_and(y <= npix - 1 - bufferlen, y >= bufferlen))
        return kappa[indx], pos[indx, :]

    def find_voids(self, snrs: List[float], dir_temp: Optional[str] = None, rtn: bool = False):
        """For every threshold nu in ``snrs``: the tunnels voids of the peaks with snr > nu.  The frames of all
        thresholds, concatenated, go to self.voids_df / self.peaks_df (or are returned as (peaks, voids) with ``rtn``)."""
        npix, angle = self.skymap.npix, self.skymap.opening_angle
        voids_all, peaks_all = [], []
        self.void_records = {}
        for snr in snrs:
            idx = self.peaks["snr"] > snr
            pos_tmp = self.peaks["pos"][idx, :]
            x_pix = np.rint(pos_tmp[:, 0] * npix / angle).astype(int)
            y_pix = np.rint(pos_tmp[:, 1] * npix / angle).astype(int)
            records = dev.tunnels_voids(x_pix, y_pix, npix)
            self.void_records[snr] = records
            self.voids = self._records_to_df(records, x_pix, y_pix, snr)
            if len(records) == 0:
                self.filtered_peaks = _empty(PEAK_COLUMNS)
                continue
            peaks_df = pd.DataFrame(data={"x_deg": pos_tmp[:, 0], "x_pix": x_pix, "y_deg": pos_tmp[:, 1],
                                          "y_pix": y_pix, "sigma": snr})
            self.filtered_peaks = self.set_peak_radii(peaks_df, self.voids, npix, angle)
            voids_all.append(self.voids)
            peaks_all.append(self.filtered_peaks)
        voids_df_sum = pd.concat(voids_all, ignore_index=True) if voids_all else _empty(VOID_COLUMNS)
        peaks_df_sum = pd.concat(peaks_all, ignore_index=True) if peaks_all else _empty(PEAK_COLUMNS)
        self.peaks_orig_df = pd.DataFrame(data=self.peaks["snr"])
        if rtn:
            return peaks_df_sum, voids_df_sum
        self.peaks_df = peaks_df_sum
        self.voids_df = voids_df_sum

    def _records_to_df(self, records, x_pix, y_pix, sigma) -> pd.DataFrame:
        npix, angle = self.skymap.npix, self.skymap.opening_angle
        if len(records) == 0:
            return _empty(VOID_COLUMNS)
        cx, cy, r = dev.tunnels_circles(records, x_pix, y_pix)
        x_deg, y_deg, rad_deg = cx * (angle / npix), cy * (angle / npix), r * (angle / npix)
        void_df = pd.DataFrame(data={
            "x_deg": x_deg, "x_pix": np.rint(x_deg * npix / angle).astype(int),
            "y_deg": y_deg, "y_pix": np.rint(y_deg * npix / angle).astype(int),
            "rad_deg": rad_deg, "rad_pix": np.rint(rad_deg * npix / angle).astype(int)})
        void_df["sigma"] = sigma
        void_df["theta1_pix"] = cx
        void_df["theta2_pix"] = cy
        return void_df

    def set_peak_radii(self, peaks: pd.DataFrame, voids: pd.DataFrame, npix, opening_angle) -> pd.DataFrame:
        return Peaks.set_radii(peaks, voids, npix, opening_angle)

    def to_file(self, dir_out: str) -> None:
        """The voids and the peaks' snr as pandas HDF5 files (key "df") in ``dir_out``."""
        self.voids_df.to_hdf(self._create_filename(obj="voids", dir_out=dir_out, on=self.on), key="df")
        self.peaks_orig_df.to_hdf(self._create_filename(obj="peaks", dir_out=dir_out, on=self.on), key="df")

    def _create_filename(self, obj: str, dir_out: str, on: str) -> str:
        _filename = SkyIO._create_filename(self.skymap.map_file, self.skymap.quantity, on, extension="_")
        _filename = "".join(_filename.split(".")[:-1])
        return f"{dir_out}/{obj}_{_filename}.h5"
