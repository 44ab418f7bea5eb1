"""Peaks on sky maps: the reference's ``astrild.rays.peak`` (``Peaks``, ``set_radii``) for the profile statistics.

The reference's ``Peaks.get_profiles`` cannot run: for "tunnels" it calls ``object_selection.trim_edges``, which does
not exist (peak.py:241-252), and it passes five arguments to the four-parameter ``from_map`` (peak.py:139-141).  Here it
does what it evidently means: the ``Voids.get_profiles`` path without the resolution cut, trimmed with
``trim_dataframe_of_objects_crossing_edge``.  ``get_profile_stats`` returns a dict (see ``rays.void``); nothing is printed.
"""
import numpy as np

from .utils import object_selection
from .void import VoidsWarning, _profile_stats, _profiles, _read_skymap, _tangential_shear


class PeaksWarning(BaseException):
    pass


class Peaks:
    def __init__(self, dataset_file, data, finder_spec, skymap_dsc):
        self.dataset_file = dataset_file
        self.data = data
        self.finder_spec = finder_spec
        self.skymap_dsc = skymap_dsc

    @classmethod
    def from_file(cls, finder, skymap_dsc, _file=None, file_dsc=None):
        """Read a "tunnels" peak catalogue (pandas HDF5, key "df") from ``_file``."""
        import pandas as pd
        if _file is None:
            raise NotImplementedError("file discovery through file_dsc is not carried over: pass _file")
        if finder != "tunnels":
            raise ValueError(f"unknown peak finder {finder!r}")
        data = pd.read_hdf(_file, key="df")
        return cls(_file, data, {"name": finder, "sigmas": {"name": "sigma", "values": data["sigma"].unique()}},
                   skymap_dsc)

    def _read_skymap(self, file_in):
        return _read_skymap(file_in)

    def get_profiles(self, radii_max, nr_rad_bins, skymap_file=None, skymap=None, save=False, field_conversion=None,
                     dir_out=None):
        """Radial profiles of the peaks -> self.profiles; "tunnels" peaks crossing the map edge are dropped first."""
        self.field_conversion = field_conversion
        if skymap is None:
            skymap = self._read_skymap(self.skymap_dsc["file"] if skymap_file is None else skymap_file)
        if self.finder_spec["name"] == "tunnels":
            self.data = self._trim_edges(self.data, radii_max, self.skymap_dsc["npix"])
            self.data = self.data.reset_index()
        self.profiles = _profiles(self.data, skymap, radii_max, nr_rad_bins, field_conversion)

    def get_profile_stats(self, cats, field_conversion=None, dir_out=None, save=False):
        """As ``Voids.get_profile_stats`` with categories; a field_conversion contradicting the one of get_profiles
        raises VoidsWarning, as in the reference."""
        current = getattr(self, "field_conversion", None)
        if field_conversion is not None and current is not None and field_conversion != current:
            raise VoidsWarning("Contradictory field convergence")
        if field_conversion is not None:
            self.field_conversion = field_conversion
        return _profile_stats(self, cats, save)

    def _trim_edges(self, peaks, radii_max, npix):
        return object_selection.trim_dataframe_of_objects_crossing_edge(peaks, radii_max, npix)

    def categorize_sizes(self, bins, min_obj_nr):
        self.data = object_selection.categorize_sizes(self.data, "log", bins, min_obj_nr)

    def _compute_tangential_shear(self, rad, prof):
        return _tangential_shear(rad, prof)


def set_radii(peaks, voids, npix, opening_angle):
    """rad_deg = distance to the nearest void centre (x_deg, y_deg; cKDTree), rad_pix = its rint in pixels (peak.py:307-344).
    ``voids`` is a DataFrame or the dict layout {"pos_x": {"deg"}, "pos_y": {"deg"}}."""
    import pandas as pd
    from scipy.spatial import cKDTree
    peaks_pos = peaks[["x_deg", "y_deg"]].values
    if isinstance(voids, dict):
        voids_pos = np.stack([np.asarray(voids["pos_x"]["deg"]), np.asarray(voids["pos_y"]["deg"])], axis=1)
    else:
        voids_pos = np.stack([voids["x_deg"].values, voids["y_deg"].values], axis=1)
    distances, _ = cKDTree(voids_pos).query(peaks_pos, k=1)
    peaks["rad_deg"] = pd.Series(distances)
    peaks["rad_pix"] = peaks["rad_deg"].apply(lambda x: np.rint(x * (npix / opening_angle)).astype(int))
    return peaks
