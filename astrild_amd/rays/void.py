"""Voids on sky maps: the reference's ``astrild.rays.void.Voids`` (rays/void.py) for the profile statistics.

``get_profiles`` (:188-257) measures every void's radial profile on the GPU (``profiles.profile_2d.from_map``);
``get_profile_stats`` (:259-410) averages them with the reference's host statistics.  Deliberate differences:

* ``get_profile_stats`` stores its result as a dict of numpy arrays on ``self.profile_stats`` and returns it (the
  reference builds an xarray Dataset and drops it); ``save=True`` needs xarray and raises ImportError without it.
* ``field_conversion="normalize"`` subtracts the map's mean from a copy; the caller's array is left as it is.
* ``from_file`` reads "tunnels" and "wvf" catalogues from a given file; "svf" and "zobov" (whose reference code uses an
  undefined ``args``) and file discovery through ``file_dsc`` raise NotImplementedError.
* nothing is printed.
"""
import numpy as np

from ..profiles import profile_2d as Profiles2D
from .utils import object_selection


class VoidsWarning(BaseException):
    pass


def _read_skymap(file_in):
    """A map stored as .npy, or as .npz under "arr_0" (lenstools' key)."""
    ext = file_in.split(".")[-1]
    if ext == "npy":
        return np.load(file_in)
    if ext == "npz":
        return np.load(file_in)["arr_0"]
    raise ValueError(f"unknown skymap file type: {file_in}")


def _normalized(skymap):
    """skymap - mean(skymap) as a new map (numpy: np.mean, as the reference's in-place ``-=``).  A device tensor is not
    copied: the mean (fixed-order device sum) is returned with it and subtracted from the annulus sums instead."""
    import torch
    if isinstance(skymap, torch.Tensor):
        from .. import device as dev
        t = dev.as_device(skymap)
        return t, dev.total_mass(t, t.numel()) / t.numel()
    skymap = np.asarray(skymap)
    return skymap - np.mean(skymap), 0.0


def _profiles(data, skymap, extend, nbins, field_conversion):
    if field_conversion == "normalize":
        skymap, mean = _normalized(skymap)
        if mean != 0.0:
            out = Profiles2D.from_map(data, skymap, extend, nbins, return_counts=True)
            sums = out.pop("sums") - mean * out["counts"]
            out["values"] = Profiles2D.aligned_values(sums, out.pop("counts"))
            return out
    return Profiles2D.from_map(data, skymap, extend, nbins)


def _profile_stats(obj, cats, save):
    """Voids.get_profile_stats / Peaks.get_profile_stats (void.py:259-410, peak.py:143-239) as a dict of arrays."""
    radii = obj.profiles["radii"]
    nr_rad_bins = len(radii)
    extend = radii.max()

    def one(cat):
        mean = Profiles2D.mean_and_interpolate(obj.profiles["values"][cat.index.values, :], cat["rad_pix"].values,
                                               extend, nr_rad_bins)
        if obj.field_conversion == "tangential_shear":
            mean = obj._compute_tangential_shear(radii, mean)
        err = Profiles2D.bootstrapping(obj.profiles["values"][cat.index.values, :], mean, cat, obj.skymap_dsc["npix"],
                                       extend, nr_rad_bins)
        return mean, err[0, :], err[1, :], cat["rad_deg"].min(), cat["rad_deg"].max(), len(cat.index)

    if cats:
        sigmas = np.unique(obj.data["sigma"].values)
        shape = tuple(len(np.unique(obj.data[c].values)) for c in cats)
        res = {k: np.zeros(shape + (nr_rad_bins,)) for k in ("mean", "lowerr", "higherr")}
        res.update({k: np.zeros(shape) for k in ("size_min", "size_max", "nr_of_obj")})
        for ss, sigma in enumerate(sigmas):
            vals = one(obj.data.loc[obj.data["sigma"] == sigma])
            for k, v in zip(("mean", "lowerr", "higherr", "size_min", "size_max", "nr_of_obj"), vals):
                res[k][ss] = v
        res["sigma"] = sigmas
    else:
        vals = one(obj.data)
        res = {k: np.asarray(v, dtype=np.float64).reshape(-1 if i < 3 else 1)
               for i, (k, v) in enumerate(zip(("mean", "lowerr", "higherr", "size_min", "size_max", "nr_of_obj"),
                                              vals))}
    res["radius"] = radii
    obj.profile_stats = res
    if save:
        _save_stats(obj, res, cats)
    return res


def _save_stats(obj, res, cats):
    import xarray as xr     # ImportError without xarray
    dims = list(cats) if cats else []
    data = {k: (dims + ["radius"], res[k]) for k in ("mean", "lowerr", "higherr")}
    coords = {"radius": res["radius"]}
    coords.update({k: (dims, res[k]) if dims else res[k] for k in ("size_min", "size_max", "nr_of_obj")})
    if cats:
        coords["sigma"] = res["sigma"]
    dir_out = "/".join(obj.dataset_file.split("/")[:-1])
    conv = obj.field_conversion or ""
    name = conv + "_" + "".join(obj.dataset_file.split("/")[-1].split(".")[:-1])
    xr.Dataset(data, coords=coords).to_netcdf(f"{dir_out}/profile_{name}.nc")


def _tangential_shear(rad, prof):
    """gamma_t(r) = (2 pi / (pi r^2)) int_0^r r' kappa(r') dr' - kappa(r), kappa linearly interpolated (and
    extrapolated) through the profile (void.py:495-512)."""
    from scipy import integrate
    from scipy.interpolate import interp1d
    kappa_r = interp1d(rad, prof, fill_value="extrapolate")
    shear = np.zeros(len(rad))
    for i in range(len(rad)):
        val = integrate.quad(lambda r: 2 * np.pi * r * kappa_r(r), 0, rad[i])[0]
        shear[i] = val / (np.pi * rad[i] ** 2) - prof[i]
    return shear


class Voids:
    """Void catalogue (a DataFrame with x_pix, y_pix, rad_pix, rad_deg, sigma, and theta1_pix / theta2_pix for the edge
    trim) of a sky map described by ``skymap_dsc`` ({"file", "npix"})."""

    def __init__(self, dataset_file, data, finder_spec, skymap_dsc):
        self.dataset_file = dataset_file
        self.data = data
        self.finder_spec = finder_spec
        self.skymap_dsc = skymap_dsc

    @classmethod
    def from_file(cls, finder, skymap_dsc, ffile=None, file_dsc=None):
        """Read a "tunnels" or "wvf" catalogue (pandas HDF5, key "df") from ``ffile``."""
        import pandas as pd
        if finder in ("svf", "zobov"):
            raise NotImplementedError(f"the {finder} reader is not carried over")
        if ffile is None:
            raise NotImplementedError("file discovery through file_dsc is not carried over: pass ffile")
        if finder == "tunnels":
            data = pd.read_hdf(ffile, key="df")
            spec = {"name": finder, "sigmas": {"name": "sigma", "values": data["sigma"].unique()}}
        elif finder == "wvf":
            data = pd.read_hdf(ffile, key="df")
            spec = {"name": finder}
        else:
            raise ValueError(f"unknown void finder {finder!r}")
        return cls(ffile, data, spec, skymap_dsc)

    def _read_skymap(self, file_in):
        return _read_skymap(file_in)

    def get_profiles(self, radii_max, nr_rad_bins, void_resolution=10, skymap_file=None, skymap=None,
                     field_conversion=None, dir_out=None, save=False):
        """Radial profiles of the voids out to ``radii_max`` void radii in ``nr_rad_bins`` annuli -> self.profiles.
        Tunnels / wvf voids crossing the map edge are dropped first, then those with radii_max * rad_pix <=
        void_resolution (each step followed by reset_index, as in the reference)."""
        self.field_conversion = field_conversion
        if skymap is None:
            skymap = self._read_skymap(self.skymap_dsc["file"] if skymap_file is None else skymap_file)
        if self.finder_spec["name"] in ("tunnels", "wvf"):
            self.data = self._trim_edges(self.data, radii_max, self.skymap_dsc["npix"])
            self.data = self.data.reset_index()
        self.data = self.data[radii_max * self.data["rad_pix"] > void_resolution]
        self.data = self.data.reset_index()
        self.profiles = _profiles(self.data, skymap, radii_max, nr_rad_bins, field_conversion)
        if save:
            import pandas as pd
            dir_out = "/".join(self.dataset_file.split("/")[:-1])
            conv = self.field_conversion or ""
            name = conv + "_" + "".join(self.dataset_file.split("/")[-1].split(".")[:-1])
            pd.DataFrame(data=self.profiles["values"].T, index=self.profiles["radii"],
                         columns=self.data.index.values).to_hdf(f"{dir_out}/signle_profiles_{name}.h5", key="df",
                                                                mode="w")

    def get_profile_stats(self, cats=None, field_conversion=None, dir_out=None, save=False):
        """Mean profile (weighted by rad_pix^2) and bootstrap errors, per "sigma" when ``cats`` is given, else of all
        voids: {"mean", "lowerr", "higherr", "size_min", "size_max", "nr_of_obj", "radius"[, "sigma"]}."""
        if field_conversion:
            self.field_conversion = field_conversion
        return _profile_stats(self, cats, save)

    def _trim_edges(self, voids, radii_max, npix):
        return object_selection.trim_dataframe_of_objects_crossing_edge(voids, radii_max, npix)

    def categorize_sizes(self, bins, min_obj_nr):
        self.data = object_selection.categorize_sizes(self.data, "log", bins, min_obj_nr)

    def _compute_tangential_shear(self, rad, prof):
        return _tangential_shear(rad, prof)
