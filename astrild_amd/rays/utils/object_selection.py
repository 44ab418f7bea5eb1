"""Selection of object catalogues (voids, peaks): the reference's ``astrild.rays.utils.object_selection``
(``categorize_sizes``, :7-34, and ``trim_dataframe_of_objects_crossing_edge``, :80-114).  ``minimal_voids`` is not
carried over (it indexes DataFrames as nested dicts)."""
import numpy as np


def categorize_sizes(objects, binning_method, nr_size_cats, min_obj_nr):
    """Adds column "size_cat" = np.digitize(size, linspace(min, max, nr_size_cats), right=True) to ``objects`` (in
    place, as the reference does), size = log10(rad_deg) for "log" and rad_deg otherwise, and returns the rows whose
    category holds at least ``min_obj_nr`` objects."""
    size = objects["rad_deg"].values
    if binning_method == "log":
        size = np.log10(size)
    edges = np.linspace(size.min(), size.max(), nr_size_cats)
    objects["size_cat"] = np.digitize(size, edges, right=True)
    cats, count = np.unique(objects["size_cat"].values, return_counts=True)
    return objects.loc[objects["size_cat"].isin(cats[count >= min_obj_nr])]


def trim_dataframe_of_objects_crossing_edge(data, extend, npix, key_size="rad_pix", rtn="DataFrame"):
    """Objects whose extent, extend * data[key_size] pixels, stays strictly inside (0, npix) on both axes (columns
    theta1_pix, theta2_pix).  rtn="bool": the boolean mask; "index": the positions where it is True; anything else: the
    rows of ``data``."""
    reach = extend * data[key_size].values
    t1, t2 = data["theta1_pix"].values, data["theta2_pix"].values
    inside = (t1 + reach < npix) & (t1 - reach > 0) & (t2 + reach < npix) & (t2 - reach > 0)
    if rtn == "bool":
        return inside
    if rtn == "index":
        return np.arange(len(inside))[inside]
    return data[inside]
