from .stats_subfind import SubFind  # noqa: F401
from .mean_pairwise_velocity import (make_rsep, make_rsep_uneven_bins, mean_pv_from_tv, mean_pv_radial,  # noqa: F401
                                     mean_pv_z_sign)
from .pair_velocity_box import (los_pvd_vs_rp, mean_los_velocity_vs_rp, mean_radial_velocity_vs_r,  # noqa: F401
                                radial_pvd_vs_r)
from .tpcf import (TPCF, rp_pi_tpcf, rp_pi_tpcf_jackknife, s_mu_tpcf, tpcf_jackknife, tpcf_multipole,  # noqa: F401
                   tpcf_r, wp, wp_from_xi, wp_jackknife)
from .fof import FOF, FoFGroups, check_fof_args, fof_features, fof_groups  # noqa: F401
from .readout import check_readout_args, density_at, readout  # noqa: F401
from .map_transform import MapTransform, MapTransformWarning  # noqa: F401
