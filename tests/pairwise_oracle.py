"""numpy restatement of the transverse-velocity pairwise estimator (mean_pv_from_tv / pairwise_one_row of the
reference's particles/hutils/mean_pairwise_velocity.py), fp64, vectorised per row i over j > i.  Same quirks as the
reference: binnr = len(bins), one bin width, a pair in bin int(d / binwidth) when that is below binnr, empty bins
dropped, coincident objects -> NaN in bin 0.  Distances are ((dx^2 + dy^2) + dz^2)^(1/2) in this order, like the GPU
kernel, so the per-bin pair counts are comparable exactly."""
import numpy as np


def angles_and_velocities(pos, vel_ang, theta1=None, theta2=None):
    """(u, t): unit position vectors and cartesian transverse velocities, t = J(th=theta2, ph=theta1)^T (0, v1, v2)
    with J = get_sph_to_cart_jacobian."""
    pos = np.asarray(pos, dtype=np.float64)
    vel = np.asarray(vel_ang, dtype=np.float64)
    if theta1 is None:
        ph = np.arctan(pos[:, 0] / pos[:, 2]) + 10 * np.pi / 180
        th = np.arctan(pos[:, 1] / pos[:, 2]) + 10 * np.pi / 180
    elif np.max(theta1) > 2 * np.pi:
        ph = np.deg2rad(np.asarray(theta1, dtype=np.float64))
        th = np.deg2rad(np.asarray(theta2, dtype=np.float64))
    else:
        ph = np.asarray(theta1, dtype=np.float64)
        th = np.asarray(theta2, dtype=np.float64)
    v1, v2 = vel[:, 0], vel[:, 1]
    t = np.stack([v1 * (np.cos(th) * np.cos(ph)) + v2 * -np.sin(ph),
                  v1 * (np.cos(th) * np.sin(ph)) + v2 * np.cos(ph),
                  v1 * -np.sin(th)], axis=1)
    nr = np.sqrt((pos[:, 0] * pos[:, 0] + pos[:, 1] * pos[:, 1]) + pos[:, 2] * pos[:, 2])
    return pos / nr[:, None], t


def pair_sums(pos, u, t, binnr, binwidth, rows=None, with_abs=False):
    """(nom, denom, counts) over all pairs i < j; `rows`: only these i (for timing a sample).  `with_abs`: also the
    per-bin sum of |term| of nom, for the error bound of a reordered sum (denom's terms are positive: it is its own)."""
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    nom = np.zeros(binnr)
    den = np.zeros(binnr)
    cnt = np.zeros(binnr, dtype=np.int64)
    sum_abs = np.zeros(binnr)
    for i in (range(n - 1) if rows is None else rows):
        d = pos[i] - pos[i + 1:]
        nrm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        with np.errstate(invalid="ignore", divide="ignore"):
            bf = nrm / binwidth
            ok = bf < binnr
            if not ok.any():
                continue
            b = bf[ok].astype(np.int64)
            p = d[ok] / nrm[ok, None]
            ui, uj = u[i], u[i + 1:][ok]
            di = (p[:, 0] * ui[0] + p[:, 1] * ui[1]) + p[:, 2] * ui[2]
            dj = (p[:, 0] * uj[:, 0] + p[:, 1] * uj[:, 1]) + p[:, 2] * uj[:, 2]
            q = 0.5 * ((2.0 * p - ui[None, :] * di[:, None]) - uj * dj[:, None])
            tij = t[i] - t[i + 1:][ok]
            term = (tij[:, 0] * q[:, 0] + tij[:, 1] * q[:, 1]) + tij[:, 2] * q[:, 2]
            nom += np.bincount(b, weights=term, minlength=binnr)
            sum_abs += np.bincount(b, weights=np.abs(term), minlength=binnr)
            den += np.bincount(b, weights=(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2], minlength=binnr)
        cnt += np.bincount(b, minlength=binnr)
    if with_abs:
        return nom, den, cnt, sum_abs
    return nom, den, cnt


def mean_pv_from_tv(pos, vel_ang, bins, theta1=None, theta2=None):
    """(rsep, pest, nom, denom, counts)."""
    binnr = len(bins)
    binwidth = float(np.diff(bins)[0])
    u, t = angles_and_velocities(pos, vel_ang, theta1, theta2)
    nom, den, cnt = pair_sums(pos, u, t, binnr, binwidth)
    with np.errstate(invalid="ignore"):
        keep = den > 0
    rsep = np.linspace(0.0, binwidth * (binnr - 1), binnr) + binwidth / 2.0
    return rsep, nom[keep] / den[keep], nom, den, cnt


def known_answer_catalogue(spec):
    """The catalogue of tests/golden/pairwise_known_answers.json from its construction parameters."""
    c = spec["catalogue"]
    n, h = c["n"], c["n"] // 2
    pos = np.zeros((n, 3))
    pos[:, 0] = np.linspace(*c["x_linspace"], n)
    pos[:h, 1] = c["y_first_half"]
    pos[h:, 1] = np.linspace(*c["y_second_half_linspace"], n - h)
    pos[:, 2] = c["z"]
    vel = np.zeros((n, 2))
    vel[:h, 1] = c["v_dec_first_half"]
    vel[h:, 1] = c["v_dec_second_half"]
    return pos, vel, np.linspace(*c["bins_linspace"])


def light_cone(n, seed, zmin=500.0, zmax=3000.0, half_angle_deg=5.0, clusters=0, sigma=3.0, vsig=300.0):
    """Light-cone-shaped catalogue: z uniform in [zmin, zmax], x / y within +-half_angle of the z axis; with
    `clusters`, objects are scattered (sigma Mpc/h) around that many centres drawn the same way."""
    rng = np.random.default_rng(seed)
    tan = np.tan(np.deg2rad(half_angle_deg))

    def draw(m):
        z = rng.uniform(zmin, zmax, m)
        return np.stack([z * rng.uniform(-tan, tan, m), z * rng.uniform(-tan, tan, m), z], axis=1)

    pos = draw(n) if not clusters else draw(clusters)[rng.integers(0, clusters, n)] + rng.normal(0.0, sigma, (n, 3))
    return pos, rng.normal(0.0, vsig, (n, 2))
