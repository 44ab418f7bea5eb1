"""numpy restatement of the pairwise-velocity histograms (mean_pv_z_sign / mean_pv_radial of the reference's
particles/utils_cython/pairwise_velocity.pyx), fp64 and op by op, vectorised per row i over j > i.

For the pair i < j of original indices, with the differences taken j - i:  d = ((dx^2 + dy^2) + dz^2)^(1/2); the pair is
seen when d <= float64(float32(r)) and ffirst <= i < ssecond.  v12 = (vz_j - vz_i) sign(z_j - z_i) (z_sign) or
((dvx dx + dvy dy) + dvz dz) / d (radial).  ds = float32(d / dist_width), vs = float32(v12 / vel_width + vel_bin // 2):
the pair counts in hist[int(ds), int(vs)] when int(ds) < dist_bin and 0 <= vs < vel_bin, else in `outside`.  Moments per
row a = int(ds) < dist_bin over the seen pairs with finite v12, whatever vs is: count, sum v12, sum v12^2 - and, for
the error bound of a reordered sum, sum |v12| (sum v12^2 is its own)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pairwise_pdf_known_answers.json")


def pair_pdf(pos, vel, r, dist_bin, vel_bin, kind, dist_width=1.0, vel_width=1.0, ffirst=0, ssecond=None):
    """dict(hist (dist_bin, vel_bin) int64, outside int, count int64, s1, s2, sum_abs float64 (dist_bin,))."""
    pos = np.asarray(pos, dtype=np.float64)
    vel = np.asarray(vel, dtype=np.float64)
    n = len(pos)
    ssecond = n if ssecond is None else ssecond
    reach = np.float64(np.float32(r))
    offset = vel_bin // 2
    hist = np.zeros(dist_bin * vel_bin, dtype=np.int64)
    count = np.zeros(dist_bin, dtype=np.int64)
    s1, s2, sum_abs = np.zeros(dist_bin), np.zeros(dist_bin), np.zeros(dist_bin)
    outside = 0
    for i in range(ffirst, min(ssecond, n - 1)):
        dr = pos[i + 1:] - pos[i]
        d = np.sqrt((dr[:, 0] * dr[:, 0] + dr[:, 1] * dr[:, 1]) + dr[:, 2] * dr[:, 2])
        seen = d <= reach
        if not seen.any():
            continue
        dr, d = dr[seen], d[seen]
        dv = vel[i + 1:][seen] - vel[i]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if kind == "z_sign":
                v12 = dv[:, 2] * np.sign(dr[:, 2])
            elif kind == "radial":
                v12 = ((dv[:, 0] * dr[:, 0] + dv[:, 1] * dr[:, 1]) + dv[:, 2] * dr[:, 2]) / d
            else:
                raise ValueError(kind)
            ds = (d / dist_width).astype(np.float32)
            vs = (v12 / vel_width + offset).astype(np.float32)
            in_rows = ds < np.float32(dist_bin)
            counted = in_rows & (vs >= 0) & (vs < np.float32(vel_bin))
        a = np.where(in_rows, ds, 0).astype(np.int64)
        b = np.where(counted, vs, 0).astype(np.int64)
        hist += np.bincount(a[counted] * vel_bin + b[counted], minlength=dist_bin * vel_bin)
        outside += int(len(d) - counted.sum())
        m = in_rows & np.isfinite(v12)
        count += np.bincount(a[m], minlength=dist_bin)
        s1 += np.bincount(a[m], weights=v12[m], minlength=dist_bin)
        s2 += np.bincount(a[m], weights=v12[m] * v12[m], minlength=dist_bin)
        sum_abs += np.bincount(a[m], weights=np.abs(v12[m]), minlength=dist_bin)
    return dict(hist=hist.reshape(dist_bin, vel_bin), outside=outside, count=count, s1=s1, s2=s2, sum_abs=sum_abs)


def mean_and_sigma(count, s1, s2):
    """(mean, sigma) per row as the product's host side forms them; NaN for empty rows."""
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = s1 / count
        return mean, np.sqrt(s2 / count - mean * mean)


def load_golden():
    """(catalogue table, edge-case table) of tests/golden/pairwise_pdf_known_answers.json with the float.hex strings
    turned into float64 arrays."""
    with open(GOLDEN) as f:
        g = json.load(f)

    def arr(rows):
        return np.array([[float.fromhex(x) for x in row] for row in rows], dtype=np.float64).reshape(-1, 3)

    cat = dict(g["catalogue"])
    cat["pos"], cat["vel"] = arr(cat["pos"]), arr(cat["vel"])
    edges = []
    for e in g["edge_cases"]:
        e = dict(e)
        e["pos"], e["vel"] = arr(e["pos"]), arr(e["vel"])
        edges.append(e)
    return cat, edges


def dense(entries, dist_bin, vel_bin):
    """(dist_bin, vel_bin) int64 histogram from the golden file's non-zero (a, b, count) entries."""
    h = np.zeros((dist_bin, vel_bin), dtype=np.int64)
    for a, b, c in entries:
        h[a, b] = c
    return h


def coherent_velocities(pos, seed, sigma=6.0, infall=0.05):
    """(N, 3) velocities: normal scatter plus a coherent infall towards the catalogue's centre, so that the per-row sums
    of v12 are not pure cancellation."""
    rng = np.random.default_rng(seed)
    return -infall * (pos - pos.mean(axis=0)) + rng.normal(0.0, sigma, pos.shape)


def compact(n=3000, seed=11):
    """n objects in a 40-wide cube far from the origin (one cell at r = 30)."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-20.0, 20.0, (n, 3)) + np.array([30.0, -10.0, 1200.0])


def lattice(side=12):
    """side^3 integer lattice points, offset (-6, 4, 1000), with integer velocities."""
    g = np.arange(float(side))
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + np.array([-6.0, 4.0, 1000.0])
    vel = np.random.default_rng(4).integers(-12, 13, pos.shape).astype(np.float64)
    return pos, vel
