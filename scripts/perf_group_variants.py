"""Site times of the tiled paint at the benchmark's configuration (1024^3 lattice, natural order, CIC, fp32, hint "ordered"),
best and mean of `reps` paints, for ONE build of the library: run once per build, one process each
(scripts/build_variants.sh <tag> -DWST_CAP_N=160 ...; ASTRILD_HIP_LIB=astrild_amd/libastrild_hip_<tag>.so).  Prints one JSON
line: the sites, the list statistics, and sum and sum of squares of the painted grid in float64 (equal between builds).
usage: python scripts/perf_group_variants.py <tag> [reps=9]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from astrild_amd import device as dev

tag = sys.argv[1] if len(sys.argv) > 1 else "default"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
n, L = 1024, 1000.0
pos = dev.synth_lattice_particles(n, n, L, shuffle=False, dtype=torch.float32)
grid = torch.empty((n, n, n), dtype=torch.float32, device="cuda")
st = {}
kw = dict(out=grid, method="tiled", accumulate=False, defer_fold=True, offset=1.0, hint="ordered")
dev.paint(pos, None, n, L, "cic", stats=st, **kw)
dev.paint(pos, None, n, L, "cic", check_dropped=False, **kw)
torch.cuda.synchronize()
rows = []
for _ in range(reps):
    dev.profile_enable(True)
    dev.paint(pos, None, n, L, "cic", check_dropped=False, **kw)
    torch.cuda.synchronize()
    rows.append({k: v[1] for k, v in dev.profile_report().items()})
    dev.profile_enable(False)
sites = sorted(rows[0])
best = {k: round(min(r[k] for r in rows), 4) for k in sites}
mean = {k: round(sum(r[k] for r in rows) / reps, 4) for k in sites}
full = dev.paint(pos, None, n, L, "cic", method="tiled", accumulate=False, hint="ordered", check_dropped=False)     # folded: complete
check = (float(full.double().sum()), float((full.double() ** 2).sum()))
print(json.dumps(dict(tag=tag, best=best, mean=mean, lists=st, check=check)), flush=True)
