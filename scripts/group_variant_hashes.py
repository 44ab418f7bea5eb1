"""Hashes of the grids that the grouping tests' overflow-free cases paint (tests/test_gpu_paint_grouping.py,
variant_cases), with the library that is loaded: run once per build and compare the lines, e.g.
  scripts/build_variants.sh w160 -DWST_CAP_N=160
  python scripts/group_variant_hashes.py > product.json
  ASTRILD_HIP_LIB=astrild_amd/libastrild_hip_w160.so python scripts/group_variant_hashes.py > w160.json
(or ASTRILD_HIP_LIB pointing at the library built from another commit).
Each entry: [sha256 of the grid, records, strays, overflow]; with overflow 0 the grids must be bit-identical."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from astrild_amd import device
from tests import test_gpu_paint_grouping as t

torch.cuda.set_device(0)
print(json.dumps(t.variant_hashes(device), sort_keys=True))
