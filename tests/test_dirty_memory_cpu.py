"""CPU: the byte-pattern logic of the dirty allocator (tests/dirty_memory.py) on host tensors - what the GPU tests of
tests/test_gpu_dirty_memory.py rely on, checked where there is no GPU."""
import math

import numpy as np
import pytest

from tests import dirty_memory as dm

torch = pytest.importorskip("torch")

DTYPES = [torch.float32, torch.float64, torch.complex64, torch.complex128, torch.int32, torch.int64, torch.uint8]


@pytest.mark.parametrize("pattern", list(dm.PATTERNS) + [dm.ZERO_BYTES], ids=lambda p: dm.PATTERN_IDS[p])
def test_every_byte_of_every_dtype_holds_the_pattern(pattern):
    with dm.dirty(pattern, device_types=("cpu",)) as alloc:
        for dtype in DTYPES:
            made = [torch.empty((3, 5), dtype=dtype), torch.empty_like(torch.ones(7, dtype=dtype)),
                    torch.ones(2, dtype=dtype).new_empty((4, 3))]
            for t in made:
                assert t.dtype == dtype and dm.all_bytes_are(t, pattern)
                assert np.all(t.numpy().view(np.uint8) == pattern)
        assert alloc.allocations == 3 * len(DTYPES)
        assert alloc.bytes == sum(3 * 5 * s + 7 * s + 12 * s for s in (4, 8, 8, 16, 4, 8, 1))
        assert alloc.log[0] == (torch.float32, (3, 5))


def test_the_patterns_mean_what_the_cases_assume():
    with dm.dirty(dm.NAN_BYTES, device_types=("cpu",)):
        assert torch.isnan(torch.empty(4, dtype=torch.float32)).all() and torch.isnan(torch.empty(4, dtype=torch.float64)).all()
        assert torch.isnan(torch.view_as_real(torch.empty(4, dtype=torch.complex128))).all()
        assert (torch.empty(4, dtype=torch.int64) == -1).all() and (torch.empty(4, dtype=torch.int32) == -1).all()
    with dm.dirty(dm.HUGE_BYTES, device_types=("cpu",)):
        f32, f64 = torch.empty(4, dtype=torch.float32), torch.empty(4, dtype=torch.float64)
        assert math.isfinite(f32[0].item()) and f32[0].item() > 3.3e38
        assert math.isfinite(f64[0].item()) and f64[0].item() > 1.3e306
        assert (torch.empty(4, dtype=torch.int64) == 0x7F7F7F7F7F7F7F7F).all()


def test_what_passes_through_untouched_and_the_restore():
    real = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with dm.dirty(dm.NAN_BYTES, device_types=("cpu",)) as alloc:
        assert torch.empty is not real[0]
        assert torch.empty(0).numel() == 0                                   # empty: nothing to poison
        assert torch.empty(5, device="meta").device.type == "meta"
        assert (torch.zeros(6) == 0).all() and (torch.zeros_like(torch.ones(3)) == 0).all()
        assert alloc.allocations == 0
        torch.empty(2)
        with alloc.using(dm.ZERO_BYTES):
            assert (torch.empty(8, dtype=torch.float64) == 0).all()
        assert alloc.allocations == 2 and alloc.since(1) == 1
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real
    assert "new_empty" not in vars(torch.Tensor)


def test_a_cuda_allocator_leaves_host_tensors_alone():
    with dm.dirty(dm.NAN_BYTES) as alloc:
        t = torch.empty(16, dtype=torch.int64)
        t.zero_()
        assert alloc.allocations == 0 and alloc.bytes == 0


def test_the_emptied_caches_come_back():
    from astrild_amd import device as dev
    from astrild_amd import lensing
    before = (dev._power_scratch, dev._geom_cache, lensing._lens_plans, lensing._smooth_plans)
    with dm.dirty(dm.NAN_BYTES):
        now = (dev._power_scratch, dev._geom_cache, lensing._lens_plans, lensing._smooth_plans)
        assert all(a is not b and b == {} for a, b in zip(before, now))
    assert all(a is b for a, b in zip(before, (dev._power_scratch, dev._geom_cache, lensing._lens_plans,
                                               lensing._smooth_plans)))
