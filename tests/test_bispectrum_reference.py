"""CPU: the plain-torch float64 reference the GPU bispectrum-kernel tests compare with (tests/bispectrum_reference.py)
against the numpy oracle."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import bispectrum as ob
from tests import bispectrum_reference as br


@pytest.mark.parametrize("n", [16, 32])
def test_shell_fields_equal_the_oracle(n):
    """Same fields as oracle.bispectrum.shell_fields (irfftn(dk * mask) * Ng with dk = rfftn / Ng: the same normalisation
    as irfftn(norm="forward")), to 1e-12 of their maximum - the shell (0, 1), shells whose edges are exact integer norms
    (|m| = 3, 5: 3-4-5 vectors) and one that reaches past the Nyquist disc included."""
    rng = np.random.default_rng(n)
    f = rng.standard_normal((n, n, n))
    f = f + 0.3 * f * f
    edges = np.array([0, 1, 3, 5, n // 2 - 1, n // 2 + 5])
    want, _ = ob.shell_fields(f, edges)
    spec = torch.from_numpy(np.fft.rfftn(f) / f.size)
    shells = list(zip(edges[:-1].tolist(), edges[1:].tolist()))
    got = br.shell_fields(spec, shells)
    assert len(got) == len(want)
    for (lo, hi), g, w in zip(shells, got, want):
        assert g.dtype == torch.float64 and np.abs(w).max() > 0
        assert np.abs(g.numpy() - w).max() <= 1e-12 * np.abs(w).max(), (lo, hi)
    # a complex64 spectrum is widened, not transformed in single precision
    g32 = br.shell_field(spec.to(torch.complex64), 1, 3)
    w32, _ = ob.shell_fields(np.fft.irfftn(spec.to(torch.complex64).numpy().astype(np.complex128), s=f.shape, axes=(0, 1, 2)) * f.size, edges[1:3])
    assert np.abs(g32.numpy() - w32[0]).max() <= 1e-12 * np.abs(w32[0]).max()
    assert torch.equal(br.m2_half(n).long(), torch.from_numpy(ob._m2_half(n)))
    # the slab-wise inverse is irfftn: any slab width, a ragged last slab, the whole spectrum (m_hi = 0)
    want = torch.fft.irfftn(spec, s=(n, n, n), norm="forward")
    for slab in (1, 5, 32, 64):
        got = br.inverse_in_slabs(spec.clone(), slab)
        assert (got - want).abs().max() <= 1e-12 * want.abs().max(), slab
    assert (br.shell_field(spec, 0, 0) - want).abs().max() <= 1e-12 * want.abs().max()
    assert np.abs(want.numpy() - f).max() <= 1e-12 * np.abs(f).max()


def test_triangle_sums_once_per_unordered_triple():
    rng = np.random.default_rng(3)
    host = [rng.standard_normal(1000).astype(np.float32) for _ in range(4)]
    fields = [torch.from_numpy(h) for h in host]
    tri = [(0, 1, 2), (2, 0, 1), (1, 1, 3), (3, 1, 1), (1, 3, 1), (2, 2, 2), (0, 1, 2)]
    ref, scale = br.triangle_sums(fields, tri, chunk=256)                  # several chunks, a ragged last one
    h64 = [h.astype(np.float64) for h in host]
    for (a, b, c), r, s in zip(tri, ref, scale):
        p = h64[a] * h64[b] * h64[c]
        assert abs(r - p.sum()) <= 1e-13 * np.abs(p).sum() and abs(s - np.abs(p).sum()) <= 1e-13 * s
    assert ref[0] == ref[1] == ref[6] and ref[2] == ref[3] == ref[4]      # one sum per unordered triple
