"""Float64 reference of the bispectrum estimator's tail in plain torch (no custom kernel; CPU or GPU tensors):
the shell fields of a half spectrum and the triangle sums over them.

    spec        rfftn(field) / Ng, shape (n, n, n/2+1), any complex dtype (widened to complex128)
    f_s(x)      sum over m_lo^2 <= |m|^2 < m_hi^2 of spec_k e^{ikx}
                = irfftn(spec * 1[shell], norm="forward")               (exact integer |m|^2 test; formed in slabs)
    ref[t]      sum_x f_a f_b f_c        for t = (a, b, c)
    S[t]        sum_x |f_a f_b f_c|      the scale the fp32 product roundings are measured against

tests/test_bispectrum_reference.py checks the fields against oracle.bispectrum.shell_fields on the CPU."""
import numpy as np
import torch


def m2_half(n, device=None):
    """|m|^2 on the half lattice (n, n, n/2+1) as int32 (at most 3 (n/2)^2)."""
    m = torch.arange(n, dtype=torch.int32, device=device)
    m = torch.where(m > n // 2, m - n, m)
    mz = torch.arange(n // 2 + 1, dtype=torch.int32, device=device)
    return m[:, None, None] ** 2 + m[None, :, None] ** 2 + mz[None, None, :] ** 2


def inverse_in_slabs(work, slab=32):
    """irfftn(work, norm="forward") of a complex128 half spectrum, the same three passes (x and y complex, then z complex to
    real) taken ``slab`` columns / planes at a time: besides ``work`` (overwritten) and the result only slab-sized
    temporaries exist, where torch's irfftn holds two more copies of the spectrum."""
    n = work.shape[0]
    assert work.dtype == torch.complex128 and tuple(work.shape) == (n, n, n // 2 + 1)
    for z0 in range(0, n // 2 + 1, slab):
        work[:, :, z0:z0 + slab] = torch.fft.ifft2(work[:, :, z0:z0 + slab], dim=(0, 1), norm="forward")
    out = torch.empty((n, n, n), dtype=torch.float64, device=work.device)
    for x0 in range(0, n, slab):
        out[x0:x0 + slab] = torch.fft.irfft(work[x0:x0 + slab], n=n, dim=2, norm="forward")
    return out


def shell_field(spec, m_lo, m_hi, m2=None):
    """The float64 field of one shell (m_hi = 0: of the whole spectrum)."""
    n = spec.shape[0]
    assert tuple(spec.shape) == (n, n, n // 2 + 1)
    masked = spec.to(torch.complex128, copy=True)
    if m_hi:
        if m2 is None:
            m2 = m2_half(n, spec.device)
        masked.mul_((m2 >= int(m_lo) ** 2) & (m2 < int(m_hi) ** 2))
    return inverse_in_slabs(masked)


def shell_fields(spec, shells):
    m2 = m2_half(spec.shape[0], spec.device)
    return [shell_field(spec, lo, hi, m2) for lo, hi in shells]


def triangle_sums(fields, triangles, chunk=1 << 24):
    """(ref, S) as float64 numpy arrays, one entry per (a, b, c) in ``triangles`` (indices or keys into ``fields``, real
    tensors of any float dtype: the products and the sums are formed in float64).  The sums are formed once per distinct
    unordered triple and mapped back to the list; ``chunk`` cells at a time, so that no temporary is larger than that."""
    triangles = [tuple(t) for t in triangles]
    sums = {}
    for key in sorted({tuple(sorted(t)) for t in triangles}):
        a, b, c = (fields[s].reshape(-1) for s in key)
        tot = torch.zeros((), dtype=torch.float64, device=a.device)
        mag = torch.zeros((), dtype=torch.float64, device=a.device)
        for i0 in range(0, a.numel(), chunk):
            p = a[i0:i0 + chunk].double() * b[i0:i0 + chunk].double() * c[i0:i0 + chunk].double()
            tot += p.sum()
            mag += p.abs().sum()
        sums[key] = (tot, mag)
    sums = {k: (float(v[0]), float(v[1])) for k, v in sums.items()}
    ref = np.array([sums[tuple(sorted(t))][0] for t in triangles], dtype=np.float64)
    scale = np.array([sums[tuple(sorted(t))][1] for t in triangles], dtype=np.float64)
    return ref, scale
