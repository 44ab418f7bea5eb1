"""Grid fields at particle positions on the GPU (``ast_readout``, csrc/mesh_readout.hip): pmesh's
``RealField.readout(pos, resampler=)``, the adjoint of the ``ParticleMesh.paint`` that ``device.paint`` replaces.  What a
grid holds - the painted density, a DTFE velocity grid of ``MapTransform``, the divergence of ``device.divergence`` -
becomes a value per halo, void or group centre without leaving the device.

* **Field**: the whole periodic grid, ``(n, n, n)`` or ``(n, n, n, C)`` with C = 1 .. 4 components interleaved on the
  last axis, float32 or float64; grid point i sits at ``x = i L / n`` (pmesh's convention, as in the paint).
* **Positions**: ``(N, 3)`` in box units, float32 or float64 independently of the field; any real value wraps.
* **Result**: ``(N,)`` for a 3-D field, ``(N, C)`` for a 4-D one, in the field's dtype.
* **Arithmetic** (tests/readout_oracle.py restates it and the GPU tests ask for the same bits): per axis
  ``s = fma(x, n / L, shift)`` in float64; base cell ``floor(s)`` (CIC) or ``floor(s + 1/2)`` (NGP, TSC) and the offset
  ``s - floor(..)``; the window's weights evaluated in the field's dtype, not renormalised; then in float64, in the
  order x, y, z of the stencil, ``acc += ((wx wy) wz) f`` from 0.0 and one cast to the field's dtype.  Repeated calls
  give the same bits.
* A NaN or infinite coordinate gives NaN for that particle (all components) and reads nothing outside the field.
"""
import numpy as np
import torch

from ... import _lib, device as dev
from ...device import as_device, check, dense, ptr, real_code, stream, to_numpy

_FLOATS = ("float32", "float64")


def _dtype_name(dt):
    """'float32' for np.float32, torch.float32, 'float32', dtype('<f4'); the repr of anything numpy cannot name."""
    if isinstance(dt, torch.dtype):
        return str(dt).replace("torch.", "")
    try:
        return np.dtype(dt).name
    except TypeError:
        return repr(dt)


def check_readout_args(field_shape, field_dtype, pos_shape, pos_dtype, boxsize, resampler="cic", shift=0.0):
    """The argument checks of ``readout``, on the host and before any GPU work: ``(n, ncomp, window code, boxsize, shift)``
    or ValueError / TypeError naming the offending value: a field that is not (n, n, n) or (n, n, n, C) with C in 1 .. 4;
    ``pos`` that is not (N, 3); a dtype that is not float32 or float64 (TypeError); a ``resampler`` that is no key of
    ``_lib.WIN`` (any letter case); a ``boxsize`` that is not positive and finite; a ``shift`` that is not finite."""
    fs = tuple(int(s) for s in field_shape)
    if len(fs) not in (3, 4) or len(set(fs[:3])) != 1 or fs[0] < 1:
        raise ValueError(f"field must be (n, n, n) or (n, n, n, C) with n >= 1, got shape {fs}")
    if len(fs) == 4 and not 1 <= fs[3] <= 4:
        raise ValueError(f"field must have 1 to 4 components on its last axis, got {fs[3]} (shape {fs})")
    ps = tuple(int(s) for s in pos_shape)
    if len(ps) != 2 or ps[1] != 3:
        raise ValueError(f"pos must be (N, 3), got shape {ps}")
    for name, dt in (("field", field_dtype), ("pos", pos_dtype)):
        if _dtype_name(dt) not in _FLOATS:
            raise TypeError(f"{name} must be float32 or float64, got {_dtype_name(dt)}")
    if not isinstance(resampler, str) or resampler.lower() not in _lib.WIN:
        raise ValueError(f"resampler must be one of {sorted(_lib.WIN)}, got {resampler!r}")
    try:
        box = float("nan") if isinstance(boxsize, (str, bytes, bool)) or boxsize is None else float(boxsize)
    except (TypeError, ValueError):
        box = float("nan")
    if not (np.isfinite(box) and box > 0):
        raise ValueError(f"boxsize must be a positive, finite real number, got {boxsize!r}")
    try:
        sh = float(shift)
    except (TypeError, ValueError):
        sh = float("nan")
    if not np.isfinite(sh):
        raise ValueError(f"shift must be a finite real number (grid units), got {shift!r}")
    return fs[0], (fs[3] if len(fs) == 4 else 1), _lib.WIN[resampler.lower()], box, sh


def readout(field, pos, boxsize, resampler="cic", shift=0.0, out=None):
    """``field`` at ``pos`` (module docstring): device tensors in, a device tensor out, on the caller's current stream and
    without a host synchronisation; numpy arrays in, a numpy array out.  ``shift`` is added to every coordinate in grid
    units, as in ``device.paint``.  Strided, offset and transposed inputs give the same result as contiguous ones
    (``device.dense``).  ``out``: a contiguous device tensor of the result's shape and dtype, written in place.
    N = 0 returns an empty result without a library call."""
    on_host = not isinstance(field, torch.Tensor) and not isinstance(pos, torch.Tensor)
    if not isinstance(field, torch.Tensor):
        field = np.asarray(field)
    if not isinstance(pos, torch.Tensor):
        pos = np.asarray(pos)
    n, ncomp, win, box, sh = check_readout_args(field.shape, field.dtype, pos.shape, pos.dtype, boxsize, resampler, shift)
    f, p = dense(as_device(field)), dense(as_device(pos))
    npart = int(p.shape[0])
    shape = (npart,) if f.dim() == 3 else (npart, ncomp)
    if out is None:
        out = torch.empty(shape, dtype=f.dtype, device=f.device)
    assert out.is_cuda and out.is_contiguous() and tuple(out.shape) == shape and out.dtype == f.dtype
    if npart:
        check(_lib.lib().ast_readout(win, real_code(f), real_code(p), ptr(f), n, ncomp, ptr(p), npart, box, sh, ptr(out),
                                     stream()), "ast_readout")
    return to_numpy(out) if on_host else out


def density_at(tracers, query, nmesh, boxsize, resampler="cic", mass=None, contrast=True):
    """The density of ``tracers`` (N, 3), painted with ``device.paint(tracers, mass, nmesh, boxsize, resampler)``, read
    out at ``query`` (M, 3) with the same window: (M,) in the tracers' dtype, a device tensor (numpy when tracers and
    query are numpy arrays).  ``contrast``: ``value / mean - 1`` with ``mean = device.total_mass(mass, N) / nmesh^3``,
    applied to the M values that were read out and not to the grid; without it, the painted mass per cell."""
    on_host = not isinstance(tracers, torch.Tensor) and not isinstance(query, torch.Tensor)
    t = dense(as_device(tracers))
    m = None if mass is None else dense(as_device(mass, dtype=t.dtype))
    grid = dev.paint(t, m, int(nmesh), boxsize, resampler)
    value = readout(grid, as_device(query), boxsize, resampler)
    if contrast:
        mean = dev.total_mass(m, int(t.shape[0])) / float(int(nmesh)) ** 3
        value = value / mean - 1.0
    return to_numpy(value) if on_host else value
