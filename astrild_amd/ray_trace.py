"""Multi-plane ray tracing over lens planes on the GPU (``ast_lens_green_multiply`` / ``ast_ray_step`` /
``ast_ray_emit``, csrc/ray_trace.hip).  ``rays.LensPlanes.ray_trace`` is the interface in physical units;
these are the one-call-per-C-entry wrappers under it and ``trace``, which composes them.

Flat sky, flat universe, comoving distances.  A ray with direction theta has the angular position beta(chi); carried from
plane to plane are d = beta - theta, s = dx/dchi - theta (x = chi beta), A = d beta / d theta - I and
B = d (dx/dchi) / d theta - I, twelve ``(npix, npix)`` float64 planes in one tensor (``STATE``), all 0 at the observer.
Component 1 is array axis 0.  At plane k the ray is advanced, ``d <- (chi_prev d + (chi_k - chi_prev) s) / chi_k`` and
the same for A from B, and then deflected by the plane's angular potential psi_k, ``s <- s - grad psi``,
``B <- B - (grad grad psi) (I + A)``, sampled at beta (``born``: at theta, and ``B <- B - grad grad psi``).  A source at
chi_s reads the state after the last plane in front of it: ``A_s = (chi_k A + (chi_s - chi_k) B) / chi_s`` =
``[[-kappa - gamma1, -gamma2 - omega], [-gamma2 + omega, -kappa + gamma1]]`` and alpha = -d_s (the lens equation is
beta = theta - alpha).  One potential is resident at a time and every source comes out of one trace.

Everything is queued on the caller's current stream; no call waits for the device; nothing is kept between calls but the
FFT plans of ``device.fft_plan``."""
import math

import numpy as np
import torch

from . import _lib, device as dev
from ._lib import check
from .device import dense, ptr, stream

STATE = ("d1", "d2", "s1", "s2", "A11", "A12", "A21", "A22", "B11", "B12", "B21", "B22")
QUANTITIES = ("kappa", "gamma1", "gamma2", "omega", "alpha1", "alpha2")
NPIX_MAX = 4 * 65535              # the step kernel's launch grid: ceil(npix / 4) rows of workgroups, at most 65535


def _positive(value, name):
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"{name} must be a positive, finite real number, got {value!r}")
    return v


def check_pad(pad):
    """``pad`` as an int: 1 (a periodic map) or 2 (an open map in the corner of a zero grid twice its side)."""
    if isinstance(pad, bool) or not isinstance(pad, (int, np.integer)) or int(pad) not in (1, 2):
        raise ValueError(f"pad must be 1 (periodic map) or 2 (open map, zero padded), got {pad!r}")
    return int(pad)


def _square(t, name, dtypes=(torch.float64,)):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 2 and t.shape[0] == t.shape[1] and t.shape[0] >= 1):
        raise ValueError(f"{name} must be a square 2-D device tensor, got {getattr(t, 'shape', t)!r}")
    if t.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    return int(t.shape[0])


def potential_work(npix, pad):
    """``(grid, spec)``: the zeroed (m, m) float64 grid and the (m, m/2 + 1) complex128 half spectrum of
    :func:`lens_potential`, m = pad npix, for callers that solve plane after plane."""
    m = check_pad(pad) * int(npix)
    return (torch.zeros((m, m), dtype=torch.float64, device=dev.device()),
            torch.empty((m, m // 2 + 1), dtype=torch.complex128, device=dev.device()))


def lens_potential(sigma, h, pad, scale, work=None, out=None):
    """psi (m, m) float64, m = pad npix, periodic, with the 5-point Laplacian
    ``(psi[a+1,b] + psi[a-1,b] + psi[a,b+1] + psi[a,b-1] - 4 psi[a,b]) / h^2 = 2 scale (sigma - mean)`` to rounding:
    ``sigma`` (npix, npix; float32 or float64, on the device) sits in the corner [0, npix)^2 of the grid, the rest is
    zero, and the mean is taken over all m^2 nodes.  An R2C and a C2R of ``device.fft_plan`` with the discrete Green's
    function between them: mode (a, b) times ``-2 scale h^2 / m^2 / (4 (sin^2(pi a / m) + sin^2(pi b / m)))``, mode (0, 0)
    set to 0.  ``work``: what :func:`potential_work` returns (allocated here when not given); ``out``: (m, m) float64."""
    npix = _square(sigma, "sigma", (torch.float32, torch.float64))
    pad, h, scale = check_pad(pad), _positive(h, "h"), float(scale)
    if not math.isfinite(scale):
        raise ValueError(f"scale must be finite, got {scale!r}")
    m = pad * npix
    grid, spec = potential_work(npix, pad) if work is None else work
    assert grid.is_cuda and grid.is_contiguous() and grid.dtype == torch.float64 and tuple(grid.shape) == (m, m)
    assert spec.is_cuda and spec.is_contiguous() and spec.dtype == torch.complex128 and tuple(spec.shape) == (m, m // 2 + 1)
    if out is None:
        out = torch.empty((m, m), dtype=torch.float64, device=sigma.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float64 and tuple(out.shape) == (m, m)
    if pad > 1:
        grid.zero_()
    grid[:npix, :npix].copy_(sigma)
    dev.fft_plan(_lib.FFT_R2C, _lib.F64, (m, m)).execute(grid, spec)
    check(_lib.lib().ast_lens_green_multiply(ptr(spec), m, scale * (h * h) / (float(m) * float(m)), stream()),
          "ast_lens_green_multiply")
    dev.fft_plan(_lib.FFT_C2R, _lib.F64, (m, m)).execute(spec, out)
    return out


def ray_state(npix):
    """The state of npix x npix rays at the observer: ``(12, npix, npix)`` float64 zeros, planes in the order ``STATE``."""
    n = int(npix)
    if not 1 <= n <= NPIX_MAX:
        raise ValueError(f"npix must lie in 1 .. {NPIX_MAX}, got {npix!r}")
    return torch.zeros((len(STATE), n, n), dtype=torch.float64, device=dev.device())


def _check_state(state):
    if not (isinstance(state, torch.Tensor) and state.is_cuda and state.dtype == torch.float64 and state.dim() == 3
            and state.shape[0] == len(STATE) and state.shape[1] == state.shape[2] and 1 <= state.shape[1] <= NPIX_MAX):
        raise ValueError(f"state must be a (12, npix, npix) float64 device tensor (ray_state), got "
                         f"{getattr(state, 'shape', state)!r}")
    assert state.is_contiguous()
    return int(state.shape[1])


def ray_step(psi, state, h, chi_prev, chi_k, born=False):
    """One lens plane: advance ``state`` from ``chi_prev`` (0 for the first plane) to ``chi_k``, then deflect it by
    ``psi`` (m, m) float64, periodic, node (i, j) under ray (i, j), nodes ``h`` radians apart (module docstring;
    operation for operation in include/astrild_hip.h).  In place; returns ``state``."""
    m = _square(psi, "psi")
    npix = _check_state(state)
    h, chi_k = _positive(h, "h"), _positive(chi_k, "chi_k")
    chi_prev = float(chi_prev)
    if not 0.0 <= chi_prev < chi_k:
        raise ValueError(f"chi_prev must lie in [0, chi_k = {chi_k!r}), got {chi_prev!r}")
    if npix > m:
        raise ValueError(f"the rays ({npix} a side) do not fit the potential ({m} a side)")
    check(_lib.lib().ast_ray_step(ptr(dense(psi)), m, ptr(state), npix, h, chi_prev, chi_k, int(bool(born)), stream()),
          "ast_ray_step")
    return state


def ray_emit(state, chi_k, chi_s, out=None):
    """The maps of a source at ``chi_s`` from the state after the plane at ``chi_k < chi_s``: ``(6, npix, npix)`` float64
    in the order ``QUANTITIES``.  ``out``: such a tensor, or a view whose six planes are dense and equally spaced (a
    column of a ``(6, S, npix, npix)`` tensor); every element is written."""
    npix = _check_state(state)
    chi_k, chi_s = _positive(chi_k, "chi_k"), _positive(chi_s, "chi_s")
    if not chi_s > chi_k:
        raise ValueError(f"the source (chi_s = {chi_s!r}) must lie behind the plane (chi_k = {chi_k!r})")
    if out is None:
        out = torch.empty((len(QUANTITIES), npix, npix), dtype=torch.float64, device=state.device)
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (len(QUANTITIES), npix, npix)
    assert out[0].is_contiguous() and out.stride(0) >= npix * npix
    check(_lib.lib().ast_ray_emit(ptr(state), npix, chi_k, chi_s, ptr(out), int(out.stride(0)), stream()), "ast_ray_emit")
    return out


def emitting_plane(chi, chi_s):
    """Index of the last plane with ``chi[k] < chi_s`` (``chi`` ascending), -1 when there is none."""
    return int(np.searchsorted(np.asarray(chi, dtype=np.float64), float(chi_s), side="left")) - 1


def trace(planes, chi, weights, h, chi_src, born=False, pad=1):
    """Rays through ``planes`` (P, npix, npix; float32 or float64, on the device) at the ascending distances ``chi``:
    plane k has the surface density ``sigma_k = chi[k] weights[k] planes[k]`` (``weights``: P float64 on the host,
    3/2 Omega_m D_H^-2 / a_k for planes of integrated contrast) and the potential
    ``lens_potential(planes[k], h, pad, chi[k] weights[k])``.  ``chi_src``: the source distances in any order.  Returns
    ``(6, S, npix, npix)`` float64, ``QUANTITIES`` by sources in the caller's order; a source at or in front of the first
    plane gets zeros.  The sources are served in ascending distance, each after the last plane in front of it, and the
    planes behind the farthest source are never solved."""
    assert isinstance(planes, torch.Tensor) and planes.is_cuda and planes.dim() == 3 and planes.shape[1] == planes.shape[2]
    P, npix = int(planes.shape[0]), int(planes.shape[1])
    pad, h = check_pad(pad), _positive(h, "h")
    chi = np.asarray(chi, dtype=np.float64).reshape(-1)
    weights = np.asarray(weights, dtype=np.float64).reshape(-1)
    if chi.size != P or weights.size != P or not (np.isfinite(chi).all() and chi[0] > 0 and (np.diff(chi) > 0).all()):
        raise ValueError(f"chi and weights must hold one number per plane, chi positive and ascending, got {chi!r}, {weights!r}")
    src = np.asarray(chi_src, dtype=np.float64).reshape(-1)
    if not (np.isfinite(src).all() and (src >= 0).all()):
        raise ValueError(f"source distances must be finite and >= 0, got {chi_src!r}")
    out = torch.zeros((len(QUANTITIES), src.size, npix, npix), dtype=torch.float64, device=planes.device)
    last = [emitting_plane(chi, c) for c in src]
    if max(last, default=-1) < 0:
        return out
    state, work = ray_state(npix), potential_work(npix, pad)
    psi = torch.empty((pad * npix, pad * npix), dtype=torch.float64, device=planes.device)
    for k in range(max(last) + 1):
        lens_potential(planes[k], h, pad, float(chi[k] * weights[k]), work=work, out=psi)
        ray_step(psi, state, h, 0.0 if k == 0 else float(chi[k - 1]), float(chi[k]), born)
        for s in sorted((s for s in range(src.size) if last[s] == k), key=lambda s: src[s]):
            ray_emit(state, float(chi[k]), float(src[s]), out=out[:, s])
    return out


def bench_ray_trace(nplanes=64, npix=4096, nsrc=8, pad=1, born=False, opening_angle_deg=5.0, rms=1.0, seed=1):
    """Times one trace of ``nsrc`` sources through ``nplanes`` float32 planes of Gaussian noise (standard deviation
    ``rms`` Mpc/h; distances 50 .. 3150 Mpc/h, Omega_m = 0.3, a = 1 for the weights), every plane's potential and step between
    their own pair of device events.  Returns a dict: ``potential_ms`` and ``step_ms`` per plane (medians over the planes
    behind the first, which pays for the plans), ``emit_ms`` per source, ``step_bytes`` = (2 x 96 + 8) npix^2 - the state
    read and written, psi read once - and ``step_hbm_share`` = step_bytes / step time / 8 TB/s; ``max_shift_px``: the largest |d| of the final state in pixels."""
    import statistics
    P, n, S = int(nplanes), int(npix), int(nsrc)
    gen = torch.Generator(device=dev.device()).manual_seed(int(seed))
    planes = torch.randn((P, n, n), dtype=torch.float32, device=dev.device(), generator=gen) * float(rms)
    chi = 50.0 + (np.arange(P) + 0.5) * (3100.0 / P)
    weights = np.full(P, 1.5 * 0.3 / 2997.92458 ** 2)
    src = np.linspace(chi[P // 2], chi[-1] + 100.0, S)
    h = math.radians(float(opening_angle_deg)) / n
    state, work = ray_state(n), potential_work(n, pad)
    psi = torch.empty((pad * n, pad * n), dtype=torch.float64, device=dev.device())
    out = torch.zeros((len(QUANTITIES), S, n, n), dtype=torch.float64, device=dev.device())
    last = [emitting_plane(chi, c) for c in src]
    marks, emits = [], []
    for k in range(P):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        lens_potential(planes[k], h, pad, float(chi[k] * weights[k]), work=work, out=psi)
        ev[1].record()
        ray_step(psi, state, h, 0.0 if k == 0 else float(chi[k - 1]), float(chi[k]), born)
        ev[2].record()
        marks.append(ev)
        for s in range(S):
            if last[s] == k:
                e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                e[0].record()
                ray_emit(state, float(chi[k]), float(src[s]), out=out[:, s])
                e[1].record()
                emits.append(e)
    torch.cuda.synchronize()
    pot = [ev[0].elapsed_time(ev[1]) for ev in marks[1:]] or [marks[0][0].elapsed_time(marks[0][1])]
    step = [ev[1].elapsed_time(ev[2]) for ev in marks[1:]] or [marks[0][1].elapsed_time(marks[0][2])]
    emit = [e[0].elapsed_time(e[1]) for e in emits]
    step_ms = statistics.median(step)
    step_bytes = (2 * 8 * len(STATE) + 8) * n * n
    return dict(nplanes=P, npix=n, nsrc=S, pad=pad, born=bool(born), potential_ms=statistics.median(pot),
                potential_ms_range=(min(pot), max(pot)), step_ms=step_ms, step_ms_range=(min(step), max(step)),
                emit_ms=statistics.median(emit) if emit else float("nan"), step_bytes=step_bytes,
                step_hbm_share=step_bytes / (step_ms * 1e-3) / 8e12, max_shift_px=float(state[:2].abs().max()) / h,
                finite=bool(torch.isfinite(out).all()))
