"""Python view of the light probes (include/rt_hip.h, "light probes"): path-traced samples of the incoming radiance at points in
space and their nine spherical-harmonic coefficients.

bake_probes takes numpy positions and a HostScene (rt_scene_probes); bake_probes_device takes a torch tensor on the GPU, an uploaded
device scene and a stream (rt_probe_trace / rt_probe_project / rt_probe_resolve).  Plumbing only: every sample, sum and coefficient
is computed by the library.  What a host does WITH coefficients -- evaluating them, the cosine convolution -- is restated here in
float64 (sh9_basis, sh9_radiance, sh9_irradiance) for tools and tests; it is not part of the traced result.
"""
import ctypes as C

import numpy as np

from . import ctypes_abi as abi
from .native import lib as _lib, last_error
from .render import Counters
from .scene import HostScene


def get_probe_counters(lib=None) -> Counters:
    """Counters of the last probe call of this process (rt_get_probe_counters)."""
    lib = lib or _lib
    c = abi.RT_Counters()
    if lib.rt_get_probe_counters(C.byref(c)) != 0:
        raise RuntimeError(last_error(lib))
    return Counters(*[int(getattr(c, f[0])) for f in c._fields_])


def _params(lib, samples, max_bounces, seed, probe_first, sample_range):
    first, count = sample_range if sample_range is not None else (0, 0)
    return abi.RT_Probe_Params(samples=samples, sample_first=first, sample_count=count, max_bounces=max_bounces,
                               seed=lib.rt_get_seed() if seed is None else seed, probe_first=probe_first)


def _range_count(p):
    return p.sample_count if p.sample_count else p.samples - p.sample_first


def bake_probes(hs: HostScene, positions, samples, max_bounces, *, seed=None, probe_first=0, sample_range=None, return_sums=False,
                return_samples=False, lib=None):
    """The SH coefficients (n, 9, 3) float32 of the probes at `positions` (n, 3): `samples` uniform directions per probe, cast_ray
    with max_bounces along each.  seed: default rt_get_seed(); probe_first: the global index of positions[0], so that a slice of a
    probe array equals the matching rows of the whole; sample_range = (first, count): trace only those samples of every probe (the
    coefficients are then that range's share of the mean over all `samples`).  return_sums: also the (n, 9, 3) uint64 32.32 sums;
    return_samples: also the records, (n, count) of abi.PROBE_SAMPLE_DTYPE.  Returns coeffs, or a tuple in that order."""
    lib = lib or _lib
    positions = np.ascontiguousarray(positions, np.float32)
    if positions.ndim != 2 or positions.shape[1] != 3:
        raise ValueError("positions must have shape (n, 3)")
    n = len(positions)
    p = _params(lib, samples, max_bounces, seed, probe_first, sample_range)
    coeffs = np.zeros((n, abi.RT_PROBE_COEFFS, 3), np.float32)
    sums = np.zeros((n, abi.RT_PROBE_COEFFS, 3), np.uint64) if return_sums else None
    records = np.zeros((n, max(_range_count(p), 0)), abi.PROBE_SAMPLE_DTYPE) if return_samples else None
    if lib.rt_scene_probes(C.byref(hs.scene), C.byref(p), n, positions.ctypes.data, coeffs.ctypes.data,
                           sums.ctypes.data if return_sums else None, records.ctypes.data if return_samples else None) != 0:
        raise RuntimeError("rt_scene_probes failed: " + last_error(lib))
    out = (coeffs,) + ((sums,) if return_sums else ()) + ((records,) if return_samples else ())
    return out[0] if len(out) == 1 else out


def bake_probes_device(dscene, positions, samples, max_bounces, *, seed=None, probe_first=0, sample_range=None, sums=None,
                       return_sums=False, return_samples=False, stream=None, lib=None):
    """bake_probes on torch tensors: positions a contiguous float32 GPU tensor (n, 3), `dscene` what rt_scene_upload returned.
    Enqueues trace, projection and resolve on `stream` (default: torch's current stream) and returns coeffs, a float32 tensor
    (n, 9, 3), plus -- return_sums -- the int64 tensor (n, 9, 3) holding the u64 sums and -- return_samples -- a float32 tensor
    (n, count, 8) holding the records.  sums: an int64 tensor (n, 9, 3) to ADD this range to (default: a zeroed one)."""
    import torch
    lib = lib or _lib
    if positions.dtype != torch.float32 or positions.dim() != 2 or positions.shape[1] != 3 or not positions.is_cuda \
            or not positions.is_contiguous():
        raise ValueError("positions must be a contiguous float32 GPU tensor of shape (n, 3)")
    n = positions.shape[0]
    p = _params(lib, samples, max_bounces, seed, probe_first, sample_range)
    sp = (stream if stream is not None else torch.cuda.current_stream(positions.device)).cuda_stream
    if sums is None:
        sums = torch.zeros((n, abi.RT_PROBE_COEFFS, 3), dtype=torch.int64, device=positions.device)
    elif sums.dtype != torch.int64 or tuple(sums.shape) != (n, abi.RT_PROBE_COEFFS, 3) or not sums.is_cuda or not sums.is_contiguous():
        raise ValueError("sums must be a contiguous int64 GPU tensor of shape (n, 9, 3)")
    records = torch.empty((n, max(_range_count(p), 0), 8), dtype=torch.float32, device=positions.device)
    coeffs = torch.empty((n, abi.RT_PROBE_COEFFS, 3), dtype=torch.float32, device=positions.device)
    if lib.rt_probe_trace(dscene, C.byref(p), n, positions.data_ptr(), records.data_ptr(), sp) != 0:
        raise RuntimeError("rt_probe_trace failed: " + last_error(lib))
    if lib.rt_probe_project(C.byref(p), n, records.data_ptr(), sums.data_ptr(), sp) != 0:
        raise RuntimeError("rt_probe_project failed: " + last_error(lib))
    if lib.rt_probe_resolve(C.byref(p), n, sums.data_ptr(), coeffs.data_ptr(), sp) != 0:
        raise RuntimeError("rt_probe_resolve failed: " + last_error(lib))
    out = (coeffs,) + ((sums,) if return_sums else ()) + ((records,) if return_samples else ())
    return out[0] if len(out) == 1 else out


def probe_grid(lo, hi, shape):
    """(nx * ny * nz, 3) float32 positions of a regular grid over the box [lo, hi], x fastest, the end points included (an axis
    with one point sits at lo)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    nx, ny, nz = (int(v) for v in shape)
    if min(nx, ny, nz) < 1:
        raise ValueError("shape must be three positive counts")
    axes = [np.linspace(lo[a], hi[a], k) if k > 1 else np.array([lo[a]]) for a, k in enumerate((nx, ny, nz))]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.float32)


_Y = (0.282095, 0.488603, 1.092548, 0.315392, 0.546274)          # the literals of rt_sh9_basis (include/rt_math.h)


def sh9_basis(d):
    """The nine basis values at the directions d (..., 3), float64 (..., 9), in rt_sh9_basis's order."""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full_like(x, _Y[0]), _Y[1] * y, _Y[1] * z, _Y[1] * x, _Y[2] * x * y, _Y[2] * y * z,
                     _Y[3] * (3.0 * z * z - 1.0), _Y[2] * x * z, _Y[4] * (x * x - y * y)], -1)


def sh9_radiance(coeffs, d):
    """sum_k coeffs[..., k, :] Y_k(d): the radiance the coefficients (..., 9, 3) stand for along the unit direction d (3,)."""
    return np.einsum("...kc,k->...c", np.asarray(coeffs, np.float64), sh9_basis(d))


_BAND = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)      # Ramamoorthi-Hanrahan: the clamped cosine per band


def sh9_irradiance(coeffs, normal):
    """The irradiance on a surface with the unit normal (3,): the cosine convolution of the coefficients (..., 9, 3), band factors
    pi, 2 pi / 3, pi / 4 (Ramamoorthi and Hanrahan 2001)."""
    return np.einsum("...kc,k->...c", np.asarray(coeffs, np.float64), sh9_basis(normal) * _BAND)


def probe_visibility(samples):
    """Per probe of the records (n, count): the fraction of samples whose first segment hit something (finite t) and the mean t
    of those (nan where there is none) -- two float64 arrays (n,)."""
    t = np.asarray(samples["t"], np.float64)
    hit = np.isfinite(t)
    k = hit.sum(axis=1)
    frac = k / max(t.shape[1], 1)
    total = np.where(hit, t, 0.0).sum(axis=1)
    mean = np.divide(total, k, out=np.full(len(t), np.nan), where=k > 0)
    return frac, mean
