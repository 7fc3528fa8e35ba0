"""What the guided denoiser must return: the contract of include/rt_hip.h ("THE FILTER") restated in numpy float32, one rounded
operation per numpy call, the 25 taps in the contract's order as shifted arrays with validity masks.  TEST INFRASTRUCTURE ONLY;
written from the contract's text, not from the kernel's.
"""
import math

import numpy as np

F = np.float32
H = (F(0.375), F(0.25), F(0.0625))
TILE = (32, 8)                    # of a phase sub-lattice, x and y: what ONE workgroup of rt_guided.hip filters (used by lost_halo only)


def _shifted(a, ox, oy):
    """(a[y + oy, x + ox] where that is inside the image, else 0; the inside mask (h, w)) -- None when no pixel has the tap."""
    h, w = a.shape[:2]
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    q = np.zeros_like(a)
    q[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return q


def luminance(c):
    return c[..., 0] * F(0.2126) + c[..., 1] * F(0.7152) + c[..., 2] * F(0.0722)


def _other_tile(h, w, s, d, axis):
    """(h, w) bool: the tap s * d away along `axis` (0: x, 1: y) lies in another TILE of the pixel's sub-lattice than the pixel."""
    u = np.arange(w if axis == 0 else h) // s
    other = u // TILE[axis] != (u + d) // TILE[axis]
    return np.broadcast_to(other[None, :] if axis == 0 else other[:, None], (h, w))


def guided(color, coverage, albedo, normal, position, iterations=4, sigma_color=1.0, sigma_normal=0.2, sigma_position=1.0,
           demodulate=True, lost_halo=None):
    """out f32 (h, w, 3).

    lost_halo, for tests of the TESTS only (it is not the contract): a dict with "step" and "axis" (0: x, 1: y).  At that step every
    tap whose pixel lies in another 32 x 8 sub-lattice tile than the centre along that axis is skipped, as if a workgroup's halo had
    never arrived; "pairs" receives the number of skipped (pixel, tap) pairs whose centre has coverage != 0 and whose weight is
    > 0.  Inputs are worth running on the GPU at a size and step only if this changes their output (tests/test_guided_cpu.py)."""
    color, cov, normal, P = [np.ascontiguousarray(a, F) for a in (color, coverage, normal, position)]
    h, w = cov.shape
    with np.errstate(all="ignore"):
        k_c, k_n, k_p = [F(1.0) / (F(s) * F(s)) for s in (sigma_color, sigma_normal, sigma_position)]
        N = normal * F(2.0) - cov[..., None]
        m = np.ascontiguousarray(albedo, F) + ((F(1.0) - cov) + F(1e-3))[..., None] if demodulate else np.ones_like(color)
        c = color / m
        inside = np.ones((h, w), bool)
        for i in range(iterations):
            s = 1 << i
            kc = k_c * F(1 << (2 * i))
            L = luminance(c)
            sum_c, sum_w = np.zeros((h, w, 3), F), np.zeros((h, w), F)
            for t in range(25):
                dy, dx = t // 5 - 2, t % 5 - 2
                valid = _shifted(inside, s * dx, s * dy)
                if valid is None:
                    continue
                Nq, covq, Pq, Lq, cq = [_shifted(a, s * dx, s * dy) for a in (N, cov, P, L, c)]
                dn = N - Nq
                dn2 = dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1] + dn[..., 2] * dn[..., 2]
                dcov = cov - covq
                e = Pq - P
                pl = N[..., 0] * e[..., 0] + N[..., 1] * e[..., 1] + N[..., 2] * e[..., 2]
                dl = L - Lq
                D = dn2 * k_n + dcov * dcov * k_n + pl * pl * k_p + dl * dl * kc
                r = F(1.0) / (F(1.0) + D)
                wgt = ((H[abs(dy)] * H[abs(dx)]) * r) * r
                if lost_halo is not None and lost_halo["step"] == s:
                    lost = valid & _other_tile(h, w, s, (dx, dy)[lost_halo["axis"]], lost_halo["axis"])
                    lost_halo["pairs"] = lost_halo.get("pairs", 0) + int((lost & (cov != 0) & (wgt > 0)).sum())
                    valid = valid & ~lost
                sum_c = np.where(valid[..., None], sum_c + wgt[..., None] * cq, sum_c)
                sum_w = np.where(valid, sum_w + wgt, sum_w)
            c = np.where((cov == 0)[..., None], c, sum_c / sum_w[..., None])
        out = np.where((cov == 0)[..., None], color, c * m)
    assert out.dtype == F
    return out


def encode_u8(x):
    """rt_encode_u8 per element (rt_math.h): the clamp that NaN fails (x > 0 ? x : 0, then the upper bound: NaN encodes to 0),
    the oracle's rt_linear_to_srgb, x 255.999, truncate."""
    from tests import _oracle
    x = np.ascontiguousarray(x, F)
    with np.errstate(invalid="ignore"):
        c = np.where(x > 0, x, F(0.0)).astype(F)
    c = np.where(c > 1, F(1.0), c).astype(F)
    return (_oracle.math(8, c) * F(255.999)).astype(np.uint8)


def sigma_position(position, coverage):
    """The default: 0.02 x the diagonal of the bounding box of position over coverage == 1, 1.0 when there is no such pixel."""
    full = np.asarray(coverage) == 1.0
    if not full.any():
        return 1.0
    pts = np.asarray(position, np.float64)[full]
    d = pts.max(axis=0) - pts.min(axis=0)
    diag = math.sqrt(float(d[0]) * float(d[0]) + float(d[1]) * float(d[1]) + float(d[2]) * float(d[2]))
    return 0.02 * diag if diag > 0.0 else 1.0
