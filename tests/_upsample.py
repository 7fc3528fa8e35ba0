"""What feature-guided upsampling must return: the contract of include/rt_hip.h ("THE UPSAMPLING") restated in numpy float32, one
rounded operation per numpy call, the nine taps in the contract's order (j outer, i inner) as gathers with validity masks.  TEST
INFRASTRUCTURE ONLY; written from the contract's text, not from the kernel's.
"""
import numpy as np

F = np.float32
H_EVEN = (F(0.125), F(0.75), F(0.125))      # a full pixel ON a low lattice point: the quadratic B-spline at -1, 0, +1
H_ODD = (F(0.5), F(0.5), F(0.0))            # ... halfway between two: at -0.5, +0.5 (and 0 at +1.5)
TILE = (16, 8)                              # full pixels, x and y: what ONE workgroup of rt_upsample.hip writes (used by lost_halo only)
MUTATIONS = ("lost_halo", "clamp", "swap", "divide")


def _weights(n, swap):
    """(n, 3) f32: the three weights of full pixel coordinate 0 .. n - 1."""
    even, odd = (H_ODD, H_EVEN) if swap else (H_EVEN, H_ODD)
    odd_pixel = (np.arange(n) & 1).astype(bool)
    return np.where(odd_pixel[:, None], np.array(odd, F)[None, :], np.array(even, F)[None, :]).astype(F)


def upsample(color_low, low, full, sigma_normal=0.2, sigma_position=1.0, demodulate=True, mutation=None, counts=None):
    """out f32 (h, w, 3).  low, full: dicts of coverage, albedo, normal, position at (h / 2, w / 2) and (h, w).

    mutation, for tests of the TESTS only (it is not the contract), one of MUTATIONS:
      "lost_halo": a tap whose low pixel lies under another TILE than the full pixel is dropped, as if a workgroup's halo had never
                   arrived
      "clamp":     a tap outside the low image is clamped to the edge instead of skipped
      "swap":      the even and the odd weight sets are exchanged
      "divide":    c_p = sum_c / sum_w also where sum_w > 0 fails
    counts (optional dict): "fallback" receives the (h, w) bool mask of the pixels where sum_w > 0 failed."""
    assert mutation is None or mutation in MUTATIONS, mutation
    color_low = np.ascontiguousarray(color_low, F)
    cov_q, nrm_q, P_q = [np.ascontiguousarray(low[k], F) for k in ("coverage", "normal", "position")]
    cov_p, nrm_p, P_p = [np.ascontiguousarray(full[k], F) for k in ("coverage", "normal", "position")]
    h, w = cov_p.shape
    hl, wl = h // 2, w // 2
    assert w % 2 == 0 and h % 2 == 0 and w >= 2 and h >= 2 and cov_q.shape == (hl, wl) and color_low.shape == (hl, wl, 3)
    with np.errstate(all="ignore"):
        k_n, k_p = [F(1.0) / (F(s) * F(s)) for s in (sigma_normal, sigma_position)]
        N_q = nrm_q * F(2.0) - cov_q[..., None]
        N_p = nrm_p * F(2.0) - cov_p[..., None]
        if demodulate:
            m_q = np.ascontiguousarray(low["albedo"], F) + ((F(1.0) - cov_q) + F(1e-3))[..., None]
            m_p = np.ascontiguousarray(full["albedo"], F) + ((F(1.0) - cov_p) + F(1e-3))[..., None]
        else:
            m_q, m_p = np.ones((hl, wl, 3), F), np.ones((h, w, 3), F)
        c_q = color_low / m_q

        xs, ys = np.arange(w), np.arange(h)
        X0, Y0 = xs >> 1, ys >> 1
        Hx, Hy = _weights(w, mutation == "swap"), _weights(h, mutation == "swap")
        sum_c, sum_w = np.zeros((h, w, 3), F), np.zeros((h, w), F)
        for j in range(3):
            Y = Y0 - 1 + (ys & 1) + j
            for i in range(3):
                X = X0 - 1 + (xs & 1) + i
                inside = ((Y >= 0) & (Y < hl))[:, None] & ((X >= 0) & (X < wl))[None, :]
                weighted = (Hy[:, j] != 0)[:, None] & (Hx[:, i] != 0)[None, :]
                valid = weighted if mutation == "clamp" else weighted & inside
                if mutation == "lost_halo":
                    same = ((Y * 2) // TILE[1] == ys // TILE[1])[:, None] & ((X * 2) // TILE[0] == xs // TILE[0])[None, :]
                    valid = valid & same
                Yc, Xc = np.clip(Y, 0, hl - 1)[:, None], np.clip(X, 0, wl - 1)[None, :]
                Nq, covq, Pq, cq = N_q[Yc, Xc], cov_q[Yc, Xc], P_q[Yc, Xc], c_q[Yc, Xc]
                dn = N_p - Nq
                dn2 = dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1] + dn[..., 2] * dn[..., 2]
                dcov = cov_p - covq
                e = Pq - P_p
                pl = N_p[..., 0] * e[..., 0] + N_p[..., 1] * e[..., 1] + N_p[..., 2] * e[..., 2]
                D = dn2 * k_n + dcov * dcov * k_n + pl * pl * k_p
                r = F(1.0) / (F(1.0) + D)
                wgt = ((Hy[:, j][:, None] * Hx[:, i][None, :]) * r) * r
                sum_c = np.where(valid[..., None], sum_c + wgt[..., None] * cq, sum_c)
                sum_w = np.where(valid, sum_w + wgt, sum_w)
        summed = sum_w > 0
        if counts is not None:
            counts["fallback"] = ~summed
        under = c_q[Y0[:, None], X0[None, :]]
        c_p = sum_c / sum_w[..., None]
        if mutation != "divide":
            c_p = np.where(summed[..., None], c_p, under)
        out = c_p * m_p
    assert out.dtype == F and out.shape == (h, w, 3)
    return out


# ---- inputs, once per size, shared by the GPU tests and the CPU tests of those tests, read-only -----------------------------------

SINGLE_TILE_SIZES = [(2, 2), (4, 2), (6, 10), (66, 38)]          # (w, h): one low pixel; ...; wl odd, 5 x 5 tiles
MULTI_TILE_SIZES = [(130, 70), (258, 66)]                        # 9 x 9 and 17 x 9 tiles of 16 x 8, ragged against them
STRIP_SIZES = [(2, 260), (516, 2)]                               # 1 x 33 and 33 x 1 tiles
SIZES = SINGLE_TILE_SIZES + MULTI_TILE_SIZES + STRIP_SIZES
SIGMAS = (0.2, 0.5)                                              # normal, position
INF = float("inf")
SIGMA_SETS = [SIGMAS, (INF, 0.5), (0.2, INF)]
FAR = 3e19                                                       # a position at which pl * pl overflows

_cases = {}


def _surface(x, y, w, h):
    """The synthetic frame at full-pixel coordinates (x, y), arrays of one shape: a sky band on top, a near plane left of a slanted
    depth edge, a far plane right of it, an albedo checker of 3 x 3 pixels.  -> (sky, near, albedo, unit normal, position,
    irradiance), the last four (..., 3)."""
    u, v = (x - w * 0.5) * 0.02, (y - h * 0.5) * 0.02
    sky = y < int(h * 0.15)
    near = ~sky & (x < w * 0.45 + 0.3 * (y - h * 0.5))
    zero = np.zeros_like(u)
    n_near = np.array([0.0, -0.2, 1.0]) / np.sqrt(1.04)
    normal = np.where(near[..., None], n_near, np.array([0.0, 0.0, 1.0]))
    position = np.where(near[..., None], np.stack([u, v, 2.0 + 0.2 * v], -1), np.stack([u * 4.5, v * 4.5, zero + 9.0], -1))
    checker = ((x // 3 + y // 3) & 1).astype(bool)
    albedo = np.where(checker[..., None], np.array([0.8, 0.7, 0.2]), np.array([0.2, 0.3, 0.7]))
    E = np.where(near[..., None], np.stack([1.2 + 0.3 * u, 0.9 + zero, 0.6 - 0.2 * v], -1),
                 np.stack([0.25 + zero, 0.35 + 0.1 * v, 0.5 + 0.1 * u], -1))
    return sky, near, albedo, normal, position, E


def _planes(x, y, w, h, cov):
    """The four planes as a resolve writes them for coverage `cov` (0 on the sky), and the noise-free colour."""
    sky, near, albedo, normal, position, E = _surface(x, y, w, h)
    cov = np.where(sky, 0.0, cov)
    c3 = cov[..., None]
    planes = dict(coverage=cov, albedo=c3 * albedo, normal=c3 * (normal * 0.5 + 0.5), position=c3 * position)
    color = c3 * (E * albedo) + (1.0 - c3) * np.array([0.5, 0.7, 1.0])
    return {k: a.astype(F) for k, a in planes.items()}, color.astype(F), near & ~sky, sky


def case(w, h, clean=False):
    """dict(color_low, low, full: the call's inputs; truth: the noise-free full-resolution colour; near, sky: (h, w) masks of the
    full frame; aimed: (h, w) mask of the pixels whose every tap overflows, the ones aimed at the sum_w > 0 fallback).
    The low planes are the frame at the low pixels' centres -- full pixels (2 X, 2 Y) -- and the low colour carries gamma noise of 16
    samples.  Not clean (what the GPU tests run): the low normals and positions are jittered as another set of samples would
    leave them, pixels along the sky line and in a column band across the depth edge have partial coverages, and where the frame
    has 60 pixels a block of up to 5 x 3 full pixels has positions of 3e19."""
    key = (w, h, clean)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(4000 + 7 * w + h + (1 if clean else 0))
    hl, wl = h // 2, w // 2
    ys, xs = np.mgrid[0:h, 0:w]
    Ys, Xs = np.mgrid[0:hl, 0:wl]
    cov_full, cov_low = np.ones((h, w)), np.ones((hl, wl))
    if not clean:
        first = int(h * 0.15)                                    # the first surface row, and a band of columns, get partial coverages
        partial = (ys == first) | ((xs % 23 == 11) & (ys > first))
        cov_full = np.where(partial, rng.uniform(0.1, 0.9, (h, w)), 1.0)
        cov_low = np.where(partial[::2, ::2], rng.uniform(0.1, 0.9, (hl, wl)), 1.0)
    full, truth, near, sky = _planes(xs, ys, w, h, cov_full)
    low, clean_low, _, _ = _planes(Xs * 2, Ys * 2, w, h, cov_low)
    noise = np.where((low["coverage"] > 0)[..., None], rng.gamma(16.0, 1.0 / 16.0, (hl, wl, 3)), 1.0)      # (sky is not noisy)
    color_low = (clean_low * noise).astype(F)
    aimed = np.zeros((h, w), bool)
    if not clean:
        hit = low["coverage"] > 0
        low["normal"] = np.where(hit[..., None], low["normal"] + rng.normal(0.0, 0.01, (hl, wl, 3)), 0.0).astype(F)
        low["position"] = np.where(hit[..., None], low["position"] + rng.normal(0.0, 0.02, (hl, wl, 3)), 0.0).astype(F)
        if w * h >= 60:
            by, bx = slice(h // 2, min(h, h // 2 + 3)), slice(w // 2, min(w, w // 2 + 5))
            aimed[by, bx] = True
            full["coverage"][by, bx] = 1.0
            full["normal"][by, bx] = F(0.5 + 0.5 / np.sqrt(3.0))   # N = (1, 1, 1) / sqrt(3): pl = -3e19 * sqrt(3) whatever the tap
            full["position"][by, bx] = F(FAR)
            full["albedo"][by, bx] = np.array([0.5, 0.4, 0.3], F)
    res = dict(color_low=color_low, low=low, full=full, truth=truth, near=near, sky=sky, aimed=aimed)
    for a in (color_low, truth, near, sky, aimed, *low.values(), *full.values()):
        a.setflags(write=False)
    _cases[key] = res
    return res


def encode_u8(x):
    """rt_encode_u8 per element, as the other passes' restatements have it."""
    from tests import _guided
    return _guided.encode_u8(x)
