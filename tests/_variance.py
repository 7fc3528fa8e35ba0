"""What variance-guided denoising must return: the three contracts of include/rt_hip.h ("THE MOMENTS", "THE VARIANCE", "THE
VARIANCE-GUIDED FILTER") restated in numpy float32, one rounded operation per numpy call, taps in the contracts' order as gathers or
shifted arrays with validity masks, no loop over pixels.  TEST INFRASTRUCTURE ONLY; written from the contracts' text, not from the
kernels'.

Cameras and histories are tests/_temporal.py's; moments are float32 (h, w, 2): (m1, m2).
"""
import numpy as np

from tests._guided import H, _other_tile, _shifted, luminance
from tests._temporal import project

F = np.float32
G = (F(0.5), F(0.25))
CLASSES = ("sky", "fresh", "blended", "clamped", "short", "long")


def temporal_variance(moments):
    """var_t of a moments record: v = m2 - m1 * m1, clamped at 0; and where v <= 0 before the clamp."""
    v = moments[..., 1] - moments[..., 0] * moments[..., 0]
    return np.where(v > F(0.0), v, F(0.0)).astype(F), ~(v > F(0.0))


def accumulate_moments(color, coverage, albedo, normal, position, cam, prev_cam=None, history=None, moments=None, alpha=0.05,
                       max_history=64, normal_tolerance=0.3, plane_tolerance=0.02, demodulate=True):
    """THE ACCUMULATION with THE MOMENTS: dict(out, length, history, moments (h, w, 2), var_t (h, w), classes: a dict of (h, w) bool
    per name of CLASSES -- sky; fresh (m' = L, S) or blended; clamped (v <= 0 before the clamp); short (len' < 4) or long)."""
    assert (history is None) == (moments is None)
    color, cov, normal, P = [np.ascontiguousarray(a, F) for a in (color, coverage, normal, position)]
    h, w = cov.shape
    alpha, cap = F(alpha), F(max_history)
    with np.errstate(all="ignore"):
        tn2, tp2 = F(normal_tolerance) * F(normal_tolerance), F(plane_tolerance) * F(plane_tolerance)
        sky = cov == 0
        N = normal * F(2.0) - cov[..., None]
        if demodulate:
            m = np.ascontiguousarray(albedo, F) + ((F(1.0) - cov) + F(1e-3))[..., None]
            c = color / m
        else:
            m, c = None, color
        L = luminance(c)
        S = L * L
        W = P / cov[..., None]
        blend = np.zeros((h, w), bool)
        new_c, new_len, new_1, new_2 = c, np.ones((h, w), F), L, S
        if history is not None:
            front_c, fxc, fyc, _ = project(cam, W, w, h)
            front_v, fxv, fyv, dv = project(prev_cam, W, w, h)
            ys, xs = np.mgrid[0:h, 0:w]
            hx, hy = xs.astype(F) + (fxv - fxc), ys.astype(F) + (fyv - fyc)
            usable = front_c & front_v & (hx >= F(-1.0)) & (hx < F(w)) & (hy >= F(-1.0)) & (hy < F(h))
            hx, hy = np.where(usable, hx, F(0.0)), np.where(usable, hy, F(0.0))        # (the others are never read)
            fx0, fy0 = np.floor(hx), np.floor(hy)
            x0, y0 = fx0.astype(np.int32), fy0.astype(np.int32)
            ax, ay = hx - fx0, hy - fy0
            Hc, Hl, Hcov, HN, HW = [np.ascontiguousarray(history[k], F) for k in ("color", "length", "coverage", "normal", "position")]
            M = np.ascontiguousarray(moments, F)
            plane_bound = (tp2 * dv) * dv
            sum_w, sum_c, sum_n = np.zeros((h, w), F), np.zeros((h, w, 3), F), np.zeros((h, w), F)
            sum_1, sum_2 = np.zeros((h, w), F), np.zeros((h, w), F)
            for k in range(4):
                xq, yq = x0 + (k & 1), y0 + (k >> 1)
                b = (ax if k & 1 else F(1.0) - ax) * (ay if k >> 1 else F(1.0) - ay)
                in_image = (xq >= 0) & (xq < w) & (yq >= 0) & (yq < h)
                xg, yg = np.clip(xq, 0, w - 1), np.clip(yq, 0, h - 1)
                cq, lq, covq, Nq, Wq, Mq = Hc[yg, xg], Hl[yg, xg], Hcov[yg, xg], HN[yg, xg], HW[yg, xg], M[yg, xg]
                dn = N - Nq
                ok_n = dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1] + dn[..., 2] * dn[..., 2] <= tn2
                e = Wq - W
                pl = N[..., 0] * e[..., 0] + N[..., 1] * e[..., 1] + N[..., 2] * e[..., 2]
                ok_p = pl * pl <= plane_bound
                valid = usable & in_image & (covq > 0) & ok_n & ok_p
                sum_w = np.where(valid, sum_w + b, sum_w)
                sum_c = np.where(valid[..., None], sum_c + b[..., None] * cq, sum_c)
                sum_n = np.where(valid, sum_n + b * lq, sum_n)
                sum_1 = np.where(valid, sum_1 + b * Mq[..., 0], sum_1)
                sum_2 = np.where(valid, sum_2 + b * Mq[..., 1], sum_2)
            blend = usable & (sum_w > 0)
            h_c, h_n = sum_c / sum_w[..., None], sum_n / sum_w
            h_1, h_2 = sum_1 / sum_w, sum_2 / sum_w
            n = np.where(h_n < cap, h_n, cap)
            a = F(1.0) / (n + F(1.0))
            a = np.where(a < alpha, alpha, a)
            new_c = np.where(blend[..., None], h_c + (c - h_c) * a[..., None], c)
            new_len = np.where(blend, n + F(1.0), F(1.0))
            new_1 = np.where(blend, h_1 + (L - h_1) * a, L)
            new_2 = np.where(blend, h_2 + (S - h_2) * a, S)
        out = np.where(sky[..., None], color, new_c * m if demodulate else new_c)
        length = np.where(sky, F(0.0), new_len)
        zero3 = np.zeros((h, w, 3), F)
        hist = dict(color=np.where(sky[..., None], color, new_c), length=length, coverage=cov.copy(),
                    normal=np.where(sky[..., None], zero3, N), position=np.where(sky[..., None], zero3, W))
        mom = np.stack([np.where(sky, F(0.0), new_1), np.where(sky, F(0.0), new_2)], -1)
        var_t, clamped = temporal_variance(mom)
    classes = dict(sky=sky, fresh=~sky & ~blend, blended=~sky & blend, clamped=~sky & clamped, short=~sky & ~(length >= F(4.0)),
                   long=~sky & (length >= F(4.0)))
    for a_ in (out, length, mom, var_t, *hist.values()):
        assert a_.dtype == F, a_.dtype
    return dict(out=out, length=length, history=hist, moments=mom, var_t=var_t, classes=classes)


TILE_W, TILE_H = 32, 8                        # the variance launch's workgroup: one thread per pixel, four waves of two rows
HALO_W, HALO_H = TILE_W + 6, TILE_H + 6       # with the 7 x 7 window's halo
ALL_SKY, EARLY, HALO_WITH_LONG, HALO_ALL_SHORT = range(4)
TILE_KINDS = ("all sky", "early return with surface", "halo tile with long pixels", "halo tile all short")


def tiles(h, w):
    """(ty, tx, rows, columns) of every 32 x 8 tile of an h x w image, in the launch's block order; the slices are clipped."""
    for ty in range((h + TILE_H - 1) // TILE_H):
        for tx in range((w + TILE_W - 1) // TILE_W):
            yield ty, tx, slice(ty * TILE_H, min(h, (ty + 1) * TILE_H)), slice(tx * TILE_W, min(w, (tx + 1) * TILE_W))


def tile_classes(length, coverage):
    """What the variance launch does with every 32 x 8 tile of a NEW history: dict of (tiles_y, tiles_x) arrays -- kind (an index
    into TILE_KINDS: no surface pixel; surface pixels and none of them short, so the workgroup stores var_t and leaves; a short
    pixel and a long one; surface pixels that are all short), sky (the tile holds a sky pixel as well as whatever else), ragged (the
    image ends inside the tile) -- and count(kind, sky=None, ragged=None), the number of tiles of a kind with those marks."""
    length, cov = np.ascontiguousarray(length, F), np.ascontiguousarray(coverage, F)
    h, w = cov.shape
    shape = ((h + TILE_H - 1) // TILE_H, (w + TILE_W - 1) // TILE_W)
    kind, sky, ragged = np.zeros(shape, np.int32), np.zeros(shape, bool), np.zeros(shape, bool)
    for ty, tx, ys, xs in tiles(h, w):
        surface = cov[ys, xs] != 0
        short = surface & ~(length[ys, xs] >= F(4.0))
        kind[ty, tx] = (ALL_SKY if not surface.any() else EARLY if not short.any() else
                        HALO_ALL_SHORT if (short == surface).all() else HALO_WITH_LONG)
        sky[ty, tx] = not surface.all()
        ragged[ty, tx] = surface.shape != (TILE_H, TILE_W)

    def count(k, sky_=None, ragged_=None):
        m = kind == k
        m = m if sky_ is None else m & (sky == sky_)
        m = m if ragged_ is None else m & (ragged == ragged_)
        return int(m.sum())
    return dict(kind=kind, sky=sky, ragged=ragged, count=count)


def tile_counts(length, coverage):
    """tile_classes as one printable dict: the number of tiles per kind; of the early returns, how many are ragged and how many
    hold sky pixels."""
    c = tile_classes(length, coverage)
    n = {TILE_KINDS[k]: c["count"](k) for k in range(4)}
    n["early and ragged"], n["early with sky pixels"] = c["count"](EARLY, ragged_=True), c["count"](EARLY, sky_=True)
    return n


def _tile_of(h, w):
    """Per pixel: the tile's (ty, tx) and the pixel's (ly, lx) within it, as (h, w) int arrays."""
    ys, xs = np.mgrid[0:h, 0:w]
    return ys // TILE_H, xs // TILE_W, ys % TILE_H, xs % TILE_W


def variance(history, moments, sigma_normal=0.2, sigma_position=1.0, lost_halo=None, tile_decision=None, tile_threshold=None):
    """THE VARIANCE of a NEW history and its NEW moments: float32 (h, w).

    lost_halo, for tests of the TESTS only (it is not the contract): a dict with "axis" (0: x, 1: y).  Every tap that lies in another
    32 x 8 tile than its centre along that axis is skipped, as if the workgroup's halo had never arrived.

    tile_decision="wave", for tests of the TESTS only (it is not the contract): whether to stage the halo is decided per wave -- 64
    threads, two rows of the tile -- instead of per workgroup.  In a tile with a short pixel a wave without one neither stages nor
    counts: slot i of the 38 x 14 halo tile, filled by thread i % 256, arrives only if wave (i % 256) // 64 has a short pixel, and a
    slot that has not arrived counts as coverage 0.

    tile_threshold=3.0, for tests of the TESTS only (it is not the contract): the workgroup asks for a length below that threshold
    where the pixel asks for one below 4 -- a tile whose shortest surface length is >= the threshold writes var_t everywhere."""
    assert tile_decision in (None, "wave")
    length, cov, N, W = [np.ascontiguousarray(history[k], F) for k in ("length", "coverage", "normal", "position")]
    moments = np.ascontiguousarray(moments, F)
    h, w = cov.shape
    tyi, txi, ly, lx = _tile_of(h, w)
    short = (cov != 0) & ~(length >= F(4.0))
    if tile_decision == "wave":
        stages = np.zeros((tyi.max() + 1, txi.max() + 1, TILE_H // 2), bool)
        np.logical_or.at(stages, (tyi, txi, ly // 2), short)
    with np.errstate(all="ignore"):
        k_n, k_p = [F(1.0) / (F(s) * F(s)) for s in (sigma_normal, sigma_position)]
        var_t, _ = temporal_variance(moments)
        s_w, s_1, s_2 = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
        inside = np.ones((h, w), bool)
        for t in range(49):
            dy, dx = t // 7 - 3, t % 7 - 3
            valid = _shifted(inside, dx, dy)
            if valid is None:
                continue
            Nq, covq, Wq, Mq = [_shifted(a, dx, dy) for a in (N, cov, W, moments)]
            counts = valid & (covq != 0)
            if lost_halo is not None:
                counts = counts & ~_other_tile(h, w, 1, (dx, dy)[lost_halo["axis"]], lost_halo["axis"])
            if tile_decision == "wave":
                slot = (ly + 3 + dy) * HALO_W + (lx + 3 + dx)
                counts = counts & stages[tyi, txi, (slot % (TILE_W * TILE_H)) // 64]
            dn = N - Nq
            dn2 = dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1] + dn[..., 2] * dn[..., 2]
            dcov = cov - covq
            e = Wq - W
            pl = N[..., 0] * e[..., 0] + N[..., 1] * e[..., 1] + N[..., 2] * e[..., 2]
            D = dn2 * k_n + dcov * dcov * k_n + pl * pl * k_p
            r = F(1.0) / (F(1.0) + D)
            wgt = r * r
            s_w = np.where(counts, s_w + wgt, s_w)
            s_1 = np.where(counts, s_1 + wgt * Mq[..., 0], s_1)
            s_2 = np.where(counts, s_2 + wgt * Mq[..., 1], s_2)
        e1, e2 = s_1 / s_w, s_2 / s_w
        v = e2 - e1 * e1
        v = np.where(v > F(0.0), v, F(0.0))
        spatial = v * (F(4.0) / length)
        var = np.where(cov == 0, F(0.0), np.where(length >= F(4.0), var_t, spatial))
        if tile_threshold is not None:
            below = np.zeros((tyi.max() + 1, txi.max() + 1), bool)
            np.logical_or.at(below, (tyi, txi), (cov != 0) & ~(length >= F(tile_threshold)))
            var = np.where(below[tyi, txi] | (cov == 0), var, var_t)
    assert var.dtype == F
    return var


def guided(color, coverage, albedo, normal, position, variance, iterations=4, sigma_color=4.0, sigma_normal=0.2, sigma_position=1.0,
           demodulate=True, lost_halo=None, prefilter_on_lattice=False):
    """THE VARIANCE-GUIDED FILTER: (out f32 (h, w, 3), the last v f32 (h, w)).

    For tests of the TESTS only (they are not the contract): lost_halo as tests/_guided.py's -- a dict with "step" and "axis"; at that
    step every tap in another 32 x 8 sub-lattice tile than its centre along that axis is skipped --, and prefilter_on_lattice: the
    3 x 3 Gaussian of the variance is taken at the iteration's spacing s instead of unit spacing."""
    color, cov, normal, P, v = [np.ascontiguousarray(a, F) for a in (color, coverage, normal, position, variance)]
    h, w = cov.shape
    with np.errstate(all="ignore"):
        k_c, k_n, k_p = [F(1.0) / (F(s) * F(s)) for s in (sigma_color, sigma_normal, sigma_position)]
        N = normal * F(2.0) - cov[..., None]
        m = np.ascontiguousarray(albedo, F) + ((F(1.0) - cov) + F(1e-3))[..., None] if demodulate else np.ones_like(color)
        c = color / m
        inside = np.ones((h, w), bool)
        for i in range(iterations):
            s = 1 << i
            sp = s if prefilter_on_lattice else 1
            gs, gw = np.zeros((h, w), F), np.zeros((h, w), F)
            for t in range(9):
                dy, dx = t // 3 - 1, t % 3 - 1
                valid = _shifted(inside, sp * dx, sp * dy)
                if valid is None:
                    continue
                g = G[abs(dy)] * G[abs(dx)]
                gs = np.where(valid, gs + g * _shifted(v, sp * dx, sp * dy), gs)
                gw = np.where(valid, gw + g, gw)
            kv = k_c / (gs / gw + F(1e-8))
            L = luminance(c)
            sum_c, sum_w, sum_v = np.zeros((h, w, 3), F), np.zeros((h, w), F), np.zeros((h, w), F)
            for t in range(25):
                dy, dx = t // 5 - 2, t % 5 - 2
                valid = _shifted(inside, s * dx, s * dy)
                if valid is None:
                    continue
                Nq, covq, Pq, Lq, cq, vq = [_shifted(a, s * dx, s * dy) for a in (N, cov, P, L, c, v)]
                dn = N - Nq
                dn2 = dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1] + dn[..., 2] * dn[..., 2]
                dcov = cov - covq
                e = Pq - P
                pl = N[..., 0] * e[..., 0] + N[..., 1] * e[..., 1] + N[..., 2] * e[..., 2]
                dl = L - Lq
                D = dn2 * k_n + dcov * dcov * k_n + pl * pl * k_p + (dl * dl) * kv
                r = F(1.0) / (F(1.0) + D)
                wgt = ((H[abs(dy)] * H[abs(dx)]) * r) * r
                if lost_halo is not None and lost_halo["step"] == s:
                    valid = valid & ~_other_tile(h, w, s, (dx, dy)[lost_halo["axis"]], lost_halo["axis"])
                sum_c = np.where(valid[..., None], sum_c + wgt[..., None] * cq, sum_c)
                sum_w = np.where(valid, sum_w + wgt, sum_w)
                sum_v = np.where(valid, sum_v + (wgt * wgt) * vq, sum_v)
            c = np.where((cov == 0)[..., None], c, sum_c / sum_w[..., None])
            v = np.where(cov == 0, v, sum_v / (sum_w * sum_w))
        out = np.where((cov == 0)[..., None], color, c * m)
    assert out.dtype == F and v.dtype == F
    return out, v


def svgf_frame(linear, planes, cam, prev_cam, history, moments, temporal=None, variance_sigmas=None, guided_params=None):
    """One frame of rt_render_svgf's chain: the moments pass, the variance, the variance-guided filter over the accumulated output.
    dict(accumulated, linear_out, length, variance, variance_out, history, moments)."""
    args = [planes[k] for k in ("coverage", "albedo", "normal", "position")]
    acc = accumulate_moments(linear, *args, cam, prev_cam, history, moments, **(temporal or {}))
    var = variance(acc["history"], acc["moments"], **(variance_sigmas or {}))
    out, var_out = guided(acc["out"], *args, var, **(guided_params or {}))
    return dict(accumulated=acc["out"], linear_out=out, length=acc["length"], variance=var, variance_out=var_out,
                history=acc["history"], moments=acc["moments"], classes=acc["classes"])
