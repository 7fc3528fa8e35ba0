"""What the motion channel of a deforming mesh must return (include/rt_hip.h: "THE MOTION", "THE ACCUMULATION WITH MOTION"), from
the CPU oracle and numpy float32 alone.  TEST INFRASTRUCTURE ONLY; written from the contracts' text, not from the kernels'.

THE MOTION.  chain(): per (x, y, sample) oracle_primary_ray -> oracle_trace_rays (t, tri, u, v) -> oracle_fill_hit, with cast_ray's
back-face rule (oracle.c path_hit: a hit whose geometric or shading normal faces along the ray moves the origin to
point + RT_EPS * direction and costs an iteration) restated with tests/_step_inputs.py's fma32 / dot32.  It yields the feature hit of
every sample as (tri, u, v, point).  expected_motion() evaluates THE MOTION on the leaf tiles of two host scenes (leaf_tiles():
build_leaf_tile restated from the SoA coordinates).  The chain validates itself: its coverage and position sums must equal
tests/_features.expected's, which come from oracle_trace_path through a recording shader (tests/test_motion_cpu.py).

THE ACCUMULATION WITH MOTION.  accumulate_motion(): tests/_temporal.accumulate (and tests/_variance.accumulate_moments when moments
are carried) restated with the contract's differences: V_p = W_p + motion_p / cov is what the previous camera projects and what a
tap's plane distance is measured from; the history keeps W_p.  motion_case() makes the synthetic inputs of the GPU test.
"""
import ctypes as C

import numpy as np

from raytracing_c_amd import ctypes_abi as abi
from tests import _features, _oracle, _refit, _temporal as T
from tests._guided import luminance
from tests._step_inputs import RT_EPS, dot32, fma32

F = np.float32
MOTION_CHANNELS = 3


# ---------------------------------------------------------------------------------------------------------------------
# THE MOTION

def leaf_tiles(hs):
    """build_leaf_tile of every leaf group: float32 (groups, 9, 8) -- rows a.x, (b - a).x, (c - a).x, a.y, ... -- from the SoA
    coordinates of the host scene (slot_views: x0 x1 x2 y0 y1 y2 z0 z1 z2 per slot)."""
    coords, _, _ = _refit.slot_views(hs)
    n = len(coords)
    assert n % 8 == 0
    c = coords.reshape(n // 8, 8, 9)
    tiles = np.zeros((n // 8, 9, 8), F)
    with np.errstate(all="ignore"):
        for r in range(3):
            a = c[:, :, 3 * r]
            tiles[:, 3 * r] = a
            tiles[:, 3 * r + 1] = c[:, :, 3 * r + 1] - a
            tiles[:, 3 * r + 2] = c[:, :, 3 * r + 2] - a
    return tiles


def chain(hs, width, height, samples, max_bounces, sample_range=None):
    """The feature hit of every (y, x, sample) of the range: dict(hit (h, w, n) bool, tri (h, w, n) int32, uv (h, w, n, 2),
    point (h, w, n, 3) float32) -- what cast_ray's loop hands to a shader first, or hit False (a miss, or the iterations ran out)."""
    orc = _oracle.load()
    first, count = sample_range if sample_range else (0, samples)
    n = width * height * count
    rays = np.zeros((n, 6), F)
    cam = C.byref(hs.scene.camera)
    i = 0
    for y in range(height):
        for x in range(width):
            for s in range(first, first + count):
                orc.oracle_primary_ray(cam, width, height, x, y, s, rays[i].ctypes.data)
                i += 1
    hit = np.zeros(n, bool)
    tri = np.full(n, -1, np.int32)
    uv = np.zeros((n, 2), F)
    point = np.zeros((n, 3), F)
    active = np.arange(n)
    scene = C.byref(hs.scene)
    filled = abi.Hit()
    for _ in range(max_bounces):
        if len(active) == 0:
            break
        r = np.ascontiguousarray(rays[active])
        t, k, b = np.zeros(len(active), F), np.zeros(len(active), np.int32), np.zeros((len(active), 2), F)
        orc.oracle_trace_rays(scene, len(active), r.ctypes.data, t.ctypes.data, k.ctypes.data, b.ctypes.data)
        on = np.flatnonzero(k >= 0)                                   # (a miss ends the path with nothing)
        ngeo, nint, pt = np.zeros((len(on), 3), F), np.zeros((len(on), 3), F), np.zeros((len(on), 3), F)
        for j, a in enumerate(on):
            ray = abi.Ray.from_buffer_copy(r[a].tobytes())
            orc.oracle_fill_hit(scene, C.byref(ray), float(t[a]), int(k[a]), float(b[a, 0]), float(b[a, 1]), C.byref(filled))
            ngeo[j] = (filled.normal_geo.x, filled.normal_geo.y, filled.normal_geo.z)
            nint[j] = (filled.normal.x, filled.normal.y, filled.normal.z)
            pt[j] = (filled.point.x, filled.point.y, filled.point.z)
        d = r[on, 3:6]
        with np.errstate(all="ignore"):
            back = (dot32(ngeo, d) > F(0.0)) | (dot32(nint, d) > F(0.0))
        idx = active[on]
        front = ~back
        hit[idx[front]], tri[idx[front]], uv[idx[front]], point[idx[front]] = True, k[on][front], b[on][front], pt[front]
        through = idx[back]
        rays[through, 0:3] = fma32(d[back], RT_EPS, pt[back])         # origin = point + RT_EPS * direction, one fma per component
        active = through
    shape = (height, width, count)
    return dict(hit=hit.reshape(shape), tri=tri.reshape(shape), uv=uv.reshape(shape + (2,)), point=point.reshape(shape + (3,)))


def _sum_signed(values, hit):
    """u64 (h, w, 3): rt_accum_quantize_signed of `values` (h, w, n, 3) summed over the samples with a hit, mod 2^64."""
    h, w, n, _ = values.shape
    out = np.zeros((h, w, 3), np.uint64)
    for y in range(h):
        for x in range(w):
            acc = [0, 0, 0]
            for s in range(n):
                if hit[y, x, s]:
                    for c in range(3):
                        acc[c] += _features.quantize_signed(values[y, x, s, c])
            out[y, x] = [v & 0xFFFFFFFFFFFFFFFF for v in acc]
    return out


def chain_sums(ch):
    """(coverage sums (h, w) uint64, position sums (h, w, 3) uint64) of a chain: what tests/_features.expected has in channels 0
    and 7 .. 9."""
    cov = (ch["hit"].sum(axis=2).astype(np.uint64)) << np.uint64(32)
    return cov, _sum_signed(ch["point"], ch["hit"])


def motion_of(ch, tiles_cur, tiles_kept):
    """THE MOTION of every sample of a chain, float32 (h, w, n, 3); 0 where there is no feature hit."""
    tri = np.where(ch["hit"], ch["tri"], 0)
    g, k = tri >> 3, tri & 7
    u, v = ch["uv"][..., 0], ch["uv"][..., 1]
    out = np.zeros(ch["hit"].shape + (3,), F)
    with np.errstate(all="ignore"):
        for r in range(3):
            cur = (tiles_cur[g, 3 * r, k] + u * tiles_cur[g, 3 * r + 1, k]) + v * tiles_cur[g, 3 * r + 2, k]
            was = (tiles_kept[g, 3 * r, k] + u * tiles_kept[g, 3 * r + 1, k]) + v * tiles_kept[g, 3 * r + 2, k]
            out[..., r] = np.where(ch["hit"], was - cur, F(0.0))
    assert out.dtype == F
    return out


def expected_motion(ch, tiles_cur, tiles_kept):
    """The motion sums, u64 (h, w, 3)."""
    return _sum_signed(motion_of(ch, tiles_cur, tiles_kept), ch["hit"])


def resolve_motion(sums, samples):
    """rt_accum_resolve_signed: float32 (h, w, 3)."""
    s = np.ascontiguousarray(sums, np.uint64).view(np.int64).astype(np.float64)
    return (s / (float(samples) * 4294967296.0)).astype(F)


def displaced_passthrough():
    """tests._features.passthrough_scene() and the positions that move its two FRONT quads (triangles 0, 1 and 4, 5) sideways,
    up and towards the camera; the back-facing quads in front of them stay.  Returns (hs, moved positions (n, 3, 3))."""
    hs = _features.passthrough_scene()
    P = hs.source_triangles["positions"].copy()
    P[[0, 1]] += np.array([0.07, -0.03, 0.05], F)
    P[[4, 5]] += np.array([-0.04, 0.06, -0.08], F)
    return hs, P


# ---------------------------------------------------------------------------------------------------------------------
# THE ACCUMULATION WITH MOTION

def accumulate_motion(color, coverage, albedo, normal, position, motion, cam, prev_cam=None, history=None, moments=None,
                      with_moments=False, alpha=0.05, max_history=64, normal_tolerance=0.3, plane_tolerance=0.02, demodulate=True,
                      plane_from_w=False):
    """dict(out, length, history, cls -- tests/_temporal.accumulate's -- and with moments (or with_moments) moments (h, w, 2)).
    plane_from_w: the WRONG restatement that measures a tap's plane distance from W_p (tests/test_motion_cpu.py)."""
    with_moments = with_moments or moments is not None
    color, cov, normal, P, motion = [np.ascontiguousarray(a, F) for a in (color, coverage, normal, position, motion)]
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
        V = W + motion / cov[..., None]                                # where the mean surface point was
        cls = np.full((h, w), T.NO_HISTORY, np.int32)
        blend = np.zeros((h, w), bool)
        new_c, new_len, new_1, new_2 = c, np.ones((h, w), F), L, S
        if history is not None:
            front_c, fxc, fyc, _ = T.project(cam, W, w, h)
            front_v, fxv, fyv, dv = T.project(prev_cam, V, w, h)
            ys, xs = np.mgrid[0:h, 0:w]
            hx, hy = xs.astype(F) + (fxv - fxc), ys.astype(F) + (fyv - fyc)
            inside = (hx >= F(-1.0)) & (hx < F(w)) & (hy >= F(-1.0)) & (hy < F(h))
            front = front_c & front_v
            usable = front & inside
            hx, hy = np.where(usable, hx, F(0.0)), np.where(usable, hy, F(0.0))        # (the others are never read)
            fx0, fy0 = np.floor(hx), np.floor(hy)
            x0, y0 = fx0.astype(np.int32), fy0.astype(np.int32)
            ax, ay = hx - fx0, hy - fy0
            Hc, Hl, Hcov, HN, HW = [np.ascontiguousarray(history[k], F) for k in ("color", "length", "coverage", "normal", "position")]
            M = np.ascontiguousarray(moments, F) if moments is not None else np.zeros((h, w, 2), F)
            plane_bound = (tp2 * dv) * dv
            sum_w, sum_c, sum_n = np.zeros((h, w), F), np.zeros((h, w, 3), F), np.zeros((h, w), F)
            sum_1, sum_2 = np.zeros((h, w), F), np.zeros((h, w), F)
            n_surface, n_normal_ok, n_valid = np.zeros((h, w), np.int32), np.zeros((h, w), np.int32), np.zeros((h, w), np.int32)
            origin = W if plane_from_w else V
            for k in range(4):
                xq, yq = x0 + (k & 1), y0 + (k >> 1)
                b = (ax if k & 1 else F(1.0) - ax) * (ay if k >> 1 else F(1.0) - ay)
                in_image = (xq >= 0) & (xq < w) & (yq >= 0) & (yq < h)
                xg, yg = np.clip(xq, 0, w - 1), np.clip(yq, 0, h - 1)
                cq, lq, covq, Nq, Wq, Mq = Hc[yg, xg], Hl[yg, xg], Hcov[yg, xg], HN[yg, xg], HW[yg, xg], M[yg, xg]
                surface = usable & in_image & (covq > 0)
                dn = N - Nq
                ok_n = dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1] + dn[..., 2] * dn[..., 2] <= tn2
                e = Wq - origin
                pl = N[..., 0] * e[..., 0] + N[..., 1] * e[..., 1] + N[..., 2] * e[..., 2]
                ok_p = pl * pl <= plane_bound
                valid = surface & ok_n & ok_p
                sum_w = np.where(valid, sum_w + b, sum_w)
                sum_c = np.where(valid[..., None], sum_c + b[..., None] * cq, sum_c)
                sum_n = np.where(valid, sum_n + b * lq, sum_n)
                sum_1 = np.where(valid, sum_1 + b * Mq[..., 0], sum_1)
                sum_2 = np.where(valid, sum_2 + b * Mq[..., 1], sum_2)
                n_surface += surface
                n_normal_ok += surface & ok_n
                n_valid += valid
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
            cls = np.where(~front, T.BEHIND,
                  np.where(~inside, T.OUTSIDE,
                  np.where(n_valid == 4, T.ALL_VALID,
                  np.where(n_valid > 0, T.SOME_VALID,
                  np.where(n_surface == 0, T.NO_SURFACE,
                  np.where(n_normal_ok == 0, T.NORMAL_REJECTED, T.PLANE_REJECTED)))))).astype(np.int32)
        cls = np.where(sky, T.SKY, cls).astype(np.int32)
        out = np.where(sky[..., None], color, new_c * m if demodulate else new_c)
        length = np.where(sky, F(0.0), new_len)
        zero3 = np.zeros((h, w, 3), F)
        hist = dict(color=np.where(sky[..., None], color, new_c), length=length, coverage=cov.copy(),
                    normal=np.where(sky[..., None], zero3, N), position=np.where(sky[..., None], zero3, W))     # (W_p, not V_p)
        res = dict(out=out, length=length, history=hist, cls=cls)
        if with_moments:
            res["moments"] = np.stack([np.where(sky, F(0.0), new_1), np.where(sky, F(0.0), new_2)], -1)
    for a_ in (out, length, *hist.values(), *([res["moments"]] if with_moments else [])):
        assert a_.dtype == F, a_.dtype
    return res


def _world_at(fx, fy, z, w, h, focal):
    """The point at depth -z that a camera at the origin looking down -z (tests/test_gpu_temporal.CAM_OLD) projects to (fx, fy)."""
    d = -z
    ux, uy = fx / (w * 0.5) - 1.0, fy / (h * 0.5) - 1.0
    return np.stack([ux * (w / h) * d / focal, -uy * d / focal, np.broadcast_to(z, np.shape(fx)) + 0.0 * fx], -1)


_motion_cases = {}
# what the motion cases are accumulated with: a short cap and a large alpha, so that the lengths differ; a normal tolerance that
# accepts partially covered neighbours (N = n * cov: up to 0.75 apart) and still rejects the frame's block with another normal
MOTION_KW = dict(alpha=0.2, max_history=3, normal_tolerance=0.8, plane_tolerance=0.02)


def motion_case(w, h):
    """(planes of the new frame, history, motion (h, w, 3)): tests/test_gpu_temporal._case(w, h) -- two planes seen by a camera
    that moved, over a history of two frames -- with the surface pushed 0.5 towards the camera since, and a motion plane AIMED per
    pixel set: where the point was is chosen so that the pixel's four taps land on a chosen spot of the history.  The sets, in
    reading order over the fully covered pixels outside the frame's special blocks: 24 pixels each aimed outside the image, into the
    history's sky block, half a unit off the old plane, and on the sky block's edge; every other one at the spot it came from on
    its old plane (all four taps valid).  The frame's own blocks give the rest: sky (motion is not read there), points behind
    the cameras, another normal.  Shared, read-only."""
    if (w, h) in _motion_cases:
        return _motion_cases[(w, h)]
    from tests import test_gpu_temporal as G
    P0, hist = G._case(w, h)
    focal = float(G.FOCAL)
    cov = P0["coverage"]
    c3 = cov[..., None].astype(np.float64)
    with np.errstate(all="ignore"):
        W0 = np.where(c3 > 0, P0["position"].astype(np.float64) / c3, 0.0)
    W0[..., 2] += 0.5                                                  # the surface moved towards the camera ...
    position = (W0 * c3).astype(F)
    P = dict(P0, position=position)
    with np.errstate(all="ignore"):
        W = position / cov[..., None]                                  # ... and this is what the kernel sees of it
        _, fxc, fyc, _ = T.project(G.CAM_NEW, W, w, h)
    fxc, fyc = fxc.astype(np.float64), fyc.astype(np.float64)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    sx, sy = (2 * w) // 3, h // 3                                       # the history's sky block: 6 x 5 from here
    HW = hist["position"].astype(np.float64)

    def aim(tx, ty, dz=0.0, z=None):
        """V for every pixel so that hx = tx + 0.5, hy = ty + 0.5: the taps are (tx, ty) .. (tx + 1, ty + 1)"""
        zt = (HW[ty, tx, 2] if z is None else z) + dz
        return _world_at((tx + 0.5) - xs + fxc, (ty + 0.5) - ys + fyc, zt, w, h, focal)

    # a spot of the far plane, away from the sky block and the near plane's edge, whose four taps are fully covered
    full = hist["coverage"] == 1
    interior = next((tx, ty) for ty in range(0, sy - 2) for tx in range(w - 3, sx + 6, -1) if full[ty:ty + 2, tx:tx + 2].all())
    edge_y = next(ty for ty in range(sy, sy + 4) if full[ty:ty + 2, sx - 1].all())
    V = aim(*interior)                                                 # (also the pixels with another normal, and those behind)
    free = (cov > 0)
    free[h // 2:h // 2 + 4, w // 8:w // 8 + 7] = False                 # behind both cameras
    free[h // 8:h // 8 + 4, w // 2:w // 2 + 8] = False                 # another normal
    order = np.flatnonzero((free & (cov == 1)).ravel())                # (fully covered: the normal test compares N = n * cov)
    sets = [order[i * 24:(i + 1) * 24] for i in range(4)]
    targets = [aim(w + 10, 1, z=-6.0), aim(sx + 2, sy + 1, z=-6.0), aim(*interior, dz=0.5), aim(sx - 1, edge_y)]
    Vf = V.reshape(-1, 3)
    for idx, tgt in zip(sets, targets):
        Vf[idx] = tgt.reshape(-1, 3)[idx]
    motion = ((Vf.reshape(h, w, 3) - W.astype(np.float64)) * c3).astype(F)
    motion[cov == 0] = (0.25, -0.5, 0.125)                             # (sky: never read)
    assert np.isfinite(motion).all()
    for a in (position, motion):
        a.setflags(write=False)
    _motion_cases[(w, h)] = (P, hist, motion)
    return _motion_cases[(w, h)]
