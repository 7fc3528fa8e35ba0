"""What temporal accumulation must return: the contract of include/rt_hip.h ("THE ACCUMULATION") restated in numpy float32, one
rounded operation per numpy call, the four taps in the contract's order as gathers with validity masks, no loop over pixels.
TEST INFRASTRUCTURE ONLY; written from the contract's text, not from the kernel's.

A camera is (view_matrix float32 (4, 4), focal_length); a history is a dict of planes: color (h, w, 3), length (h, w),
coverage (h, w), normal (h, w, 3) -- the signed N -- and position (h, w, 3) -- W.
"""
import numpy as np

F = np.float32

# the per-pixel class, by precedence: what decided the pixel's fate
SKY, NO_HISTORY, BEHIND, OUTSIDE, NO_SURFACE, NORMAL_REJECTED, PLANE_REJECTED, SOME_VALID, ALL_VALID = range(9)
CLASS_NAMES = ["sky", "no history given", "behind a camera", "outside the image", "no tap on a surface (outside the image or sky)",
               "all taps rejected by the normal test", "all taps rejected by the plane test", "some taps valid", "all four taps valid"]


def camera(view_matrix, focal_length):
    return np.ascontiguousarray(view_matrix, F).reshape(4, 4), F(focal_length)


def camera_of(cam):
    """(view_matrix, focal_length) of a ctypes Camera."""
    return camera(np.array([[cam.view_matrix.rows[i][k] for k in range(4)] for i in range(4)], F), cam.focal_length)


def project(cam, W, w, h):
    """proj(cam, W): front (h, w) bool, fx, fy, d."""
    M, focal = cam
    half_w, half_h, aspect = F(w) * F(0.5), F(h) * F(0.5), F(w) / F(h)
    ex, ey, ez = W[..., 0] - M[0, 3], W[..., 1] - M[1, 3], W[..., 2] - M[2, 3]
    cx = M[0, 0] * ex + M[1, 0] * ey + M[2, 0] * ez
    cy = M[0, 1] * ex + M[1, 1] * ey + M[2, 1] * ez
    cz = M[0, 2] * ex + M[1, 2] * ey + M[2, 2] * ez
    d = F(0.0) - cz
    ux = ((cx * focal) / d) / aspect
    uy = F(0.0) - ((cy * focal) / d)
    return cz < F(0.0), (ux + F(1.0)) * half_w, (uy + F(1.0)) * half_h, d


def accumulate(color, coverage, albedo, normal, position, cam, prev_cam=None, history=None, alpha=0.05, max_history=64,
               normal_tolerance=0.3, plane_tolerance=0.02, demodulate=True):
    """dict(out (h, w, 3), length (h, w), history (the new one), cls (h, w) int: the class of every pixel)."""
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
        W = P / cov[..., None]
        cls = np.full((h, w), NO_HISTORY, np.int32)
        blend = np.zeros((h, w), bool)
        new_c, new_len = c, np.ones((h, w), F)
        if history is not None:
            front_c, fxc, fyc, _ = project(cam, W, w, h)
            front_v, fxv, fyv, dv = project(prev_cam, W, w, h)
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
            plane_bound = (tp2 * dv) * dv
            sum_w, sum_c, sum_n = np.zeros((h, w), F), np.zeros((h, w, 3), F), np.zeros((h, w), F)
            n_surface = np.zeros((h, w), np.int32)
            n_normal_ok = np.zeros((h, w), np.int32)
            n_valid = np.zeros((h, w), np.int32)
            for k in range(4):
                xq, yq = x0 + (k & 1), y0 + (k >> 1)
                b = (ax if k & 1 else F(1.0) - ax) * (ay if k >> 1 else F(1.0) - ay)
                in_image = (xq >= 0) & (xq < w) & (yq >= 0) & (yq < h)
                xg, yg = np.clip(xq, 0, w - 1), np.clip(yq, 0, h - 1)
                cq, lq, covq, Nq, Wq = Hc[yg, xg], Hl[yg, xg], Hcov[yg, xg], HN[yg, xg], HW[yg, xg]
                surface = usable & in_image & (covq > 0)
                dn = N - Nq
                ok_n = dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1] + dn[..., 2] * dn[..., 2] <= tn2
                e = Wq - W
                pl = N[..., 0] * e[..., 0] + N[..., 1] * e[..., 1] + N[..., 2] * e[..., 2]
                ok_p = pl * pl <= plane_bound
                valid = surface & ok_n & ok_p
                sum_w = np.where(valid, sum_w + b, sum_w)
                sum_c = np.where(valid[..., None], sum_c + b[..., None] * cq, sum_c)
                sum_n = np.where(valid, sum_n + b * lq, sum_n)
                n_surface += surface
                n_normal_ok += surface & ok_n
                n_valid += valid
            blend = usable & (sum_w > 0)
            h_c, h_n = sum_c / sum_w[..., None], sum_n / sum_w
            n = np.where(h_n < cap, h_n, cap)
            a = F(1.0) / (n + F(1.0))
            a = np.where(a < alpha, alpha, a)
            new_c = np.where(blend[..., None], h_c + (c - h_c) * a[..., None], c)
            new_len = np.where(blend, n + F(1.0), F(1.0))
            cls = np.where(~front, BEHIND,
                  np.where(~inside, OUTSIDE,
                  np.where(n_valid == 4, ALL_VALID,
                  np.where(n_valid > 0, SOME_VALID,
                  np.where(n_surface == 0, NO_SURFACE,
                  np.where(n_normal_ok == 0, NORMAL_REJECTED, PLANE_REJECTED)))))).astype(np.int32)
        cls = np.where(sky, SKY, cls).astype(np.int32)
        out = np.where(sky[..., None], color, new_c * m if demodulate else new_c)
        length = np.where(sky, F(0.0), new_len)
        zero3 = np.zeros((h, w, 3), F)
        hist = dict(color=np.where(sky[..., None], color, new_c), length=length, coverage=cov.copy(),
                    normal=np.where(sky[..., None], zero3, N), position=np.where(sky[..., None], zero3, W))
    for a_ in (out, length, *hist.values()):
        assert a_.dtype == F, a_.dtype
    return dict(out=out, length=length, history=hist, cls=cls)


def encode_u8(x):
    from tests import _guided
    return _guided.encode_u8(x)


def pack_history(hist):
    """The device layout: three planes of float4 records, float32 (3, h, w, 4)."""
    h, w = hist["length"].shape
    rec = np.zeros((3, h, w, 4), F)
    rec[0, ..., :3], rec[0, ..., 3] = hist["color"], hist["length"]
    rec[1, ..., :3], rec[1, ..., 3] = hist["normal"], hist["coverage"]
    rec[2, ..., :3] = hist["position"]
    return rec


def unpack_history(rec):
    rec = np.asarray(rec, F)
    return dict(color=rec[0, ..., :3].copy(), length=rec[0, ..., 3].copy(), coverage=rec[1, ..., 3].copy(),
                normal=rec[1, ..., :3].copy(), position=rec[2, ..., :3].copy())
