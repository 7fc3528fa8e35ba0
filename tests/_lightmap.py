"""Helpers of the lightmap and denoiser tests: a numpy restatement of the reference's UV rasteriser, images with row
padding, scenes whose lightmaps carry radiance a u8 can see, and the conditions that keep a comparison from being blind.

The lightmap stores RAW radiance truncated to u8 (no *255, oracle/oracle.h), so a scene whose radiance stays below 1 bakes
to a map of zeros and a comparison of two such maps checks only which texels are owned.  emissive_soup() emits in the tens
to low hundreds; assert_discriminating() states what a map must contain before a test may compare it with anything.
"""
import ctypes as C

import numpy as np

from raytracing_c_amd import ctypes_abi as abi

F = np.float32
EPSILON = F(0.0001)                   # common.h:8
ALL_CHECKS = ("written", "overlap", "distinct", "zero", "saturated")


def aos_uvs(hs):
    """(slots, 3, 2) fp32 VIEW of the UVs inside the host scene's Triangle_AOS records: six floats at byte 72 of each
    112-byte record (scene.h:46-51).  Writing through it edits the scene in place."""
    n = hs.n_slots
    raw = np.ctypeslib.as_array(C.cast(hs.scene.triangles.aos, C.POINTER(C.c_uint8)), (n, 112))
    return raw[:, 72:96].view(np.float32).reshape(n, 3, 2)


def np_rasterise(hs, W, H):
    """raytracer.c:722-747 in numpy, stepwise in fp32: per triangle slot the integer bounds by C truncation
    (`i32 min_x = min(a, min(b, c)) * width`), p = uv * (width, height), denom, w0, w1 and w2 = 1 - w0 - w1 in the
    reference's association, accepted when all three are >= -EPSILON; texels outside the image are skipped (the reference
    would write out of bounds, oracle.h).  Returns (owner, count), both (H, W) int32: the LAST covering slot or -1, and the
    number of covering slots.  `hs` may also be a (slots, 3, 2) array of UVs.

    |uv * size| must stay far below 2^31: beyond it the C conversion to i32 is undefined and the reference's loop would not
    finish.  That is outside the contract of lightmap_bake and is not tested."""
    uv = np.array(hs if isinstance(hs, np.ndarray) else aos_uvs(hs), F)
    fw, fh = F(W), F(H)
    owner = np.full(H * W, -1, np.int32)
    count = np.zeros(H * W, np.int32)
    ax, ay, bx, by, cx, cy = (uv[:, k, j] for k in range(3) for j in range(2))
    min_x = np.trunc(np.minimum(ax, np.minimum(bx, cx)) * fw).astype(np.int64)
    max_x = np.trunc(np.maximum(ax, np.maximum(bx, cx)) * fw).astype(np.int64)
    min_y = np.trunc(np.minimum(ay, np.minimum(by, cy)) * fh).astype(np.int64)
    max_y = np.trunc(np.maximum(ay, np.maximum(by, cy)) * fh).astype(np.int64)
    # the part of [min, max] that lies on the image; the loop over the rest writes nothing
    x0, x1, y0, y1 = np.maximum(min_x, 0), np.minimum(max_x, W - 1), np.maximum(min_y, 0), np.minimum(max_y, H - 1)
    bw, bh = x1 - x0 + 1, y1 - y0 + 1

    def accept(sel, x, y):
        """triangles `sel` (n,) against texels x, y (n, m) int: the acceptance test of raytracer.c:733-747"""
        p0x, p0y = (ax[sel] * fw)[:, None], (ay[sel] * fh)[:, None]
        p1x, p1y = (bx[sel] * fw)[:, None], (by[sel] * fh)[:, None]
        p2x, p2y = (cx[sel] * fw)[:, None], (cy[sel] * fh)[:, None]
        px, py = x.astype(F), y.astype(F)
        denom = (p1y - p2y) * (p0x - p2x) + (p2x - p1x) * (p0y - p2y)
        w0 = ((p1y - p2y) * (px - p2x) + (p2x - p1x) * (py - p2y)) / denom
        w1 = ((p2y - p0y) * (px - p2x) + (p0x - p2x) * (py - p2y)) / denom
        w2 = F(1.0) - w0 - w1
        assert w0.dtype == F and w1.dtype == F and w2.dtype == F
        return (w0 >= -EPSILON) & (w1 >= -EPSILON) & (w2 >= -EPSILON)

    def record(sel, x, y, hit):
        tri = np.broadcast_to(sel[:, None], hit.shape)[hit].astype(np.int32)
        at = (y * W + x)[hit]
        np.add.at(count, at, 1)
        np.maximum.at(owner, at, tri)

    with np.errstate(all="ignore"):
        # boxes of at most 4 x 4 texels (most triangles of a large soup): all of them at once, 16 candidates each
        K = 4
        small = np.nonzero((bw >= 1) & (bh >= 1) & (bw <= K) & (bh <= K))[0]
        if len(small):
            ox, oy = np.arange(K * K) % K, np.arange(K * K) // K
            x, y = x0[small, None] + ox, y0[small, None] + oy
            inside = (ox < bw[small, None]) & (oy < bh[small, None])
            x, y = np.where(inside, x, 0), np.where(inside, y, 0)
            record(small, x, y, accept(small, x, y) & inside)
        # larger boxes: chunks of triangles against the whole image, masked by the box
        large = np.nonzero((bw >= 1) & (bh >= 1) & ((bw > K) | (bh > K)))[0]
        ys, xs = np.mgrid[0:H, 0:W]
        xi, yi = xs.reshape(1, -1), ys.reshape(1, -1)
        step = max(1, (1 << 21) // (W * H))
        for s in range(0, len(large), step):
            sel = large[s:s + step]
            x, y = np.broadcast_to(xi, (len(sel), W * H)), np.broadcast_to(yi, (len(sel), W * H))
            inside = (xi >= x0[sel, None]) & (xi <= x1[sel, None]) & (yi >= y0[sel, None]) & (yi <= y1[sel, None])
            record(sel, x, y, accept(sel, x, y) & inside)
    return owner.reshape(H, W), count.reshape(H, W)


def padded_image(H, W, comp, stride, fill):
    """abi.Image of W x H texels over a backing array of (H, stride, comp) bytes, all `fill`: rows have stride - W texels
    of padding.  Comparisons are made over the WHOLE backing array: padding, alpha and untouched texels included."""
    assert stride >= W and comp >= 1
    arr = np.full((H, stride, comp), fill, np.uint8)
    img = abi.Image()
    img.components, img.pixel_type, img.width, img.stride, img.height = comp, 0, W, stride, H
    img.pixels.data, img.pixels.len = arr.ctypes.data, arr.size
    return img, arr


def oracle_bake(oracle, hs, H, W, comp=3, stride=None, samples=1, fill=7, seed=0x1234ABCD):
    """The oracle's bake into a fresh padded image; returns the backing array."""
    from tests import _oracle
    img, arr = padded_image(H, W, comp, W if stride is None else stride, fill)
    cfg = _oracle.config_for(hs, seed=seed, n_threads=1)
    oracle.oracle_lightmap_bake(C.byref(img), C.byref(hs.scene), samples, C.byref(cfg))
    return arr


def written_mask(oracle, hs, H, W, comp=3, stride=None, samples=1):
    """Bakes over fill 7 and over fill 200: a texel is written iff it differs from its fill in either bake.  Returns
    (mask (H, W), the two backing arrays)."""
    a = oracle_bake(oracle, hs, H, W, comp, stride, samples, fill=7)
    b = oracle_bake(oracle, hs, H, W, comp, stride, samples, fill=200)
    mask = (a[:, :W, :3] != 7).any(axis=-1) | (b[:, :W, :3] != 200).any(axis=-1)
    return mask, a, b


_printed = set()


def assert_discriminating(lm, mask, count, checks=ALL_CHECKS, label=""):
    """What a baked map must contain before a comparison against it means anything, computed on the oracle's output alone.
    `lm`: (H, W, >= 3) texels (no padding columns), `mask`: written texels, `count`: covering triangles per texel
    (np_rasterise).  `checks` names the conditions that make sense for the case; the numbers are printed once per label.

      written    share of written texels within [0.15, 0.95]: the owner mask has an inside and an outside
      overlap    share of texels covered by >= 2 triangles >= 0.10: "last triangle wins" decides something
      distinct   >= 48 distinct u8 values among the written texels' channels
      zero       at most half of the written channel values are 0
      saturated  at most 5 % of them are 255
      some       (tiny maps) at least one texel is written with a value other than 0
    """
    vals = lm[..., :3][mask]
    st = dict(written=float(mask.mean()), overlap=float((count >= 2).mean()), distinct=int(len(np.unique(vals))),
              zero=float((vals == 0).mean()) if vals.size else 1.0, saturated=float((vals == 255).mean()) if vals.size else 0.0)
    if label not in _printed:
        _printed.add(label)
        print(f"\nlightmap[{label}] {lm.shape[1]}x{lm.shape[0]}: written {st['written']:.3f} overlap {st['overlap']:.3f} "
              f"distinct {st['distinct']} zero {st['zero']:.3f} saturated {st['saturated']:.3f} checks={','.join(checks)}")
    for c in checks:
        assert c in ALL_CHECKS + ("some",), c
    if "written" in checks:
        assert 0.15 <= st["written"] <= 0.95, st
    if "overlap" in checks:
        assert st["overlap"] >= 0.10, st
    if "distinct" in checks:
        assert st["distinct"] >= 48, st
    if "zero" in checks:
        assert st["zero"] <= 0.5, st
    if "saturated" in checks:
        assert st["saturated"] <= 0.05, st
    if "some" in checks:
        assert vals.size and vals.max() > 0, st
    return st


# UVs of the special triangles of emissive_soup(), by name
SPECIAL_UVS = {
    "zero_area":   [(0.5, 0.5), (0.5, 0.5), (0.5, 0.5)],                 # denom == 0: 0/0 and x/0, never accepted
    "collinear":   [(0.25, 0.25), (0.5, 0.5), (0.75, 0.75)],             # denom == 0 exactly as well (every product is exact)
    "sliver":      [(0.1, 0.1), (0.3, 0.3), (0.5, 0.5)],                 # collinear but for the rounding of 0.1f * size: a tiny denom
    "sub_texel":   [(0.4010, 0.6010), (0.4030, 0.6015), (0.4015, 0.6030)],
    # two triangles sharing the edge u = 0.5, v in [0.25, 0.75]: on a map of even width the edge runs exactly through
    # texel centres, both triangles accept them with a weight of 0 and the later slot wins
    "edge_left":   [(0.5, 0.25), (0.5, 0.75), (0.3, 0.5)],
    "edge_right":  [(0.5, 0.25), (0.5, 0.75), (0.7, 0.5)],
    "zero_normal": [(0.6, 0.1), (0.9, 0.15), (0.7, 0.4)],                # three zero vertex normals: the 64-try guard, writes 0
    "outside":     [(1.5, 1.6), (1.9, 1.5), (1.7, 1.9)],                 # wholly off the map
    "negative":    [(-0.15, 0.3), (0.2, 0.1), (0.1, 0.6)],               # straddles u = 0: (int) truncates toward zero
    "origin":      [(-0.1, -0.1), (0.3, -0.05), (-0.05, 0.3)],           # holds texel (0, 0): a 1 x 1 map has an owner
}


def emissive_soup(seed, n_tris, chart=0.15, emission=60.0, textured=False, offset=0.0, builder="reference"):
    """The triangle soup of tests.test_gpu_random_scenes.make_scene -- duplicated triangles, a degenerate one, axis-aligned
    ones, perturbed vertex normals, materials that switch on every optional shading term -- made fit for baking:

      * UV charts of a controlled size: a random centre in [-0.2, 1.2]^2 plus offsets of scale `chart`, so that a map is
        partly covered, partly overlapped and clipped by every edge (make_scene's +-2 spread covers any map completely);
      * emission in the tens to low hundreds (`emission` times make_scene's 0 / 2), plus a floor of emission / 10 on
        every channel so that few texels truncate to 0;
      * `textured`: albedo / normal / metal-roughness / emission textures as in make_scene, or none at all (then UVs feed
        nothing but the rasteriser);
      * the special triangles of SPECIAL_UVS (n_tris >= 24);
      * `offset` translates every vertex by (offset, offset, offset), as tests/_far_scene.py does.
    """
    from raytracing_c_amd.background import procedural_background
    from raytracing_c_amd.loaders import camera_from_trs
    from raytracing_c_amd.scene import Material, build_scene
    assert n_tris >= 24
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1, 1, (n_tris, 1, 3))
    P = (c + rng.normal(size=(n_tris, 3, 3)) * rng.choice([0.05, 0.3, 0.8], (n_tris, 1, 1))).astype(np.float32)
    k = max(2, n_tris // 10)
    P[-k:] = P[:k]                                     # exact duplicates
    P[k] = P[k][[0, 0, 0]]                             # a degenerate triangle
    P[k + 1] = [[0, -1, -1], [0, 1, -1], [0, 1, 1]]
    P[k + 2] = [[-1, 0, -1], [1, 0, -1], [1, 0, 1]]
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    fn = np.cross(e1, e2)
    fn = fn / np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-20)
    N = (fn[:, None, :] + rng.normal(size=(n_tris, 3, 3)) * 0.2).astype(np.float32)
    UV = (rng.uniform(-0.2, 1.2, (n_tris, 1, 2)) + rng.uniform(-1, 1, (n_tris, 3, 2)) * chart).astype(np.float32)
    for j, (name, uv) in enumerate(SPECIAL_UVS.items()):
        UV[k + 3 + j] = uv
        if name == "zero_normal":
            N[k + 3 + j] = 0.0
    images = []
    if textured:
        images = [rng.integers(0, 256, (h, w, comp), dtype=np.uint8) for (h, w, comp) in
                  ((16, 16, 3), (8, 32, 4), (5, 7, 3), (32, 32, 3))]
    mats = []
    for m in range(6):
        em = rng.choice([0.0, 0.0, 2.0], 3) * emission + emission / 10.0
        mt = Material(base_color=tuple(rng.uniform(0, 1, 3)), emission=tuple(em),
                      roughness=float(rng.choice([0.0, 0.001, 0.2, 0.7, 1.5])), metalness=float(rng.choice([0, 0.5, 0.95, 1.0])),
                      normal_map_strength=float(rng.choice([0.0, 0.5, 1.0])), sheen=float(rng.choice([0.0, 0.6])),
                      sheen_tint=float(rng.uniform(0, 1)), anisotropic_strength=float(rng.choice([0.0, 0.7])))
        ti = rng.integers(0, 4, 4)
        if textured and m % 2 == 0:
            mt.texture_albedo, mt.texture_normal = int(ti[0]), int(ti[1])
        if textured and m % 3 == 0:
            mt.texture_metal_roughness, mt.texture_emission = int(ti[2]), int(ti[3])
        mats.append(mt)
    ids = rng.integers(0, len(mats), n_tris)
    P = (P + np.float32(offset)).astype(np.float32)
    cam = camera_from_trs((0.1 + offset, 0.2 + offset, 3.5 + offset))
    return build_scene(P, N, UV, ids, mats, images, cam, 0.9, procedural_background(64, 32), builder=builder)


def special_slots(hs):
    """{name: slot} of the special triangles, found by their UVs in the scene's records."""
    uv = aos_uvs(hs)
    out = {}
    for name, want in SPECIAL_UVS.items():
        hit = np.nonzero((uv == np.array(want, F)).all(axis=(1, 2)))[0]
        assert len(hit) == 1, (name, hit)
        out[name] = int(hit[0])
    return out
