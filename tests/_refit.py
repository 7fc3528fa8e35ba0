"""What tests/test_refit_cpu.py and tests/test_gpu_refit.py share: triangle soups built from arrays the test keeps, the bytes of a
Scene, deformations."""
import ctypes as C

import numpy as np

SHAPES = [1, 8, 9, 64, 65, 513, 4097]      # depth 0, one node, the 64 / 65 boundary, early-leaf chains, a mostly empty depth-4 tree
BUILDERS = ["reference", "sah"]


class Soup:
    """A soup like tests.test_gpu_random_scenes.make_scene's, with byte-identical duplicates (positions, normals, uvs AND material),
    a zero-area triangle and axis-aligned quads; the arrays stay with the test."""

    def __init__(self, seed, n_tris):
        from raytracing_c_amd.background import procedural_background
        from raytracing_c_amd.loaders import camera_from_trs
        from raytracing_c_amd.scene import Material
        rng = np.random.default_rng(seed)
        n = n_tris
        c = rng.uniform(-1, 1, (n, 1, 3))
        P = (c + rng.normal(size=(n, 3, 3)) * rng.choice([0.05, 0.3, 0.8], (n, 1, 1))).astype(np.float32)
        self.zero_area = min(1, n - 1)
        P[self.zero_area] = P[self.zero_area][[0, 0, 0]]
        if n > 12:
            P[3] = [[0, -1, -1], [0, 1, -1], [0, 1, 1]]
            P[4] = [[-1, 0, -1], [1, 0, -1], [1, 0, 1]]
        e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        fn = np.cross(e1, e2)
        fn = fn / np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-20)
        N = (fn[:, None, :] + rng.normal(size=(n, 3, 3)) * 0.2).astype(np.float32)
        UV = rng.uniform(-1.5, 2.5, (n, 3, 2)).astype(np.float32)
        self.images = [rng.integers(0, 256, (h, w, comp), dtype=np.uint8) for (h, w, comp) in ((16, 16, 3), (8, 32, 4), (5, 7, 3))]
        self.materials = []
        for m in range(4):
            mt = Material(base_color=tuple(rng.uniform(0, 1, 3)), emission=tuple(rng.choice([0.0, 0.0, 2.0], 3)),
                          roughness=float(rng.choice([0.0, 0.2, 0.7])), metalness=float(rng.choice([0, 0.5, 1.0])),
                          normal_map_strength=float(rng.choice([0.0, 1.0])))
            if m % 2 == 0:
                mt.texture_albedo = int(rng.integers(0, 3))
                mt.texture_normal = int(rng.integers(0, 3))
            self.materials.append(mt)
        ids = rng.integers(0, len(self.materials), n)
        self.n_duplicates = n // 10 if n >= 20 else (2 if n >= 8 else 0)
        k = self.n_duplicates
        self.copies = [(n - k + i, i) for i in range(k)]      # (index of the copy, index of its original)
        if n >= 64:                                 # a triple: the k-th of three goes to the k-th slot
            self.copies.append((n - k - 1, 0))
        for arr in (P, N, UV, ids):
            self.copy_duplicates(arr)
        self.P, self.N, self.UV, self.ids = P, N, UV, ids
        self.camera = camera_from_trs((0.1, 0.2, 3.5))
        self.background = procedural_background(64, 32)
        self.n = n

    def build(self, builder="reference", P=None, N=None, UV=None):
        from raytracing_c_amd.scene import build_scene
        return build_scene(self.P if P is None else P, self.N if N is None else N, self.UV if UV is None else UV, self.ids,
                           self.materials, self.images, self.camera, 0.9, self.background, builder=builder)

    def copy_duplicates(self, arr):
        """makes the copies equal their originals again, in place"""
        for dst, src in self.copies:
            arr[dst] = arr[src]
        return arr

    def moved(self, seed=99, amount=0.05):
        """positions, normals, uvs after a per-vertex displacement of about `amount`"""
        rng = np.random.default_rng(seed)
        P = (self.P + rng.normal(size=self.P.shape) * amount).astype(np.float32)
        N = (self.N + rng.normal(size=self.N.shape) * 0.1).astype(np.float32)
        UV = (self.UV + rng.normal(size=self.UV.shape) * 0.1).astype(np.float32)
        return P, N, UV


_SOUPS = {}


def soup(n_tris):
    """One soup per size, shared by every test that needs it and never changed (tests copy what they edit)."""
    if n_tris not in _SOUPS:
        _SOUPS[n_tris] = Soup(1000 + n_tris, n_tris)
    return _SOUPS[n_tris]


def scene_bytes(hs):
    from tests.test_gpu_builder import _scene_bytes
    return _scene_bytes(hs)


def raw_bytes(hs):
    """(node bytes, triangle block bytes) as they are, Shader pointers included: for a scene compared with ITSELF before and after"""
    n_nodes = int(hs.scene.bvh.nodes.len)
    n = int(hs.scene.triangles.len)
    return (bytes(C.string_at(hs.scene.bvh.nodes.data, n_nodes * 192)) if n_nodes else b"",
            bytes(C.string_at(C.cast(hs.scene.triangles.x[0], C.c_void_p), n * 148)))


def slot_views(hs):
    """(coords (len, 9) in the order x0 x1 x2 y0 y1 y2 z0 z1 z2, aos records (len, 112) u8, populated (len,) bool): copies"""
    n = int(hs.scene.triangles.len)
    raw = np.frombuffer(C.string_at(C.cast(hs.scene.triangles.x[0], C.c_void_p), n * 148), np.uint8).copy()
    coords = raw[:n * 36].view(np.float32).reshape(9, n).T.copy()
    aos = raw[n * 36:].reshape(n, 112).copy()
    populated = aos[:, 104:112].copy().view(np.uint64).reshape(n) != 0
    return coords, aos, populated


def call_refit_on(lib, hs, tri, smap, which="scene_refit_gpu"):
    """the C call of library `lib` on an explicit Triangle array and map; returns its result"""
    from raytracing_c_amd import ctypes_abi as abi
    smap = np.ascontiguousarray(smap, np.int32)
    return getattr(lib, which)(C.byref(hs.scene), abi.Triangle_Slice(tri.ctypes.data, len(tri)), smap.ctypes.data)


def call_refit(hs, tri, smap, which="scene_refit"):
    import raytracing_c_amd as rt
    return call_refit_on(rt.lib, hs, tri, smap, which)
