"""Denoiser (reference denoiser.c:51-153): oracle pinned by an independent numpy
statement of the reference text; HIP kernel bit-exact against the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

from raytracing_c_amd.scene import make_image

F = np.float32


def np_denoise(src, before_equal=False, windows=None):
    """Literal restatement of denoiser.c:51-129 for (H, W, 3) uint8.  `before_equal` inserts before the first entry that is
    brighter OR EQUAL instead: the order an unstable sort may leave -- what a tie image must be able to tell apart.
    `windows`, a list, receives one bool per pixel: sorted slots 3-5 hold a tie between unequal colours at the median."""
    h, w, _ = src.shape
    dst = np.zeros_like(src)
    wts = np.array([0.2126, 0.7152, 0.0722], F)
    for y in range(h):
        for x in range(w):
            colors = []
            original = None
            for yo in (-1, 0, 1):
                for xo in (-1, 0, 1):
                    xx, yy = min(max(x + xo, 0), w - 1), min(max(y + yo, 0), h - 1)
                    rgb = (src[yy, xx].astype(F) / F(255.999)).astype(F)
                    lum = F(F(F(rgb[0] * wts[0]) + F(rgb[1] * wts[1])) + F(rgb[2] * wts[2]))
                    c = (rgb, lum)
                    if xo == 0 and yo == 0:
                        original = c
                    for i, (_, l2) in enumerate(colors):
                        if l2 > lum or (before_equal and l2 == lum):
                            colors.insert(i, c)
                            break
                    else:
                        colors.append(c)
            median = colors[4]
            if windows is not None:
                windows.append(any(colors[i][1] == colors[4][1] and (colors[i][0] != colors[4][0]).any() for i in (3, 5)))
            mean = F(0)
            for i in range(1, 8):
                mean = F(mean + colors[i][1])
            mean = F(mean / F(7))
            noisiness = abs(F(median[1] - mean))
            diff = F(abs(F(median[1] - original[1])) - F(noisiness * F(5)))
            diff = F(min(max(diff, F(0)), F(0.0125)) / F(0.0125))
            out = (original[0] * F(F(1) - diff) + median[0] * diff).astype(F)
            dst[y, x] = (out * F(255.999)).astype(np.uint8)
    return dst


def _oracle_denoise(oracle, src):
    dst = np.zeros_like(src)
    si, sk = make_image(src)
    di, dk = make_image(dst)
    oracle.oracle_denoise_image(C.byref(si), C.byref(di))
    return dk


def test_oracle_denoiser_matches_reference_text(oracle):
    rng = np.random.default_rng(1)
    for shape in ((7, 9, 3), (1, 5, 3), (12, 12, 3)):
        src = rng.integers(0, 256, shape, dtype=np.uint8)
        src[shape[0] // 2, shape[1] // 2] = (255, 255, 255)           # a firefly
        assert np.array_equal(_oracle_denoise(oracle, src), np_denoise(src)), shape
    flat = np.full((6, 6, 3), 128, np.uint8)          # v/255.999*255.999 truncated: 128 or 127, never more
    assert np.abs(_oracle_denoise(oracle, flat).astype(int) - 128).max() <= 1


def test_denoiser_removes_a_firefly(oracle):
    src = np.full((9, 9, 3), 60, np.uint8)
    src[4, 4] = (250, 250, 250)
    out = _oracle_denoise(oracle, src)
    assert out[4, 4].max() < 80


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(64, 64, 3), (45, 71, 3), (33, 31, 4), (1, 1, 3), (2, 130, 3), (40, 100, 3), (21, 96, 3)])
def test_gpu_denoiser_bit_exact(oracle, shape):
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, shape, dtype=np.uint8)
    src[::7, ::5] = 255
    want = _oracle_denoise(oracle, src)
    got = np.zeros_like(src)
    si, sk = make_image(src)
    di, dk = make_image(got)
    rt.lib.rt_clear_error()
    rt.lib.denoise_image(C.byref(si), C.byref(di), 4)
    assert rt.last_error() == ""
    assert np.array_equal(dk[..., :3], want[..., :3])


@pytest.mark.gpu
def test_gpu_denoiser_on_a_rendered_frame(oracle):
    """driver.c:827-837: -D runs the denoiser on the finished u8 frame; device-pointer form on the GPU image."""
    import torch
    import raytracing_c_amd as rt
    from raytracing_c_amd.configs import load_config
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    hs, _ = load_config("helmet")
    img = rt.render_frame(hs, 192, 108, 2, 8)["image"]
    want = _oracle_denoise(oracle, img)
    src = torch.from_numpy(img).cuda()
    dst = torch.zeros_like(src)
    assert rt.lib.rt_denoise(192, 108, src.data_ptr(), dst.data_ptr(), None) == 0, rt.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), want)
    assert (want != img).mean() > 0.01        # 2 spp is noisy: the filter does change pixels


# ---------------------------------------------------------------------------------------------------------------------
# luminance ties between DIFFERENT colours: the only inputs on which the reference's stable insertion differs from an
# unstable sort.  Random images and rendered frames hold essentially none.

def _luminance_of_all_colours():
    """the kernel's stepwise fp32 luminance of all 2^24 u8 colours, indexed [r, g, b]"""
    v = (np.arange(256, dtype=F) / F(255.999)).astype(F)
    r, g, b = (v * F(0.2126)).astype(F), (v * F(0.7152)).astype(F), (v * F(0.0722)).astype(F)
    lum = ((r[:, None, None] + g[None, :, None]).astype(F) + b[None, None, :]).astype(F)
    assert lum.dtype == F
    return lum


@functools.lru_cache(maxsize=None)
def tie_palettes():
    """Four groups of four different colours, equal luminance within a group: the colours of 2^24 that tie with a seed
    colour, taken as far apart as the group allows.  The group luminances differ by more than DENOISING_THRESHOLD in three
    cases and by less in one, so that the blend weight takes 1 and values in between."""
    lum = _luminance_of_all_colours()
    groups = []
    for seed in ((96, 90, 80), (100, 92, 84), (200, 160, 40), (20, 30, 140)):
        r, g, b = np.nonzero(lum == lum[seed])
        same = np.stack([r, g, b], axis=1).astype(np.uint8)
        assert len(same) >= 3, (seed, len(same))
        order = np.argsort(same[:, 0].astype(int) - same[:, 2].astype(int))           # from blue-ish to red-ish
        pick = same[order[np.linspace(0, len(same) - 1, min(4, len(same))).astype(int)]]
        assert len(np.unique(pick, axis=0)) == len(pick) >= 3
        groups.append(pick)
    return groups


def tie_image(h, w, seed=3):
    """Most pixels draw from the first group; one in three from the others: fireflies whose 3x3 window is a run of ties."""
    groups = tie_palettes()
    rng = np.random.default_rng(seed)
    which = rng.choice(len(groups), (h, w), p=[0.67, 0.13, 0.1, 0.1])
    col = rng.integers(0, 1 << 30, (h, w))
    img = np.zeros((h, w, 3), np.uint8)
    for k, g in enumerate(groups):
        img[which == k] = g[col[which == k] % len(g)]
    return img


TIE_SHAPES = [(64, 64, 3), (45, 71, 3)]


@pytest.mark.parametrize("shape", TIE_SHAPES)
def test_oracle_denoiser_is_stable_on_luminance_ties(oracle, shape):
    src = tie_image(*shape[:2])
    lum = _luminance_of_all_colours()
    for g in tie_palettes():
        assert len({lum[tuple(c)].tobytes() for c in g}) == 1 and len(g) >= 3
    windows = []
    want = np_denoise(src, windows=windows)
    share = float(np.mean(windows))
    print(f"\ntie image {shape}: windows with a tie of unequal colours at the median: {share:.3f}")
    assert share >= 0.2
    assert np.array_equal(_oracle_denoise(oracle, src), want)
    if shape == TIE_SHAPES[0]:          # the image tells a stable sort from an unstable one, and the filter does act on it
        unstable = np_denoise(src, before_equal=True)
        changed = float((unstable != want).any(axis=-1).mean())
        print(f"tie image {shape}: pixels an unstable order would change: {changed:.3f}")
        assert changed > 0.05
        assert (want != src).any(axis=-1).mean() > 0.05


@pytest.mark.gpu
@pytest.mark.parametrize("shape", TIE_SHAPES)
def test_gpu_denoiser_is_stable_on_luminance_ties(oracle, shape):
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    src = tie_image(*shape[:2])
    want = _oracle_denoise(oracle, src)
    assert (want != src).any(axis=-1).mean() > 0.05
    si, sk = make_image(src)
    di, dk = make_image(np.zeros_like(src))
    rt.lib.rt_clear_error()
    rt.lib.denoise_image(C.byref(si), C.byref(di), 4)
    assert rt.last_error() == ""
    assert np.array_equal(dk, want)


# ---------------------------------------------------------------------------------------------------------------------
# layout: strides, component counts, alignment of the destination

# W, H, src components, src stride, dst components, dst stride
LAYOUTS = [(50, 20, 3, 57, 3, 61),        # src stride != dst stride, both > width
           (64, 17, 3, 64, 3, 65),        # full tiles in x, rows of 195 bytes: the whole-dword store must switch itself off
           (64, 17, 3, 66, 3, 68),        # rows of 204 bytes: it stays on, and must leave the 4 texels of padding alone
           (45, 11, 4, 45, 3, 45),        # RGBA -> RGB
           (45, 11, 3, 49, 4, 47),        # RGB -> RGBA: alpha unchanged
           (64, 9, 4, 64, 4, 64),
           (37, 10, 2, 39, 2, 38),        # two components: the third reads as 0 and is not stored (denoiser.c:23,35)
           (64, 9, 2, 64, 3, 64),
           (33, 9, 1, 33, 1, 36)]


def _layout_pair(W, H, sc, ss, dc, ds):
    from tests._lightmap import padded_image
    rng = np.random.default_rng(W * 1000 + H)
    si, sk = padded_image(H, ss, sc, ss, 0)
    sk[...] = rng.integers(0, 256, sk.shape, dtype=np.uint8)           # the padding holds noise: it must not be read
    sk[::5, ::7] = 255
    si.width = W
    di, dk = padded_image(H, W, dc, ds, 99)
    return si, sk, di, dk


@pytest.mark.parametrize("layout", LAYOUTS[:2] + LAYOUTS[3:5] + LAYOUTS[6:])
def test_oracle_denoiser_layouts_match_reference_text(oracle, layout):
    """The oracle reads and writes through stride and components like denoiser.c:20-41: missing source channels are 0,
    min(components, 3) channels are stored, nothing else is touched."""
    W, H, sc, ss, dc, ds = layout
    W, H = min(W, 13), min(H, 6)                       # np_denoise is a Python loop
    si, sk, di, dk = _layout_pair(W, H, sc, ss, dc, ds)
    oracle.oracle_denoise_image(C.byref(si), C.byref(di))
    rgb = np.zeros((H, W, 3), np.uint8)
    rgb[..., :min(sc, 3)] = sk[:, :W, :min(sc, 3)]
    want = np.full_like(dk, 99)
    want[:, :W, :min(dc, 3)] = np_denoise(rgb)[..., :min(dc, 3)]
    assert np.array_equal(dk, want)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gpu_denoiser_layouts(oracle, layout):
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    W, H, sc, ss, dc, ds = layout
    si, sk, di, want = _layout_pair(*layout)
    oracle.oracle_denoise_image(C.byref(si), C.byref(di))
    assert (want[:, W:] == 99).all() and (want[..., 3:] == 99).all() and (want[:, :W, :min(dc, 3)] != 99).any()
    si, sk, di, got = _layout_pair(*layout)
    rt.lib.rt_clear_error()
    rt.lib.denoise_image(C.byref(si), C.byref(di), 4)
    assert rt.last_error() == ""
    assert np.array_equal(got, want)                   # the whole backing buffer: padding and alpha included


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [1, 2, 3, 4])
def test_gpu_denoiser_into_an_unaligned_device_destination(oracle, offset):
    """rt_denoise on device pointers: a destination that is not 4-byte aligned (only this entry point can produce one) at
    a width of whole tiles.  The bytes before and after the image are not the kernel's to write."""
    import torch
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    W, H = 64, 17
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[::4, ::9] = 255
    want = _oracle_denoise(oracle, img)
    src = torch.from_numpy(img).cuda()
    n = W * H * 3
    dst = torch.full((n + 16,), 99, dtype=torch.uint8, device="cuda")
    assert dst.data_ptr() % 4 == 0
    assert rt.lib.rt_denoise(W, H, src.data_ptr(), dst.data_ptr() + offset, None) == 0, rt.last_error()
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert (out[:offset] == 99).all() and (out[offset + n:] == 99).all()
    assert np.array_equal(out[offset:offset + n].reshape(H, W, 3), want)
