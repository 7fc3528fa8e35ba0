"""The output stage on buffers a test builds: rt_resolve (rt_resolve_kernel), rt_resolve_features and rt_resolve_motion
(rt_features.hip) and rt_untile on fixed-point sums no rendered frame contains, BIT FOR BIT against

  * numpy float64 division followed by astype(float32), as tests/_features.resolve states rt_accum_resolve(_signed),
  * oracle_encode_u8 (rt_encode_u8 of include/rt_math.h),
  * multi_gpu.extract_tiles / multi_gpu.untile, the numpy statements of the two tile layouts.

THE SUMS, per sample count of SAMPLES (1, 3, 7, 16, 1000, 2^31 - 1), by class:
  small     0, 1, 2^32 - 1
  mean_one  samples x 2^32, whose mean is exactly 1, and that sum - 1 and + 1
  inexact   sums at and above 2^53 whose conversion to double rounds: ties to even both ways, below and above a half, up to 2^64 - 1025
  max       2^64 - 1
  steps     for each of the 255 steps of tests/golden/encode_u8_steps.npz the two sums whose mean is exactly first[k] and exactly the
            float below it -- where the sample count is a power of two (1 and 16); with 16 samples every step has its pair
  signed    (position, motion) 0, +-1, 2^63 - 1, -2^63, +-samples x 2^32 and their neighbours, +-(2^53 + 1), ..., and every sum with bit
            63 set reads as another sign when taken as unsigned: a kernel that resolved position or motion unsigned fails on them
and random sums with means in [0, 1.25) (signed: (-1.25, 1.25)) for the rest of the buffer.  Each test asserts that its classes are in
the reference it compares with.  Every output buffer is prefilled with a sentinel and has slack at both ends: what a call must not
write -- texels of chunks another rank owns, tile slots past the rank's last chunk, a plane that was not asked for, the slack --
must come back as the sentinel."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
SAMPLES = [1, 3, 7, 16, 1000, (1 << 31) - 1]
M64 = (1 << 64) - 1
GUARD = 64                                  # elements of slack before and after every output buffer
BYTE, WORD = 0xA5, 0x5A5AA5A5               # the sentinels: of u8 buffers, of f32 buffers (as a bit pattern)


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


# ---- the sums ---------------------------------------------------------------------------------------------------------------------

def _step_pairs(samples):
    """[(k, sum whose mean is first[k], sum whose mean is the float below)] for the steps both sums of which are integers."""
    from tests.test_encode_cpu import steps_fixture
    if samples & (samples - 1):
        return []
    first = steps_fixture()["first"]
    pairs = []
    for k in range(1, 256):
        sums = []
        for bits in (int(first[k]), int(first[k]) - 1):
            man, shift = (bits & 0x7FFFFF) | 0x800000, (bits >> 23) - 150 + 32 + samples.bit_length() - 1
            assert bits >> 23 > 0                                   # (no step is a denormal)
            if shift >= 0:
                sums.append(man << shift)
            elif man % (1 << -shift) == 0:
                sums.append(man >> -shift)
        if len(sums) == 2:
            pairs.append((k, sums[0], sums[1]))
    return pairs


def unsigned_classes(samples):
    """{class: [sums]} for an unsigned channel."""
    one = samples << 32
    classes = dict(small=[0, 1, (1 << 32) - 1], mean_one=[one, one - 1, one + 1],
                   inexact=[(1 << 53) + 1, (1 << 53) + 3, (1 << 54) + 1, (1 << 54) + 3, (1 << 60) + 129, (1 << 63) + 1024,
                            (1 << 63) + 1025, (1 << 63) + 3072, (1 << 64) - 1025],
                   max=[M64])
    classes["steps"] = [s for _, a, b in _step_pairs(samples) for s in (a, b)]
    return classes


def signed_classes(samples):
    """{class: [sums as u64]} for a signed channel."""
    one = samples << 32
    values = [0, 1, -1, (1 << 63) - 1, -(1 << 63), one, -one, one - 1, one + 1, -one + 1, -one - 1,
              (1 << 53) + 1, -((1 << 53) + 1), (1 << 53) + 3, -((1 << 53) + 3), -((1 << 60) + 129), -(1 << 63) + 1024,
              -(1 << 63) + 1025, -(1 << 63) + 3072, (1 << 63) - 1025]
    return dict(signed=[v & M64 for v in values])


def _fill(n, classes, rng, samples, signed):
    """(u64[n] with every class value at a random place and random sums elsewhere, {class: indices}); n too small: the first n values
    of the classes `max`, `mean_one`, `inexact` / `signed`, and no index map."""
    flat = [(name, v) for name, vs in classes.items() for v in vs]
    hi = min(int(1.25 * (samples << 32)), (1 << 63) - 1)
    if signed:
        buf = rng.integers(-hi, hi, n, dtype=np.int64).view(np.uint64)
    else:
        buf = rng.integers(0, int(1.25 * (samples << 32)), n, dtype=np.uint64)
    if n < len(flat):
        order = [v for name in ("max", "mean_one", "inexact", "signed") for v in classes.get(name, [])]
        buf[:] = np.array(order[:n], np.uint64)
        return buf, None
    where = rng.permutation(n)[:len(flat)]
    buf[where] = np.array([v for _, v in flat], np.uint64)
    index = {name: np.array([int(i) for i, (nm, _) in zip(where, flat) if nm == name], np.int64) for name in classes}
    return buf, index


def resolve_unsigned(sums, samples):
    """rt_accum_resolve: numpy float64 division, then astype(float32)."""
    return (np.ascontiguousarray(sums, np.uint64).astype(np.float64) / (float(samples) * 4294967296.0)).astype(F32)


def _check_unsigned_classes(flat_sums, lin, img, index, samples):
    """The classes are in the reference: flat_sums u64[n], lin f32[n], img u8[n] (None: no encode), index from _fill."""
    from tests.test_encode_cpu import steps_fixture
    at = lambda name: index[name]
    assert lin[at("small")].tolist() == [0.0, float(F32(1.0 / (samples * 4294967296.0))), float(F32(((1 << 32) - 1) / (samples << 32)))]
    one = lin[at("mean_one")]
    assert one[0] == 1.0 and one[1] <= 1.0 and one[2] >= 1.0
    for i in at("inexact"):
        v = int(flat_sums[i])
        assert int(float(v)) != v and float(flat_sums[i:i + 1].astype(np.float64)[0]) == float(v)      # rounds, and numpy rounds as Python does
    assert int(flat_sums[at("max")[0]]) == M64 and lin[at("max")[0]] == F32(2.0 ** 64 / (samples * 2.0 ** 32))
    if img is not None:
        assert img[at("small")[0]] == 0 and (img[at("mean_one")] >= 254).all() and img[at("mean_one")[0]] == 255
    pairs = _step_pairs(samples)
    if samples == 16:
        assert len(pairs) == 255
    if samples == 1:
        assert len(pairs) > 200
    if pairs:
        first = steps_fixture()["first"]
        steps = at("steps").reshape(-1, 2)
        ks = np.array([k for k, _, _ in pairs])
        assert np.array_equal(lin[steps[:, 0]].view(np.uint32), first[ks]) and np.array_equal(lin[steps[:, 1]].view(np.uint32), first[ks] - 1)
        if img is not None:
            assert np.array_equal(img[steps[:, 0]], ks.astype(np.uint8)) and np.array_equal(img[steps[:, 1]], (ks - 1).astype(np.uint8))


# ---- guarded device buffers -------------------------------------------------------------------------------------------------------

class Guarded:
    """A device buffer of n elements (u8, or 32-bit words holding f32) filled with the sentinel, with GUARD more at each end."""

    def __init__(self, n, byte):
        import torch
        self.n, self.byte = n, byte
        self.t = torch.full((n + 2 * GUARD,), BYTE if byte else WORD, dtype=torch.uint8 if byte else torch.int32, device="cuda")
        self.ptr = self.t.data_ptr() + GUARD * (1 if byte else 4)

    def get(self, what):
        """The n elements (u8, or the words as u32) after asserting that the slack is untouched."""
        a = self.t.cpu().numpy()
        a = a if self.byte else a.view(np.uint32)
        sentinel = BYTE if self.byte else WORD
        assert (a[:GUARD] == sentinel).all() and (a[GUARD + self.n:] == sentinel).all(), "%s: written outside the buffer" % what
        return a[GUARD:GUARD + self.n]


def _device_sums(sums):
    import torch
    return torch.from_numpy(np.array(sums, np.uint64).view(np.int64)).cuda()


# ---- rt_resolve -------------------------------------------------------------------------------------------------------------------

_frames = {}


def _frame(w, h, samples):
    """(sums u64 (h, w, 3), mean f32 (h, w, 3), image u8 (h, w, 3), index map or None): once per size and sample count, read-only."""
    from tests import _oracle
    key = (w, h, samples)
    if key not in _frames:
        rng = np.random.default_rng(1000 * w + h + samples % 9973)
        flat, index = _fill(w * h * 3, unsigned_classes(samples), rng, samples, False)
        lin = resolve_unsigned(flat, samples)
        img = _oracle.encode_u8(lin)
        if index is not None:
            _check_unsigned_classes(flat, lin, img, index, samples)
        out = (flat.reshape(h, w, 3), lin.reshape(h, w, 3), img.reshape(h, w, 3))
        for a in out:
            a.setflags(write=False)
        _frames[key] = out + (index,)
    return _frames[key]


OUTPUTS = [("tiles",), ("image",), ("linear",), ("tiles", "image", "linear")]


@pytest.mark.parametrize("w,h", [(1, 1), (33, 31), (33, 33), (64, 32)])
def test_resolve_on_synthetic_sums(rt, oracle, w, h):
    """1 x 1: one texel of one chunk; 33 x 31: two chunks, ragged both ways (a chunk one pixel wide, every chunk a row short); 33 x 33:
    four chunks, ragged both ways; 64 x 32: two whole chunks.  World 1, and world 3 with every rank -- at two chunks one rank owns
    none, at 1 x 1 two.  Each output alone and all together, every sample count."""
    import torch
    from raytracing_c_amd import ctypes_abi as abi
    from raytracing_c_amd.multi_gpu import CHUNK, FramePartition, extract_tiles
    for samples in SAMPLES:
        sums, lin, img, _ = _frame(w, h, samples)
        d_sums = _device_sums(sums)
        for world in (1, 3):
            part = FramePartition(w, h, world)
            assert sum(part.n_local(r) for r in range(world)) == part.n_chunks
            for rank in range(world):
                owned = np.zeros((h, w), bool)
                for c in part.chunk_ids(rank):
                    x0, y0 = part.chunk_origin(c)
                    owned[y0:y0 + CHUNK, x0:x0 + CHUNK] = True
                want_img = np.where(owned[..., None], img, np.uint8(BYTE))
                want_lin = np.where(owned[..., None], lin.view(np.uint32), np.uint32(WORD))
                want_tiles = extract_tiles(np.array(img), rank, world)
                want_tiles[part.n_local(rank):] = BYTE                          # slots past the rank's last chunk
                p = abi.RT_Render_Params(width=w, height=h, samples=samples, max_bounces=1, seed=1, rank=rank, world=world)
                for outputs in OUTPUTS:
                    what = (samples, world, rank, outputs)
                    tiles, image, linear = Guarded(want_tiles.size, True), Guarded(img.size, True), Guarded(lin.size, False)
                    torch.cuda.synchronize()
                    rc = rt.lib.rt_resolve(C.byref(p), d_sums.data_ptr(), tiles.ptr if "tiles" in outputs else None,
                                           image.ptr if "image" in outputs else None, linear.ptr if "linear" in outputs else None, None)
                    assert rc == 0, (what, rt.last_error())
                    torch.cuda.synchronize()
                    got_t, got_i, got_l = tiles.get(what), image.get(what), linear.get(what)
                    for name, got, want, sentinel in (("tiles", got_t, want_tiles, BYTE), ("image", got_i, want_img, BYTE),
                                                      ("linear", got_l, want_lin, WORD)):
                        if name in outputs:
                            bad = np.nonzero(got != want.reshape(-1))[0]
                            assert bad.size == 0, (what, name, bad.size, bad[:4].tolist(), got[bad[:4]].tolist(), want.reshape(-1)[bad[:4]].tolist())
                        else:
                            assert (got == sentinel).all(), (what, name, "written though not asked for")


def test_resolve_zeroes_tile_texels_outside_the_image(rt, oracle):
    """(the class check of the tile layout, on the reference) at 33 x 31 chunk 1 has ONE column of the image: 31 x 3 bytes of its tile
    come from the image, every other byte is 0; chunk 0 has a zero last row."""
    from raytracing_c_amd.multi_gpu import extract_tiles
    _, _, img, _ = _frame(33, 31, 16)
    tiles = extract_tiles(np.array(img), 0, 1).reshape(2, 32, 32, 3)
    assert not tiles[0, 31].any() and not tiles[1, :, 1:].any() and not tiles[1, 31].any()
    assert np.array_equal(tiles[1, :31, 0], img[:, 32]) and np.array_equal(tiles[0, :31], img[:, :32])
    assert (img[:, 32] != 0).any() and (img[30] != 0).any()


# ---- rt_resolve_features, rt_resolve_motion ---------------------------------------------------------------------------------------

_feature_cases = {}


def _feature_case(n, samples):
    """(sums u64 (n, 10), motion sums u64 (n, 3), {plane: f32 reference}, motion reference): once per (n, samples), read-only."""
    from tests import _features, _motion
    key = (n, samples)
    if key not in _feature_cases:
        rng = np.random.default_rng(77 * n + samples % 9973)
        u, u_index = _fill(n * 7, unsigned_classes(samples), rng, samples, False)
        s, s_index = _fill(n * 3, signed_classes(samples), rng, samples, True)
        m, m_index = _fill(n * 3, signed_classes(samples), rng, samples, True)
        sums = np.concatenate([u.reshape(n, 7), s.reshape(n, 3)], axis=1)
        want = _features.resolve(sums.reshape(1, n, 10), samples)
        want = {k: np.ascontiguousarray(v.reshape((n,) + v.shape[2:])) for k, v in want.items()}
        want_m = np.ascontiguousarray(_motion.resolve_motion(m.reshape(1, n, 3), samples).reshape(n, 3))
        flat_u = np.concatenate([want["coverage"][:, None], want["albedo"], want["normal"]], axis=1).reshape(-1)
        assert np.array_equal(flat_u.view(np.uint32), resolve_unsigned(u, samples).view(np.uint32))
        if u_index is not None:
            _check_unsigned_classes(u, flat_u, None, u_index, samples)
        for flat, ref, index in ((s, want["position"].reshape(-1), s_index), (m, want_m.reshape(-1), m_index)):
            # the signed classes are in the reference: every sum with bit 63 set gives a negative mean, another than its unsigned reading
            negative = flat >= np.uint64(1 << 63)
            assert (ref[negative] < 0).all() and (ref[~negative] >= 0).all()
            assert (resolve_unsigned(flat, samples)[negative] > 0).all()
            if index is not None:
                at = index["signed"]
                assert negative[at].sum() >= 9 and (~negative[at]).sum() >= 9 and negative.sum() > n
                assert ref[at[:5]].tolist() == [0.0, float(F32(2.0 ** -32 / samples)), float(F32(-2.0 ** -32 / samples)),
                                                float(F32(2.0 ** 31 / samples)), float(F32(-2.0 ** 31 / samples))]
                assert ref[at[5]] == 1.0 and ref[at[6]] == -1.0
        out = (sums, m.reshape(n, 3), want, want_m)
        for a in (sums, out[1], want_m, *want.values()):
            a.setflags(write=False)
        _feature_cases[key] = out
    return _feature_cases[key]


PLANES = ("coverage", "albedo", "normal", "position")


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_resolve_features_and_motion_on_synthetic_sums(rt, n):
    """n pixels around the launch's block of 256: one thread, a block one short, a whole block, a second block of one thread.  Every
    plane NULL in turn and all four present; the plane left out stays the sentinel, as does the slack around the others."""
    import torch
    from raytracing_c_amd import ctypes_abi as abi
    for samples in SAMPLES:
        sums, msums, want, want_m = _feature_case(n, samples)
        d_sums, d_msums = _device_sums(sums), _device_sums(msums)
        p = abi.RT_Render_Params(width=n, height=1, samples=samples, max_bounces=1, seed=1, rank=0, world=1)
        for left_out in (None,) + PLANES:
            what = (samples, left_out)
            bufs = {k: Guarded(want[k].size, False) for k in PLANES}
            torch.cuda.synchronize()
            rc = rt.lib.rt_resolve_features(C.byref(p), d_sums.data_ptr(), *[None if k == left_out else bufs[k].ptr for k in PLANES], None)
            assert rc == 0, (what, rt.last_error())
            torch.cuda.synchronize()
            for k in PLANES:
                got = bufs[k].get((what, k))
                if k == left_out:
                    assert (got == WORD).all(), (what, k)
                    continue
                ref = want[k].reshape(-1).view(np.uint32)
                bad = np.nonzero(got != ref)[0]
                assert bad.size == 0, (what, k, bad.size, bad[:4].tolist(), got[bad[:4]].tolist(), ref[bad[:4]].tolist())
        motion = Guarded(n * 3, False)
        torch.cuda.synchronize()
        assert rt.lib.rt_resolve_motion(C.byref(p), d_msums.data_ptr(), motion.ptr, None) == 0, (samples, rt.last_error())
        torch.cuda.synchronize()
        got, ref = motion.get((samples, "motion")), want_m.reshape(-1).view(np.uint32)
        bad = np.nonzero(got != ref)[0]
        assert bad.size == 0, (samples, "motion", bad.size, bad[:4].tolist(), got[bad[:4]].tolist(), ref[bad[:4]].tolist())


# ---- rt_untile --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(33, 31), (100, 70)])
@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_untile_on_synthetic_tiles(rt, w, h, world):
    """Gathered tiles with random bytes per (chunk, texel) -- a texel read from another chunk, slot or rank matches with probability
    1 / 256 per byte --, garbage in the texels outside the image and in the slots past a rank's last chunk (world 5 at 33 x 31: three
    ranks own no chunk), into a sentinel-filled image with slack at both ends."""
    import torch
    from raytracing_c_amd.multi_gpu import FramePartition, extract_tiles, untile
    rng = np.random.default_rng(31 * w + h + world)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    part = FramePartition(w, h, world)
    clean = np.stack([extract_tiles(img, rank, world) for rank in range(world)])
    inside = np.stack([extract_tiles(np.full_like(img, 1), rank, world) for rank in range(world)]) != 0
    garbage = rng.integers(1, 256, clean.shape, dtype=np.uint8)
    all_tiles = np.where(inside, clean, garbage)
    assert all_tiles.shape == (world, part.max_local, 3072) and (~inside).sum() >= 3072 - 31 * 3
    want = untile(all_tiles, w, h, world)
    assert np.array_equal(want, img)
    dst = Guarded(img.size, True)
    d_tiles = torch.from_numpy(all_tiles).cuda()
    torch.cuda.synchronize()
    assert rt.lib.rt_untile(w, h, world, d_tiles.data_ptr(), dst.ptr, None) == 0, rt.last_error()
    torch.cuda.synchronize()
    got = dst.get((w, h, world))
    bad = np.nonzero(got != want.reshape(-1))[0]
    assert bad.size == 0, (bad.size, bad[:4].tolist())
