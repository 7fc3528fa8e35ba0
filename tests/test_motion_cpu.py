"""The motion tests' own instruments, on the CPU (tests/_motion.py): the oracle chain that yields (triangle, u, v) of every feature
hit reproduces tests/_features.expected's coverage and position sums on every scene the GPU tests use; an unmoved scene has motion
0; the restated accumulation with zero motion IS tests/_temporal.accumulate (and tests/_variance.accumulate_moments); the GPU
inputs hold every class of pixel among the pixels that moved; and a restatement that ignores the motion, or measures the plane
distance from W_p, is told apart from the right one."""
import numpy as np
import pytest

F32 = np.float32
SHAPE = (21, 13, 5, 4)              # w, h, samples, max_bounces: what tests/test_gpu_motion_features.py renders


def _soup_scenes():
    """(name, host scene refitted on the CPU to moved(amount=0.05), kept tiles, current tiles) of the GPU tests' soups"""
    from tests import _motion as M, _refit
    for n in (65, 513):
        for builder in _refit.BUILDERS:
            soup = _refit.soup(n)
            hs = soup.build(builder)
            kept = M.leaf_tiles(hs)
            P, N, UV = soup.moved(amount=0.05)
            hs.refit(P, N, UV, device="cpu")
            yield f"soup{n}-{builder}", hs, kept, M.leaf_tiles(hs)


def _passthrough():
    from tests import _motion as M
    hs, P = M.displaced_passthrough()
    kept = M.leaf_tiles(hs)
    hs.refit(P, device="cpu")
    return "passthrough", hs, kept, M.leaf_tiles(hs)


@pytest.fixture(scope="module")
def scenes(oracle):
    return list(_soup_scenes()) + [_passthrough()]


def test_leaf_tiles_restate_the_upload(scenes):
    """a - a = 0, edges from the coordinates: rows 0, 3, 6 are vertex a, and the moved scenes' tiles differ from the kept ones"""
    from tests import _refit
    for name, hs, kept, cur in scenes:
        coords, _, populated = _refit.slot_views(hs)
        assert cur.shape == (len(coords) // 8, 9, 8) and cur.dtype == F32
        assert np.array_equal(cur[:, 0].ravel(), coords[:, 0]) and np.array_equal(cur[:, 6].ravel(), coords[:, 6])
        assert np.array_equal(cur[:, 4].ravel(), coords[:, 4] - coords[:, 3])
        assert (kept != cur).any(), name


def test_chain_equals_the_feature_oracle_and_the_motion_is_there(scenes):
    from tests import _features, _motion as M
    w, h, s, b = SHAPE
    for name, hs, kept, cur in scenes:
        ch = M.chain(hs, w, h, s, b)
        want = _features.expected_cached("motion-" + name, hs, w, h, s, b)["sums"]
        cov, pos = M.chain_sums(ch)
        assert np.array_equal(cov, want[..., 0]), name
        assert np.array_equal(pos, want[..., 7:10]), name
        covered = want[..., 0] != 0
        assert covered.sum() >= 40, (name, int(covered.sum()))
        # unmoved against itself: +0, every sum 0
        assert not M.motion_of(ch, cur, cur).view(np.uint32).any(), name
        assert not M.expected_motion(ch, cur, cur).any(), name
        sums = M.expected_motion(ch, cur, kept)
        moving = (sums != 0).any(axis=2)
        assert not moving[~covered].any(), name
        assert moving.sum() * 4 >= covered.sum(), (name, int(moving.sum()), int(covered.sum()))
        mot = M.resolve_motion(sums, s)
        assert (mot < 0).any() and (mot > 0).any(), name


def test_passthrough_and_motion_meet(scenes):
    """behind one and behind two back faces there are feature hits that moved; at max_bounces 1 there are none"""
    from tests import _motion as M
    w, h, s, _ = SHAPE
    name, hs, kept, cur = scenes[-1]
    moving = {b: (M.expected_motion(M.chain(hs, w, h, s, b), cur, kept) != 0).any(axis=2) for b in (1, 2, 3)}
    assert not moving[1].any()
    assert (moving[2]).sum() >= 10 and (moving[3] & ~moving[2]).sum() >= 10


def test_a_sample_range_adds_up(scenes):
    from tests import _motion as M
    w, h, s, b = SHAPE
    name, hs, kept, cur = scenes[0]
    whole = M.expected_motion(M.chain(hs, w, h, s, b), cur, kept)
    parts = [M.expected_motion(M.chain(hs, w, h, s, b, r), cur, kept) for r in ((0, 2), (2, 3))]
    assert np.array_equal(whole, parts[0] + parts[1]) and parts[0].any() and parts[1].any()


SIZES = [(67, 35), (33, 9)]

def _kw():
    from tests import _motion as M
    return M.MOTION_KW



def _args(P):
    return [P[k] for k in ("color", "coverage", "albedo", "normal", "position")]


@pytest.mark.parametrize("w,h", SIZES)
def test_zero_motion_is_the_accumulation(w, h):
    from tests import _motion as M, _temporal as T, _variance as V, test_gpu_temporal as G
    P, hist, _ = M.motion_case(w, h)
    zero = np.zeros((h, w, 3), F32)
    mom = np.random.default_rng(w).random((h, w, 2)).astype(F32)
    for demodulate in (True, False):
        for history in (hist, None):
            want = T.accumulate(*_args(P), G.CAM_NEW, G.CAM_OLD, history, demodulate=demodulate, **_kw())
            got = M.accumulate_motion(*_args(P), zero, G.CAM_NEW, G.CAM_OLD, history, demodulate=demodulate, **_kw())
            assert got["out"].tobytes() == want["out"].tobytes() and got["length"].tobytes() == want["length"].tobytes()
            assert np.array_equal(got["cls"], want["cls"])
            for k in want["history"]:
                assert got["history"][k].tobytes() == want["history"][k].tobytes(), k
            m_in = None if history is None else mom
            want = V.accumulate_moments(*_args(P), G.CAM_NEW, G.CAM_OLD, history, m_in, demodulate=demodulate, **_kw())
            got = M.accumulate_motion(*_args(P), zero, G.CAM_NEW, G.CAM_OLD, history, m_in, with_moments=True, demodulate=demodulate, **_kw())
            assert got["moments"].tobytes() == want["moments"].tobytes() and got["out"].tobytes() == want["out"].tobytes()


@pytest.mark.parametrize("w,h", SIZES)
def test_every_class_occurs_among_the_pixels_that_moved(w, h):
    from tests import _motion as M, _temporal as T, test_gpu_temporal as G
    P, hist, motion = M.motion_case(w, h)
    moved = (motion != 0).any(axis=2)
    right = M.accumulate_motion(*_args(P), motion, G.CAM_NEW, G.CAM_OLD, hist, **_kw())
    counts = {T.CLASS_NAMES[k]: int(((right["cls"] == k) & moved).sum()) for k in range(9)}
    print(counts)
    for k in range(9):
        if k != T.NO_HISTORY:
            assert counts[T.CLASS_NAMES[k]] >= 20, counts
    # "no history given" is a call's class, not a pixel's: the same planes without a history
    first = M.accumulate_motion(*_args(P), motion, G.CAM_NEW, None, None, **_kw())["cls"]
    assert ((first == T.NO_HISTORY) & moved).sum() >= 20 and set(np.unique(first)) == {T.SKY, T.NO_HISTORY}
    # the wrong restatements are told apart
    ignoring = M.accumulate_motion(*_args(P), np.zeros_like(motion), G.CAM_NEW, G.CAM_OLD, hist, **_kw())
    from_w = M.accumulate_motion(*_args(P), motion, G.CAM_NEW, G.CAM_OLD, hist, plane_from_w=True, **_kw())
    for what, wrong in (("ignores the motion", ignoring), ("plane test from W_p", from_w)):
        differ = (wrong["out"].view(np.uint32) != right["out"].view(np.uint32)).any(axis=2)
        assert differ.sum() >= 100, (what, int(differ.sum()))
    assert (right["history"]["position"].tobytes() == ignoring["history"]["position"].tobytes())      # the history keeps W_p
