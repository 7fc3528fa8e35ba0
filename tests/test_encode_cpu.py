"""rt_encode_u8 (include/rt_math.h) -- mean -> clamp -> sRGB -> byte, the last step of every image -- on the CPU: its step table
over every float of [0, 1] against the table of the function BEFORE its clamp was rewritten for NaN (tests/golden/
encode_u8_steps.npz, one table per numeric contract), what it does outside [0, 1], and the numpy restatement the post-pass tests
use (tests/_guided.encode_u8).

A step table is first[k] = the lowest bit pattern in [0, 0x3F800000] that encodes to k.  With no descent in ascending pattern order
and all 256 bytes present, the table IS the function on [0, 1]: two functions with equal tables, both monotone, agree on every
one of the 1 065 353 217 patterns.  tests/test_gpu_parity.py compares the device's table with the oracle's in the same way."""
import os
import time

import numpy as np
import pytest

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode_u8_steps.npz")
ONE = 0x3F800000


def _f(bits):
    return np.asarray(bits, np.uint32).view(F32)


def steps_fixture():
    """The step tables of the encode before the NaN rule: "first" (contract v3, the library's), "first_v1", "first_v2"; 256 u32 each,
    made by a single-threaded sweep of that header with gcc and -ffp-contract=off."""
    with np.load(GOLDEN) as z:
        return {k: z[k].copy() for k in z.files}


_sweeps = {}


def oracle_steps(contract="v3"):
    """(first, descents, bytes present, seconds) of liboracle[_v1|_v2].so -- swept once per process, shared."""
    from tests import _oracle
    if contract not in _sweeps:
        lib = None if contract == "v3" else _oracle.load(os.path.join(_oracle.ORACLE_DIR, "liboracle_%s.so" % contract))
        t0 = time.perf_counter()
        first, descents, seen = _oracle.encode_steps(8, lib=lib)
        first.setflags(write=False)
        _sweeps[contract] = (first, descents, seen, time.perf_counter() - t0)
    return _sweeps[contract]


def test_the_fixture_is_a_step_table():
    fx = steps_fixture()
    assert sorted(fx) == ["first", "first_v1", "first_v2"]
    for k, first in fx.items():
        assert first.dtype == np.uint32 and first.shape == (256,), k
        assert first[0] == 0 and (np.diff(first.astype(np.int64)) > 0).all() and first[255] < ONE, k
    first = fx["first"]
    assert (first[1], first[10], first[11], first[255]) == (0x399E83BA, 0x3B4624A8, 0x3B5A6AB5, 0x3F7DBBBA)
    # contract v2 differs from v3 in the sRGB DECODE only; v1 has no fused multiply-add in the encode's 1.055 * pow - 0.055
    # (which is why there is a table per contract: v1's steps sit elsewhere)
    assert np.array_equal(first, fx["first_v2"]) and not np.array_equal(first, fx["first_v1"])


@pytest.mark.parametrize("contract", ["v3", "v1", "v2"])
def test_the_oracle_still_produces_the_fixture(oracle, contract):
    """oracle_encode_steps over all of [0, 0x3F800000], on 8 threads: the table the header gave before the NaN rule, no descent, all
    256 bytes -- so every float of [0, 1] kept its byte, under each contract.  Measured: 0.66 s for one sweep on 8 threads (4.3 s on
    one) of the machine this was written on; the bound below is what keeps it from growing unnoticed."""
    first, descents, seen, seconds = oracle_steps(contract)
    print("oracle_encode_steps, contract %s: %.2f s" % (contract, seconds))
    want = steps_fixture()["first" if contract == "v3" else "first_" + contract]
    bad = np.nonzero(first != want)[0]
    assert bad.size == 0, [(int(k), hex(int(first[k])), hex(int(want[k]))) for k in bad[:4]]
    assert descents == 0 and seen == 256
    assert seconds < 10.0


def test_the_table_is_the_function_at_its_steps(oracle):
    """(of the table's meaning, through the one-value entry point) first[k] encodes to k, the float below it to k - 1."""
    from tests import _oracle
    first = steps_fixture()["first"]
    assert np.array_equal(_oracle.encode_u8(_f(first)), np.arange(256, dtype=np.uint8))
    assert np.array_equal(_oracle.encode_u8(_f(first[1:] - np.uint32(1))), np.arange(255, dtype=np.uint8))
    assert oracle.oracle_encode_u8(float(_f(first[200]))) == 200


def _outside_patterns():
    """Every exponent of both signs with a few mantissas, the neighbours of 1.0, infinities, NaNs quiet and signalling, of both signs."""
    man = np.array([0, 1, 0x400000, 0x7FFFFF], np.uint32)
    finite = (np.arange(0, 256, dtype=np.uint32)[:, None] << np.uint32(23)) | man[None, :]
    pos = finite.reshape(-1)
    return pos, pos | np.uint32(0x80000000)


def test_outside_the_unit_interval_and_nan(oracle):
    """Above 1.0 up to +inf: 255.  Negative, -0 and -inf included: 0.  NaN, any sign and payload: 0 -- deviation D11 (oracle/oracle.h);
    before it the conversion of a negative float to uint8_t decided, which C leaves undefined (242 from gcc on x86-64)."""
    from tests import _oracle
    pos, neg = _outside_patterns()
    nan = lambda b: (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    above = pos[(pos > ONE) & ~nan(pos)]
    assert above.size > 400 and 0x7F800000 in above and ONE + 1 in above
    assert (_oracle.encode_u8(_f(above)) == 255).all()
    negative = neg[~nan(neg)]
    assert 0x80000000 in negative and 0xFF800000 in negative and 0x80000001 in negative
    assert (_oracle.encode_u8(_f(negative)) == 0).all()
    nans = np.concatenate([pos[nan(pos)], neg[nan(neg)]])
    assert nans.size == 6 and 0x7FC00000 in nans and 0xFFC00000 in nans and 0x7F800001 in nans
    assert (_oracle.encode_u8(_f(nans)) == 0).all()
    assert oracle.oracle_encode_u8(float("nan")) == 0


def test_the_numpy_restatement_is_the_oracle(oracle):
    """tests/_guided.encode_u8, and _temporal's, which calls it, against oracle_encode_u8: every step of the table and the float
    below it, 200 000 random floats of [0, 1.2), and everything of test_outside_the_unit_interval_and_nan, NaN -> 0 included."""
    from tests import _guided, _oracle, _temporal
    first = steps_fixture()["first"]
    pos, neg = _outside_patterns()
    rng = np.random.default_rng(5)
    x = np.concatenate([_f(first), _f(first[1:] - np.uint32(1)), _f(pos), _f(neg), (rng.random(200000) * 1.2).astype(F32)])
    with np.errstate(all="ignore"):
        got = _guided.encode_u8(x)
        again = _temporal.encode_u8(x)
    assert got.dtype == np.uint8 and np.array_equal(got, _oracle.encode_u8(x)) and np.array_equal(again, got)


@pytest.mark.parametrize("name", ["guided", "temporal", "variance"])
def test_the_special_pixel_cases_are_worth_running(oracle, name):
    """(of tests/_post_special.py's inputs, on the restatements alone; tests/test_gpu_post_encode.py runs them on the GPU) At most six
    pixels of the colour plane are special, every kind occurs, sky and surface both have some; between 1 % and 25 % of the
    restatement's output pixels are NaN -- the comparison is neither empty nor all NaN --, at least one of them a sky pixel and one a
    surface pixel, and the expected image has 0 exactly there and the clamp's 255 somewhere."""
    from tests import _post_special as S
    c = S.case(name)
    color, cov, out, image = c["P"]["color"], c["P"]["coverage"], c["want"]["out"], c["want"]["image"]
    special = ~((color >= 0) & (color < 1) & (np.abs(color) >= F32(2.0 ** -126)) | (color.view(np.uint32) == 0))
    assert special.any(axis=2).sum() == 6 == len(c["where"]) and all(special[y, x].any() for y, x in c["where"])
    values = color[special]
    assert np.isnan(values).any() and (values == np.inf).any() and (values == -np.inf).any() and (values > 1).any()
    assert (values.view(np.uint32) == 0x80000000).any() and ((values > 0) & (values < F32(2.0 ** -126))).any()
    assert sum(cov[y, x] == 0 for y, x in c["where"]) == 3 and sum(cov[y, x] > 0 for y, x in c["where"]) == 3
    nan = S.nan_pixels(out)
    print(name, "NaN pixels", int(nan.sum()), "of", nan.size, "sky", int((nan & (cov == 0)).sum()), "surface", int((nan & (cov > 0)).sum()))
    assert 0.01 * nan.size <= nan.sum() <= 0.25 * nan.size
    assert (nan & (cov == 0)).any() and (nan & (cov > 0)).any()
    assert (image[np.isnan(out)] == 0).all() and (image == 255).any() and len(np.unique(image)) > 100
