"""The u8 output of the post passes on pixels that are not in [0, 1]: the guided denoiser, the temporal accumulation and the
variance-guided filter at 37 x 21 (one filter iteration) on tests/_post_special.py's inputs -- a colour plane with six special
pixels: NaN, +inf, -inf, -0, a denormal, a value above 1, on sky and on surface pixels -- through the host path and through the
device path.  Bar: `out` has the restatement's bits or both are NaN; `image` equals tests/_guided.encode_u8 of the restatement,
where NaN encodes to 0 (deviation D11, oracle/oracle.h).  That the restatement's output has NaN on 1 % .. 25 % of its pixels, sky and
surface, is shown on the CPU (tests/test_encode_cpu.py)."""
import numpy as np
import pytest

from tests import _post_special as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import raytracing_c_amd as rt
    assert rt.lib.rt_init(0) == 0, rt.last_error()
    return rt


def _run(rt, name, path):
    """(out f32 (h, w, 3), image u8 (h, w, 3)) of pass `name` on its special case."""
    import torch
    from tests.test_gpu_guided import SIGMAS, _side_stream_call
    from tests.test_gpu_temporal import TOLERANCES, _args, _device, _host
    from tests.test_gpu_variance import FSIGMAS
    c = S.case(name)
    P = c["P"]
    if name == "guided":
        kw = dict(iterations=1, sigma_color=SIGMAS[0], sigma_normal=SIGMAS[1], sigma_position=SIGMAS[2], demodulate=True, image=True)
        return rt.guided_denoise(*_args(P), **kw) if path == "host" else _side_stream_call(rt, P, **kw)
    if name == "temporal":
        r = (_host if path == "host" else _device)(rt, P, c["hist"], True, TOLERANCES[0])
        return r["out"], r["image"]
    kw = dict(iterations=1, sigma_color=FSIGMAS[0], sigma_normal=FSIGMAS[1], sigma_position=FSIGMAS[2], demodulate=True, image=True)
    if path == "host":
        r = rt.guided_denoise_variance(*_args(P), c["variance"], **kw)
        return r["out"], r["image"]
    side = torch.cuda.Stream()
    t = [torch.from_numpy(np.array(a)).cuda() for a in (*_args(P), c["variance"])]
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        r = rt.guided_denoise_variance(*t, **kw)
    side.synchronize()
    return r["out"].cpu().numpy(), r["image"].cpu().numpy()


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("name", S.PASSES)
def test_post_pass_u8_of_pixels_outside_the_unit_interval(rt, oracle, name, path):
    want = S.case(name)["want"]
    out, image = _run(rt, name, path)
    assert out.dtype == np.float32 and out.shape == want["out"].shape and image.dtype == np.uint8 and image.shape == want["image"].shape
    same = S.same_bits_or_both_nan(out, want["out"])
    bad = np.argwhere(~same)
    print(name, path, "NaN pixels", int(S.nan_pixels(out).sum()), "of the restatement", int(S.nan_pixels(want["out"]).sum()),
          "differing floats", len(bad), "differing bytes", int((image != want["image"]).sum()))
    assert len(bad) == 0, (len(bad), bad[:4].tolist(), [hex(int(v)) for v in out.view(np.uint32)[~same][:4]],
                           [hex(int(v)) for v in want["out"].view(np.uint32)[~same][:4]])
    diff = np.argwhere(image != want["image"])
    assert len(diff) == 0, (len(diff), diff[:4].tolist(), image[image != want["image"]][:4].tolist(), want["image"][image != want["image"]][:4].tolist())
    assert (image[np.isnan(out)] == 0).all()
