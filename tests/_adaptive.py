"""What adaptive sampling must return: the contract of include/rt_hip.h ("THE MERGE", rt_resolve_adaptive, rt_render_adaptive's
rounds) restated in numpy, one rounded operation per numpy call, the chunk's error summed in integers.  TEST INFRASTRUCTURE ONLY;
written from the contract's text, not from the kernel's.
"""
import numpy as np

F = np.float32
CHUNK = 32
MUTATIONS = ("no_clamp", "ragged_1024", "no_rezero", "float_sum")


def chunk_grid(w, h):
    """(chunks_x, chunks_y)"""
    return (w + CHUNK - 1) // CHUNK, (h + CHUNK - 1) // CHUNK


def chunk_box(w, h, c):
    """(x0, y0, x1, y1): the pixels of chunk c that lie inside the image."""
    cx, _ = chunk_grid(w, h)
    x0, y0 = (c % cx) * CHUNK, (c // cx) * CHUNK
    return x0, y0, min(x0 + CHUNK, w), min(y0 + CHUNK, h)


def ragged_chunks(w, h):
    """The chunks with fewer than 1024 pixels inside the image."""
    cx, cy = chunk_grid(w, h)
    out = []
    for c in range(cx * cy):
        x0, y0, x1, y1 = chunk_box(w, h, c)
        if (x1 - x0) * (y1 - y0) < CHUNK * CHUNK:
            out.append(c)
    return out


def accum_resolve(sums, n):
    """rt_accum_resolve (rt_math.h): the division in double, rounded once to f32.  n: a number, or an array that broadcasts."""
    return (np.ascontiguousarray(sums, np.uint64).astype(np.float64) / (np.asarray(n, np.float64) * 4294967296.0)).astype(F)


def pixel_errors(accum, fresh, n, mutation=None):
    """e f32 (h, w) of THE MERGE for every pixel, from u64 (h, w, 3) sums that hold n samples each."""
    with np.errstate(all="ignore"):
        a, b = accum_resolve(accum, n), accum_resolve(fresh, n)
        if mutation != "no_clamp":
            a, b = np.minimum(a, F(1.0)), np.minimum(b, F(1.0))
        d = (np.abs(a[..., 0] - b[..., 0]) + np.abs(a[..., 1] - b[..., 1])) + np.abs(a[..., 2] - b[..., 2])
        m = ((a[..., 0] + b[..., 0]) + (a[..., 1] + b[..., 1])) + (a[..., 2] + b[..., 2])
        e = d / np.sqrt(m + F(1e-4))
    assert e.dtype == F
    return e


def merge(accum, fresh, n, chunks, err, mutation=None):
    """(accum', fresh', err') after rt_adaptive_merge over `chunks`: u64 (h, w, 3), (h, w, 3), (chunks of the image,).  The inputs
    are not written.  mutation, for tests of the TESTS only (it is not the contract), one of MUTATIONS:
      "no_clamp":    the means are not clamped at 1
      "no_rezero":   fresh keeps what the merge consumed
      "float_sum":   the chunk's error is summed in f32, pixel after pixel, and quantised once
      "ragged_1024": (the merge is the contract's; chunk_error divides by 1024 whatever lies inside the image)"""
    assert mutation is None or mutation in MUTATIONS, mutation
    accum, fresh, err = np.array(accum, np.uint64), np.array(fresh, np.uint64), np.array(err, np.uint64)
    h, w, _ = accum.shape
    e = pixel_errors(accum, fresh, n, mutation)
    q = (e * F(4294967296.0)).astype(np.uint64)                 # (e <= 300: exact, and the conversion truncates)
    for c in chunks:
        x0, y0, x1, y1 = chunk_box(w, h, c)
        if mutation == "float_sum":
            total = F(0.0)
            for v in e[y0:y1, x0:x1].reshape(-1):
                total = F(total + v)
            err[c] = np.uint64(int(float(total) * 4294967296.0))
        else:
            err[c] = q[y0:y1, x0:x1].sum(dtype=np.uint64)
        accum[y0:y1, x0:x1] += fresh[y0:y1, x0:x1]
        if mutation != "no_rezero":
            fresh[y0:y1, x0:x1] = 0
    return accum, fresh, err


def chunk_error(err_sum, w, h, c, mutation=None):
    """The host's err_c, in double: sum / 2^32 / (pixels of chunk c inside the image)."""
    x0, y0, x1, y1 = chunk_box(w, h, c)
    pixels = CHUNK * CHUNK if mutation == "ragged_1024" else (x1 - x0) * (y1 - y0)
    return float(int(err_sum)) / 4294967296.0 / float(pixels)


def stays_active(err_sum, w, h, c, n, max_samples, threshold, mutation=None):
    """The host's decision after the round that brought chunk c from n to 2n samples."""
    return chunk_error(err_sum, w, h, c, mutation) > float(F(threshold)) and 2 * n < max_samples


def resolve(accum, chunk_samples, encode):
    """(linear f32 (h, w, 3), image u8 (h, w, 3), sample_map i32 (h, w)) of rt_resolve_adaptive; chunk_samples i32 (chunks,);
    encode: rt_encode_u8 per element (tests/_oracle.encode_u8)."""
    accum = np.ascontiguousarray(accum, np.uint64)
    h, w, _ = accum.shape
    cx, cy = chunk_grid(w, h)
    grid = np.asarray(chunk_samples, np.int32).reshape(cy, cx)
    sample_map = np.ascontiguousarray(np.repeat(np.repeat(grid, CHUNK, axis=0), CHUNK, axis=1)[:h, :w])
    with np.errstate(all="ignore"):
        linear = accum_resolve(accum, sample_map[..., None].astype(np.uint32))
    return linear, encode(linear), sample_map


def run(sums_of, w, h, min_samples, max_samples, threshold, mutation=None):
    """The rounds of rt_render_adaptive on sums a caller supplies: sums_of(first, count) -> u64 (h, w, 3), the sums of samples
    [first, first + count) of every pixel.  dict(chunk_samples i32 (chunks,), accum u64 (h, w, 3) -- every chunk's sums over its own
    samples --, fresh (all zero under the contract), first_errors [err_c of the first round per chunk], rounds [(n, active list,
    err u64 (chunks,))])."""
    cx, cy = chunk_grid(w, h)
    n_chunks = cx * cy
    accum = np.array(sums_of(0, min_samples), np.uint64)
    fresh = np.zeros_like(accum)
    err = np.zeros(n_chunks, np.uint64)
    counts = np.zeros(n_chunks, np.int32)
    active = list(range(n_chunks))
    rounds, first_errors = [], None
    n = min_samples
    while active:
        more = np.asarray(sums_of(n, n), np.uint64)
        for c in active:                                        # a launch adds to the listed chunks alone
            x0, y0, x1, y1 = chunk_box(w, h, c)
            fresh[y0:y1, x0:x1] += more[y0:y1, x0:x1]
        accum, fresh, err = merge(accum, fresh, n, active, err, mutation)
        rounds.append((n, list(active), err.copy()))
        if first_errors is None:
            first_errors = [chunk_error(err[c], w, h, c, mutation) for c in range(n_chunks)]
        counts[active] = 2 * n
        active = [c for c in active if stays_active(err[c], w, h, c, n, max_samples, threshold, mutation)]
        n *= 2
    return dict(chunk_samples=counts, accum=accum, fresh=fresh, first_errors=first_errors, rounds=rounds)
