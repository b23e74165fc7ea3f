"""CPU: the PNG writer's stream contract.  zlib.decompress and Pillow decide whether the numpy restatement (tests/png_ref.py,
DESIGN.md 6.12) writes valid streams and files that decode to the exact pixels; the library's host-only entry points
(cidnet_png_code_lengths: the procedure the kernel runs; cidnet_png_plan: the function the launcher calls) are pinned to the
restatement; the size of the files is held against Pillow's default writer on photographic content; then the public surface
that needs no device."""
import ctypes
import heapq
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import png_ref as R  # noqa: E402


def _decodes(img, mode, seg):
    from PIL import Image
    h, w, _ = img.shape
    info = {}
    stream = R.zlib_stream(img, mode, seg, info)
    assert stream[:2] == b"\x78\x01"
    assert zlib.decompress(stream) == info["filtered"], (mode, seg)
    assert len(stream) == 2 + (info["bits"] + 7) // 8 + 4
    assert len(stream) <= R.capacity(h, w, seg), (h, w, mode, seg, len(stream), R.capacity(h, w, seg))
    with Image.open(io.BytesIO(R.png_file(h, w, stream))) as im:
        assert im.mode == "RGB" and im.size == (w, h)
        assert np.array_equal(np.asarray(im), img), (h, w, mode, seg)
    return stream


@pytest.mark.parametrize("h,w", R.SIZES)
def test_zlib_and_pillow_decode_the_restatement(h, w):
    for kind in R.KINDS:
        img = R.image(kind, h, w, 1000 * h + w)
        for seg in R.SEGMENTS:
            for mode in R.MODES:
                _decodes(img, mode, seg)


def test_the_cases_reach_their_plans():
    assert R.plan(40, 56, 512) == dict(rows=3, segments=14, last_short=1, row_exceeds=0, row_bytes=169)
    assert R.plan(17, 300, 512) == dict(rows=1, segments=17, last_short=0, row_exceeds=1, row_bytes=901)
    assert R.plan(64, 96, 32768)["segments"] == 1 and R.plan(64, 96, 512)["segments"] == 64


def test_filters_invert_and_adaptive_takes_the_smallest_score():
    img = R.image("grain", 7, 9, 3)
    for mode in R.MODES:
        types, filt = R.filter_rows(img, mode)
        assert np.array_equal(R.unfilter_reference(filt, 7, 9), img), mode
        assert (filt[:, 0] == types).all()
    cand = R._candidates(img).astype(np.int64)
    score = np.minimum(cand, 256 - cand).sum(axis=2)
    types, _ = R.filter_rows(img, "adaptive")
    for y in range(7):
        assert score[types[y], y] == score[:, y].min() and not (score[:types[y], y] == score[:, y].min()).any()
    flat = np.full((3, 4, 3), 9, np.uint8)                               # ties go to the lowest type: Sub = Paeth in row 0,
    assert R.filter_rows(flat, "adaptive")[0].tolist() == [1, 2, 2]      # Up = Paeth = 0 below it


def test_a_constant_image_has_a_two_symbol_code():
    img = np.zeros((40, 56, 3), np.uint8)
    _, filt = R.filter_rows(img, "none")
    freq = np.bincount(filt.reshape(-1), minlength=257).tolist()
    freq[256] = 1
    lens = R.code_lengths(freq, 15)
    assert sorted(v for v in lens if v) == [1, 1]
    _decodes(img, "none", 32768)


def _fib_freq():
    img = R.fibonacci_image()
    _, filt = R.filter_rows(img, "none")
    freq = np.bincount(filt.reshape(-1), minlength=257)
    freq[256] = 1
    return img, freq.tolist()


def test_the_limiter():
    img, freq = _fib_freq()
    assert img.shape == (48, 47, 3) and R.plan(48, 47)["segments"] == 1
    depth = R.tree_depths({s: c for s, c in enumerate(freq) if c})
    assert max(depth.values()) > 15, max(depth.values())
    lens = R.code_lengths(freq, 15)
    assert max(lens) <= 15
    _decodes(img, "none", 32768)


def _heap_cost(freq):
    """(cost, depth) of a heapq Huffman tree of the used counts"""
    heap = [(c, i, 0) for i, c in enumerate(freq) if c]
    if len(heap) == 1:
        return heap[0][0], 1
    heapq.heapify(heap)
    cost, tick = 0, len(freq)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], tick, max(a[2], b[2]) + 1))
        tick += 1
    return cost, heap[0][2]


def _lib_lengths(freq, maxbits):
    from hvi_cidnet_amd import _lib
    f = (ctypes.c_uint * len(freq))(*freq)
    out = (ctypes.c_uint8 * len(freq))()
    rc = _lib.lib().raw("cidnet_png_code_lengths")(f, len(freq), maxbits, out)
    return rc, list(out)


def _histograms():
    rng = np.random.default_rng(12)
    out = [_fib_freq()[1], [0] * 40 + [7] + [0] * 216, [3, 0, 0, 5], [1, 1], [5] * 257, list(range(1, 258))]
    for t in range(60):
        n = int(rng.integers(2, 258))
        f = rng.integers(0, 60, n) * (rng.random(n) < 0.7)
        if t % 3 == 0:
            f = rng.geometric(0.002, n)
        if t % 3 == 1:
            f = (2.0 ** rng.uniform(0, 20, n)).astype(np.int64) * (rng.random(n) < 0.5)
        out.append([int(v) for v in f])
    return [f for f in out if any(f)]


@pytest.mark.parametrize("maxbits", [15, 7])
def test_library_code_lengths_equal_the_restatement(maxbits):
    for freq in _histograms():
        if maxbits == 7:
            freq = freq[:19]                                             # the code-length code has 19 symbols
            if not any(freq):
                continue
        rc, lens = _lib_lengths(freq, maxbits)
        assert rc == 0
        want = R.code_lengths(freq, maxbits)
        assert lens == want, (freq, lens, want)
        used = [v for v in lens if v]
        assert len(used) == sum(1 for c in freq if c) and all(v == 0 for v, c in zip(lens, freq) if not c)
        assert max(used) <= maxbits
        if len(used) >= 2:
            assert sum(2 ** (maxbits - v) for v in used) == 2 ** maxbits    # Kraft: the code is complete
        else:
            assert used == [1]
        cost, depth = _heap_cost(freq)
        if len(used) >= 2 and depth <= maxbits:                          # a Huffman tree fits: ours costs what it costs
            assert sum(c * v for c, v in zip(freq, lens)) == cost, freq


def test_library_code_lengths_refusals():
    assert _lib_lengths([1, 2, 3], 0)[0] == -1 and _lib_lengths([1, 2, 3], 16)[0] == -1
    assert _lib_lengths([1] * 9, 3)[0] == -2                             # nine symbols have no 3-bit code
    assert _lib_lengths([1 << 23, 1], 15)[0] == -2                       # a count must fit the sort key
    from hvi_cidnet_amd import _lib
    assert _lib.lib().raw("cidnet_png_code_lengths")(None, 3, 15, None) == -1


def _plan(h, w, seg, n=6):
    from hvi_cidnet_amd import _lib
    buf = (ctypes.c_long * 8)(*([-7] * 8))
    rc = _lib.lib().raw("cidnet_png_plan")(h, w, seg, buf, n)
    return rc, list(buf)


def test_library_plan():
    from hvi_cidnet_amd import image_io as IO
    for h, w in R.SIZES + [(48, 47), (400, 600), (1024, 1024)]:
        for seg in R.SEGMENTS + (1, 100000000):
            rc, out = _plan(h, w, seg)
            want = R.plan(h, w, seg)
            assert rc == 0 and out[6:] == [-7, -7]
            assert out[:4] == [want["rows"], want["segments"], want["last_short"], want["row_exceeds"]], (h, w, seg, out)
            assert out[4] == (h * (1 + 3 * w) + 15) // 16 * 16 + want["segments"] * 1328
            assert out[5] == R.capacity(h, w, seg) and out[5] % 4 == 0
            p = IO.png_plan(h, w, seg)
            assert (p.rows, p.segments, p.last_short, p.row_exceeds, p.ws_bytes, p.capacity) == \
                (out[0], out[1], bool(out[2]), bool(out[3]), out[4], out[5])
    assert IO.png_plan(400, 600).capacity < 1.39 * 400 * 600 * 3         # what a slot costs over the raw image
    for bad in ((0, 5, 512), (5, 0, 512), (5, 5, 0), (-1, 5, 512)):
        assert _plan(*bad)[0] == -1 and _plan(*bad)[1] == [-7] * 8
        with pytest.raises(ValueError):
            IO.png_plan(*bad)
    assert _plan(5, 5, 512, n=5) == (-1, [-7] * 8)
    from hvi_cidnet_amd import _lib
    assert _lib.lib().raw("cidnet_png_plan")(5, 5, 512, None, 6) == -1
    assert _plan(4, 1400000, 512)[0] == -2                               # one row of more than 2^22 bytes
    assert _plan(4000, 2000, 1 << 30)[0] == -2                           # a segment of more than 2^22 bytes
    assert _plan(4000, 2000, 1 << 22)[0] == 0
    with pytest.raises(ValueError):
        IO.png_plan(4, 1400000)


def test_capacity_bounds_every_stream_of_the_restatement():
    for h, w in R.SIZES:
        for kind in R.KINDS:
            img = R.image(kind, h, w, 7 * h + w)
            for seg in R.SEGMENTS:
                for mode in ("adaptive", "none"):
                    assert len(R.zlib_stream(img, mode, seg)) <= R.capacity(h, w, seg)
    img, _ = _fib_freq()
    assert len(R.zlib_stream(img, "none")) <= R.capacity(48, 47)


def test_files_are_no_larger_than_pillows_on_grain():
    """the three grain cases of DESIGN.md 6.12's table: at most 1.02 x Pillow's default file (measured: 0.952, 0.973, 0.978)"""
    from PIL import Image
    for h, w, sigma in ((100, 150, 1.0), (100, 150, 4.0), (64, 96, 12.0)):
        img = R.scene(h, w, sigma, 7)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "PNG")
        ours = len(R.png_file(h, w, _decodes(img, "adaptive", 32768)))
        print(h, w, sigma, "ours", ours, "pillow", buf.tell(), "ratio", ours / buf.tell())
        assert ours <= 1.02 * buf.tell(), (h, w, sigma, ours, buf.tell())


def test_public_surface_without_a_device():
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib, image_io as IO
    for name in ("png_plan", "PngPlan", "png_zlib_u8", "png_file", "png_encode_u8"):
        assert name in P.__all__ and getattr(P, name) is getattr(IO, name), name
    protos = _lib.parse_header()
    for name, n_args in (("cidnet_png_plan", 5), ("cidnet_png_code_lengths", 4), ("cidnet_png_encode_u8", 13)):
        assert name in protos and len(protos[name][1]) == n_args, name
    assert _lib.lib().raw("cidnet_abi_version")() >= 21
    stream = R.zlib_stream(R.image("grain", 7, 9, 1))
    assert IO.png_file(7, 9, stream) == R.png_file(7, 9, stream)
    assert IO.png_file(7, 9, np.frombuffer(stream, np.uint8)) == R.png_file(7, 9, stream)
    with pytest.raises(ValueError):
        IO.png_file(0, 9, stream)
    with pytest.raises(RuntimeError, match="CPU"):
        IO.png_zlib_u8(torch.zeros((2, 2, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="CPU"):
        IO.png_encode_u8(torch.zeros((2, 2, 3), dtype=torch.uint8))
    for bad in (dict(filter="best"), dict(segment_bytes=0), dict(segment_bytes=2.5)):
        with pytest.raises(ValueError):
            IO.png_zlib_u8(torch.zeros((2, 2, 3), dtype=torch.uint8), **bad)


def test_png_mode_is_checked_before_anything_runs(tmp_path):
    import hvi_cidnet_amd as P
    for bad in ("gpu", None, True, "Device"):
        with pytest.raises(ValueError, match="png"):
            P.enhance_folder(None, str(tmp_path), str(tmp_path / "out"), png=bad)
        with pytest.raises(ValueError, match="png"):
            P.evaluate(None, [], save_dir=str(tmp_path / "out"), png=bad)
        with pytest.raises(ValueError, match="png"):
            P.evaluate_unpaired(None, [torch.zeros(3, 96, 96)], P.metrics.NiqeParams(None, None, None),
                                save_dir=str(tmp_path / "out"), png=bad)
    assert not (tmp_path / "out").exists()
    assert P.EnhanceReport().png == "pillow"
    import inspect
    for fn in (P.enhance_folder, P.evaluate, P.evaluate_unpaired):
        assert inspect.signature(fn).parameters["png"].default == "pillow"
