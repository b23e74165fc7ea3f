"""CPU: the JPEG round-trip oracle.  Pillow's save + open decides (jpeg_ref.pil_roundtrip); the numpy restatement of the lossy
stages (jpeg_ref.roundtrip) is pinned to it byte for byte, metrics.jpeg_quant_plan's tables to the
restatement's and its exact-division constants, exhaustively, to //; then the launch-plan query of the library
(cidnet_metric_jpeg_plan: host only, no device is touched) and the public surface that needs no device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpeg_ref as R  # noqa: E402

PLAN_FIELDS = ("mcu_cols", "mcu_rows", "partial_right", "partial_bottom", "chroma_h", "chroma_w", "tiles_x", "workgroups",
               "ws_bytes")


def test_pillow_is_linked_against_libjpeg_turbo():
    """the restatement was pinned against libjpeg-turbo's islow DCTs; another libjpeg would show below, this names the cause"""
    from PIL import features
    assert features.check_feature("libjpeg_turbo"), "Pillow is not linked against libjpeg-turbo (DESIGN.md 6.10)"


@pytest.mark.parametrize("h,w", R.CASES + [R.WIDE])
def test_restatement_equals_pillow(h, w):
    for kind in R.KINDS:
        img = R.image(kind, h, w, 1000 * h + w)
        got, want = R.roundtrip(img, 75), R.pil_roundtrip(img, 75)
        assert got.dtype == np.uint8 and got.shape == img.shape
        assert np.array_equal(got, want), (kind, h, w, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("quality", R.QUALITIES)
def test_restatement_equals_pillow_at_other_qualities(quality):
    for kind in R.KINDS:
        img = R.image(kind, 50, 70, quality)
        assert np.array_equal(R.roundtrip(img, quality), R.pil_roundtrip(img, quality)), (kind, quality)


def test_saturated_images_reach_both_clamps():
    out = R.pil_roundtrip(R.image("saturated", 50, 70, 3), 75)
    assert out.min() == 0 and out.max() == 255


def test_narrow_images_are_refused():
    with pytest.raises(AssertionError):
        R.roundtrip(np.zeros((3, 8, 4), np.uint8))
    from hvi_cidnet_amd import _lib
    L = _lib.lib()
    assert _plan(8, 4)[0] == -1 and _plan(8, 5)[0] == 0                    # CIDNET_ERR_ARG below five columns
    assert L.raw("cidnet_metric_jpeg_ws_bytes")(1, 8, 4) == 0


def test_quant_plan_tables_equal_the_restatement():
    from hvi_cidnet_amd import metrics as M
    for q in (1, 10, 25, 49, 50, 75, 90, 95, 100):
        p = M.jpeg_quant_plan(q)
        luma, chroma = R.tables(q)
        assert p.quality == q and p.luma.dtype == np.int32 and p.luma.shape == (8, 8) and p.chroma.shape == (8, 8)
        assert np.array_equal(p.luma, luma) and np.array_equal(p.chroma, chroma)
        assert np.array_equal(p.divisors, np.stack([luma, chroma]) * 8)
        assert p.luma.min() >= 1 and p.chroma.max() <= 255
        dev = p.device_table()
        assert dev.dtype == np.int32 and dev.shape == (2, 2, 64) and dev.flags["C_CONTIGUOUS"]
        assert np.array_equal(dev[:, 0], np.stack([luma, chroma]).reshape(2, 64))
        assert np.array_equal(dev[:, 1].astype(np.int64), p.magic.reshape(2, 64)) and dev.min() >= 1
        assert M.jpeg_quant_plan(q) is p                                   # cached
        with pytest.raises(ValueError):
            p.luma[0, 0] = 3                                               # read-only
    assert M.jpeg_quant_plan(75).luma[0, 0] == 8 and M.jpeg_quant_plan(100).luma.max() == 1
    assert M.jpeg_quant_plan(1).chroma.min() == 255
    for bad in (0, 101, -5, 75.5, True):
        with pytest.raises(ValueError):
            M.jpeg_quant_plan(bad)


def test_division_constants_are_exact_for_every_divisor_and_numerator():
    """the kernel's quotient, the high 32 bits of n * magic, against // for every divisor 8 t, t = 1..255, and every
    numerator 0..65535"""
    from hvi_cidnet_amd import metrics as M
    n = np.arange(65536, dtype=np.uint64)
    for t in range(1, 256):
        d, m = 8 * t, M._jpeg_magic(8 * t)
        assert m == -((-1 << 32) // d) and 0 < m < 2 ** 31                 # it travels as an int32
        got = (n * np.uint64(m)) >> np.uint64(32)
        assert np.array_equal(got, n // np.uint64(d)), d
    for q in range(1, 101):                                                # and every plan carries exactly those
        p = M.jpeg_quant_plan(q)
        assert p.shift == 32
        assert p.magic.reshape(-1).tolist() == [M._jpeg_magic(d) for d in p.divisors.reshape(-1).tolist()]


def _plan(h, w, n=12):
    """cidnet_metric_jpeg_plan -> (status, {field: value}); the buffer is prefilled so that unwritten fields show"""
    from hvi_cidnet_amd import _lib
    buf = (ctypes.c_int * 12)(*([-7] * 12))
    rc = _lib.lib().raw("cidnet_metric_jpeg_plan")(h, w, buf, n)
    vals = list(buf)
    if rc == 0:
        assert vals[9:] == [-7] * 3                                        # never past its own fields
    else:
        assert vals == [-7] * 12                                           # nothing is written on an error
    return rc, dict(zip(PLAN_FIELDS, vals))


def test_plan_query_contract():
    from hvi_cidnet_amd import _lib
    L = _lib.lib()
    for h, w in R.CASES + [R.WIDE, (400, 600), (1024, 1024), (16, 128), (16, 129), (65500, 16)]:
        rc, p = _plan(h, w)
        what = (h, w, p)
        assert rc == 0, what
        assert (p["mcu_cols"], p["mcu_rows"]) == (-(-w // 16), -(-h // 16)), what
        assert (p["partial_right"], p["partial_bottom"]) == (int(w % 16 != 0), int(h % 16 != 0)), what
        assert (p["chroma_h"], p["chroma_w"]) == ((h + 1) // 2, (w + 1) // 2), what
        assert p["tiles_x"] >= 1 and p["workgroups"] == p["tiles_x"] * p["mcu_rows"], what
        assert (p["tiles_x"] - 1) * 8 < p["mcu_cols"] <= p["tiles_x"] * 8, what      # 8 MCUs a workgroup, none without one
        assert p["ws_bytes"] >= 256 * p["mcu_cols"] * p["mcu_rows"] + 2 * p["chroma_h"] * p["chroma_w"], what
        assert L.raw("cidnet_metric_jpeg_ws_bytes")(1, h, w) == p["ws_bytes"], what
        assert L.raw("cidnet_metric_jpeg_ws_bytes")(3, h, w) == 3 * p["ws_bytes"], what
    # aligned, partial on the right only, partial at the bottom only
    assert _plan(16, 16)[1]["partial_right"] == 0 and _plan(16, 16)[1]["partial_bottom"] == 0
    assert (_plan(32, 34)[1]["partial_right"], _plan(32, 34)[1]["partial_bottom"]) == (1, 0)
    assert (_plan(18, 32)[1]["partial_right"], _plan(18, 32)[1]["partial_bottom"]) == (0, 1)
    wide = _plan(*R.WIDE)[1]
    assert wide["tiles_x"] > 1 and wide["mcu_rows"] > 1                    # what tests/test_jpeg_gpu.py's WIDE case relies on
    assert wide["mcu_cols"] < 8 * wide["tiles_x"]                          # and its last workgroup of a row is not full


def test_plan_query_bad_arguments():
    from hvi_cidnet_amd import _lib
    for h, w in [(0, 8), (-3, 8), (8, 0), (8, 4), (8, -1)]:
        assert _plan(h, w)[0] == -1, (h, w)                                # CIDNET_ERR_ARG
    assert _plan(8, 8, n=8)[0] == -1                                       # too small a buffer: nothing written
    assert _plan(8, 8, n=9)[0] == 0
    assert _lib.lib().raw("cidnet_metric_jpeg_plan")(8, 8, None, 9) == -1
    assert _plan(65501, 16)[0] == -2 and _plan(16, 65501)[0] == -2         # CIDNET_ERR_SHAPE: no such JPEG file
    assert _plan(40000, 40000)[0] == -2                                    # more than 2^22 MCUs


def test_launcher_argument_checks_need_no_device():
    """every refusal of the launcher that is decided before anything is launched"""
    from hvi_cidnet_amd import _lib
    L = _lib.lib()
    f = L.raw("cidnet_metric_jpeg_roundtrip_u8")
    p = ctypes.c_void_p(4096)                                              # never dereferenced: every call below is refused
    ws = L.raw("cidnet_metric_jpeg_ws_bytes")(2, 24, 40)
    assert ws == 2 * 2 * 3 * 384
    assert f(None, p, p, ws, p, 2, 24, 40, None) == -1
    assert f(p, None, p, ws, p, 2, 24, 40, None) == -1
    assert f(p, p, None, ws, p, 2, 24, 40, None) == -1
    assert f(p, p, p, ws, None, 2, 24, 40, None) == -1
    assert f(p, p, ctypes.c_void_p(4100), ws, p, 2, 24, 40, None) == -1    # a workspace off its 16-byte alignment
    for B, h, w in [(0, 24, 40), (2, 0, 40), (2, 24, 4), (2, 24, 0)]:
        assert f(p, p, p, ws, p, B, h, w, None) == -1, (B, h, w)
    assert f(p, p, p, ws - 1, p, 2, 24, 40, None) == -3                    # CIDNET_ERR_WS
    assert f(p, p, p, 1 << 40, p, 65536, 24, 40, None) == -2               # CIDNET_ERR_SHAPE
    assert f(p, p, p, 1 << 40, p, 1, 65501, 40, None) == -2


def test_names_are_exported_and_cpu_tensors_refused():
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import metrics as M
    assert P.jpeg_roundtrip_u8 is M.jpeg_roundtrip_u8 and P.jpeg_quant_plan is M.jpeg_quant_plan
    assert _lib_version() >= 19
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.jpeg_roundtrip_u8(torch.zeros((1, 3, 8, 8), dtype=torch.uint8))
    r = M.UnpairedResult(alpha=1.0, niqe=4.0)
    assert "file_roundtrip" not in r.per_image


def _lib_version():
    from hvi_cidnet_amd import _lib
    return _lib.lib().raw("cidnet_abi_version")()
