"""CPU: the contract of the on-device JPEG encoder before any device is involved.  The numpy restatement of the file
(tests/jpegenc_ref.py: coefficients of tests/jpeg_ref.py, dummy blocks, DC chain, Huffman coding, stuffing, framing) equals
Pillow's bytes with no tolerance on every case of the contract, each coding path is reached by a named case (asserted through
the restatement's counters), the library's plan equals the restatement's, the slot capacity bounds every scan, every refusal
is decided before a launch, and jpeg_file's 623 header bytes are Pillow's."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import jpegenc_ref as R  # noqa: E402

_files = {}


def _file(kind, h, w, q):
    """-> (image, the restatement's file, its counters), computed once and shared"""
    key = (kind, h, w, q)
    if key not in _files:
        img = R.case_image(kind, h, w, q)
        img.setflags(write=False)
        _files[key] = (img, *R.jpeg_file(img, q))
    return _files[key]


def test_pillow_is_libjpeg_turbo():
    from PIL import features
    assert features.check_feature("libjpeg_turbo"), "these bytes were pinned to libjpeg-turbo's encoder; another libjpeg: " + \
        str(features.version("jpg"))


@pytest.mark.parametrize("kind,h,w,q", R.cases(), ids=lambda v: str(v))
def test_restatement_equals_pillow(kind, h, w, q):
    img, data, n = _file(kind, h, w, q)
    want = R.pil_file(img, q)
    assert data[:R.HEADER_BYTES] == want[:R.HEADER_BYTES]
    assert data == want, (kind, h, w, q, len(data), len(want))
    assert len(data) - R.HEADER_BYTES - 2 <= R.plan(h, w)["capacity"]         # the slot bounds the scan


def test_every_coding_path_is_reached_by_a_named_case():
    n = _file("random", 50, 70, 1)[2]
    print("(50,70) random q1:", n)
    assert n["zrl"] == 47                                                     # runs of 16 and more zeros
    n = _file("random", 50, 70, 100)[2]
    print("(50,70) random q100:", n)
    # blocks that end on coefficient 63; stuffed bytes -- counted in Pillow's own file, whose framing holds no FF 00
    assert n["no_eob"] == 92 and n["stuffed"] == R.pil_file(_file("random", 50, 70, 100)[0], 100).count(b"\xff\x00") == 61
    n = _file("checker_pixels", 16, 16, 100)[2]
    print("checker of pixels q100:", n)
    assert n["ac_cat"] == 10 and n["stuffed"] == 30                           # the largest AC category
    n = _file("checker_blocks", 16, 32, 100)[2]
    print("checker of blocks q100:", n)
    assert n["dc_cat"] == 11                                                  # the largest DC category
    # dummy blocks: the right column alone, both, the bottom row alone; and none
    assert (R.plan(8, 8)["dummies"], R.plan(24, 24)["dummies"], R.plan(18, 34)["dummies"], R.plan(1, 1)["dummies"]) == (3, 7, 9, 3)
    for (h, w), (right, bottom) in {(16, 8): (True, False), (8, 16): (False, True), (8, 8): (True, True),
                                    (24, 24): (True, True), (18, 34): (True, True), (1, 1): (True, True)}.items():
        p = R.plan(h, w)
        assert (2 * p["mcu_cols"] > p["block_cols"], 2 * p["mcu_rows"] > p["block_rows"]) == (right, bottom), (h, w)
    for h, w in ((8, 8), (24, 24), (18, 34)):
        assert _file("random", h, w, 75)[2]["dummies"] == R.plan(h, w)["dummies"] > 0
    assert _file("random", 1, 1, 75)[2]["dummies"] == 3
    assert _file("constant", 16, 16, 75)[2]["dummies"] == 0


def test_dummy_blocks_are_six_bits_and_leave_the_predictor():
    """(8,8): one real luma block, three dummies.  The scan's length is that of the real blocks + 3 x 6 bits"""
    img, data, n = _file("random", 8, 8, 75)
    y, cb, cr = R.coefficients(img, 75)
    assert np.abs(y[0, 1, 1:]).sum() > 0                                      # the replicated block the round trip transforms has AC
    assert n["dummies"] == 3
    wide = np.concatenate([np.asarray(img)] * 2, axis=2)[:, :, :9]            # (8,9): the second block column is real
    assert R.jpeg_file(wide, 75)[1]["dummies"] == 2


def _plan(h, w, n=9):
    from hvi_cidnet_amd import _lib
    buf = (ctypes.c_long * 11)(*([-7] * 11))
    rc = _lib.lib().raw("cidnet_jpeg_encode_plan")(h, w, buf, n)
    return rc, list(buf)


def test_library_plan():
    from hvi_cidnet_amd import _lib, image_io as IO
    for h, w in R.SIZES + R.TINY + [(16, 32), (400, 600), (1024, 1024), (1728, 2304), (65500, 16), (16, 65500)]:
        rc, out = _plan(h, w)
        want = R.plan(h, w)
        assert rc == 0 and out[9:] == [-7, -7]
        assert out[:5] == [want[k] for k in ("mcu_cols", "mcu_rows", "block_cols", "block_rows", "dummies")], (h, w, out)
        assert out[6] == want["capacity"] and out[6] % 4 == 0 and out[5] % 16 == 0 and out[7] == want["groups"]
        assert out[8] == -(-want["mcu_cols"] // 8) * want["mcu_rows"]
        p = IO.jpeg_encode_plan(h, w)
        assert (p.mcu_cols, p.mcu_rows, p.block_cols, p.block_rows, p.dummies, p.ws_bytes, p.capacity, p.groups,
                p.workgroups) == tuple(out[:9])
    assert R.plan(97, 131)["groups"] >= 3 and IO.jpeg_encode_plan(97, 131).groups == 4     # the scan crosses its block size
    assert R.plan(35, 277)["mcu_rows"] == 3 and IO.jpeg_encode_plan(35, 277).workgroups == 9
    assert 3.0 < IO.jpeg_encode_plan(400, 600).capacity / (400 * 600 * 3) < 3.3                  # what a slot costs over the raw image
    for bad in ((0, 5), (5, 0), (-1, 5)):
        assert _plan(*bad) == (-1, [-7] * 11)
        with pytest.raises(ValueError):
            IO.jpeg_encode_plan(*bad)
    assert _plan(5, 5, n=8) == (-1, [-7] * 11)
    assert _lib.lib().raw("cidnet_jpeg_encode_plan")(5, 5, None, 9) == -1
    assert _plan(65501, 16)[0] == -2 and _plan(16, 65501)[0] == -2
    assert _plan(32768, 32768)[0] == 0 and _plan(32768, 32784)[0] == -2                    # 2^22 MCUs, and one column more
    with pytest.raises(ValueError):
        IO.jpeg_encode_plan(65501, 16)
    for w in (1, 2, 3, 4):                                                                  # the round trip's w >= 5 is not ours
        assert _plan(7, w)[0] == 0


def test_every_refusal_is_decided_before_a_launch():
    """no device here: a call that got as far as a launch would fail with a HIP error (a positive code) or fault"""
    from hvi_cidnet_amd import _lib, image_io as IO
    h, w = 7, 9
    p = IO.jpeg_encode_plan(h, w)
    fake = 0x10000                                                                          # never dereferenced
    good = dict(src=fake + 1, ss=3 * h * w, dst=fake, ds=p.capacity, sizes=fake, ws=fake, wsb=p.ws_bytes, qtab=fake, B=1, h=h, w=w)

    def call(**kw):
        a = {**good, **kw}
        return _lib.lib().raw("cidnet_jpeg_encode_u8")(a["src"], a["ss"], a["dst"], a["ds"], a["sizes"], a["ws"], a["wsb"],
                                                       a["qtab"], a["B"], a["h"], a["w"], None)
    for bad in (dict(src=None), dict(dst=None), dict(sizes=None), dict(ws=None), dict(qtab=None), dict(B=0), dict(h=0), dict(w=0),
                dict(h=-3), dict(ds=p.capacity - 4), dict(ds=p.capacity + 2), dict(dst=fake + 2), dict(ws=fake + 8),
                dict(sizes=fake + 4), dict(qtab=fake + 2), dict(ss=3 * h * w - 1)):
        assert call(**bad) == -1, bad
    assert call(wsb=p.ws_bytes - 1) == -3 and call(B=2) == -3
    assert call(h=65501) == -2 and call(w=65501) == -2 and call(B=65536, wsb=1 << 60, ds=p.capacity) == -2
    assert call(h=32768, w=32784) == -2


def test_header_is_pillows():
    from hvi_cidnet_amd import image_io as IO
    for q in R.QUALITIES:
        for h, w in ((50, 70), (1, 1), (300, 65500)):
            head = IO.jpeg_file(h, w, q, b"")
            assert len(head) == IO.JPEG_HEADER_BYTES + 2 == 625 and head[-2:] == b"\xff\xd9"
            assert head[:-2] == R.header(h, w, q)
        img = R.case_image("random", 50, 70, q)
        assert IO.jpeg_file(50, 70, q, b"")[:623] == R.pil_file(img, q)[:623], q
        data, _ = R.scan(img, q)
        assert IO.jpeg_file(50, 70, q, data) == R.pil_file(img, q)
        assert IO.jpeg_file(50, 70, q, np.frombuffer(data, np.uint8)) == R.pil_file(img, q)


def test_public_surface_without_a_device(tmp_path):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib, image_io as IO
    for name in ("jpeg_encode_plan", "JpegEncodePlan", "jpeg_scan_u8", "jpeg_file", "jpeg_encode_u8"):
        assert name in P.__all__ and getattr(P, name) is getattr(IO, name), name
    protos = _lib.parse_header()
    for name, n_args in (("cidnet_jpeg_encode_plan", 4), ("cidnet_jpeg_encode_u8", 12)):
        assert name in protos and len(protos[name][1]) == n_args, name
    assert _lib.lib().raw("cidnet_abi_version")() >= 22
    for bad in ((0, 9), (9, 0), (65501, 9)):
        with pytest.raises(ValueError):
            IO.jpeg_file(*bad, 75, b"")
    for bad in (0, 101, 7.5, True):
        with pytest.raises(ValueError):
            IO.jpeg_file(8, 8, bad, b"")
        with pytest.raises(ValueError):
            IO.jpeg_scan_u8(torch.zeros((2, 2, 3), dtype=torch.uint8), bad)
    with pytest.raises(RuntimeError, match="CPU"):
        IO.jpeg_scan_u8(torch.zeros((2, 2, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="CPU"):
        IO.jpeg_encode_u8(torch.zeros((2, 2, 3), dtype=torch.uint8))
    for bad in ("gpu", None, True, "Device"):
        with pytest.raises(ValueError, match="jpeg"):
            P.enhance_folder(None, str(tmp_path), str(tmp_path / "out"), jpeg=bad)
        with pytest.raises(ValueError, match="jpeg"):
            P.evaluate(None, [], save_dir=str(tmp_path / "out"), jpeg=bad)
        with pytest.raises(ValueError, match="jpeg"):
            P.evaluate_unpaired(None, [torch.zeros(3, 96, 96)], P.metrics.NiqeParams(None, None, None),
                                save_dir=str(tmp_path / "out"), jpeg=bad)
        with pytest.raises(ValueError, match="jpeg"):
            IO._Writer(None, jpeg=bad)
    with pytest.raises(ValueError, match="jpeg_prefix"):
        IO._Writer(None, jpeg_prefix=0)
    assert not (tmp_path / "out").exists()
    r = P.EnhanceReport()
    assert (r.jpeg, r.jpeg_second_copies, r.png) == ("pillow", 0, "pillow")
    for fn in (P.enhance_folder, P.evaluate, P.evaluate_unpaired):
        assert inspect.signature(fn).parameters["jpeg"].default == "pillow"
    assert inspect.signature(IO._Writer.__init__).parameters["jpeg_prefix"].default == 0.25
