"""The oracle of the JPEG encoder tests (tests/test_jpegenc_cpu.py, tests/test_jpegenc_gpu.py, tests/test_enhance_jpeg_gpu.py).

pil_file() IS the oracle: the bytes Pillow's Image.fromarray(a).save(f, 'JPEG', quality=q) writes.  scan() and header() restate
that file in numpy and plain Python: the quantised coefficients of tests/jpeg_ref.py's transform (taken before
the dequantise step), libjpeg's dummy blocks, the DC chain, run-length / Huffman coding with the Annex K tables, MSB-first bit
packing, byte stuffing and the 1-filled tail; then the 623 bytes of framing.  test_jpegenc_cpu.py pins the restatement to
Pillow, so a disagreement is a mistake of the restatement, never of Pillow.  Images are planar uint8 (3,h,w) as jpeg_ref.image
makes them; any h, w >= 1 (the w >= 5 limit of the round trip belongs to the decoder)."""
import io
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_ref as J  # noqa: E402

I32 = np.int32
KINDS = J.KINDS
SIZES = [(1, 5), (7, 9), (8, 8), (16, 16), (18, 34), (24, 24), (31, 33), (40, 56), (50, 70), (35, 277), (97, 131)]
TINY = [(1, 1), (3, 2), (2, 4)]
QUALITIES = (1, 50, 75, 100)
SCAN_GROUP = 16                    # MCUs per partial sum of the device's bit-offset scan (csrc/jpegenc.hip: kGroupMcus)
HEADER_BYTES = 623

# ITU T.81 Annex K.3 - K.6: per table the number of codes of each length 1..16, then the symbols in code order
DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), (
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa))
AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), (
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa))


def _zigzag():
    """natural (row-major) index of zigzag position k"""
    order = sorted(range(64), key=lambda n: (n // 8 + n % 8, (n // 8 if (n // 8 + n % 8) % 2 else n % 8)))
    return np.array(order, dtype=np.int64)


ZIGZAG = _zigzag()


def codes(spec):
    """(counts per length, symbols) -> {symbol: (code, length)}: the canonical assignment of T.81 Annex C"""
    counts, symbols = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    assert k == len(symbols)
    return out


_DC = (codes(DC_LUMA), codes(DC_CHROMA))
_AC = (codes(AC_LUMA), codes(AC_CHROMA))


def plan(h, w):
    """what cidnet_jpeg_encode_plan reports, restated: MCU columns / rows, luma block columns / rows, dummy blocks, the
    number of partial sums of the bit-offset scan, and the slot capacity (a real block at most 22 + 63 * 26 = 1660 bits, a
    dummy 6; bytes doubled for stuffing, + 2, rounded up to 4)"""
    mc, mr, bw, bh = -(-w // 16), -(-h // 16), -(-w // 8), -(-h // 8)
    dummies = 4 * mc * mr - bw * bh
    bits = (bw * bh + 2 * mc * mr) * 1660 + dummies * 6
    return dict(mcu_cols=mc, mcu_rows=mr, block_cols=bw, block_rows=bh, dummies=dummies, groups=-(-(mc * mr) // SCAN_GROUP),
                capacity=(2 * ((bits + 7) // 8) + 2 + 3) // 4 * 4)


def _quantised(plane, table):
    """samples (H,W), multiples of 8 -> the quantised coefficients (H/8, W/8, 64) in zigzag order"""
    b = J._blocks(plane.astype(I32) - I32(128))
    b = J._fdct_1d(b, True)
    b = J._fdct_1d(b.swapaxes(-1, -2), False).swapaxes(-1, -2)
    div = table << 3
    c = (np.sign(b) * ((np.abs(b) + (div >> 1)) // div)).astype(I32)
    return c.reshape(*c.shape[:2], 64)[..., ZIGZAG]


def coefficients(img, quality=75):
    """uint8 (3,h,w) -> (y, cb, cr): zigzag coefficients (2 mr, 2 mc, 64) of luma over whole MCUs (a block past ceil(h/8) x
    ceil(w/8) is NOT what the file holds: scan() replaces it) and (mr, mc, 64) of each chroma plane"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[0] == 3, (img.dtype, img.shape)
    _, h, w = img.shape
    H, W = -(-h // 16) * 16, -(-w // 16) * 16
    ch = (h + 1) // 2
    r, g, b = (img[i].astype(I32) for i in range(3))
    y = (I32(J._fix(.299)) * r + I32(J._fix(.587)) * g + I32(J._fix(.114)) * b + I32(32768)) >> 16
    off = I32((128 << 16) + 32767)
    cb = (I32(-J._fix(.16874)) * r - I32(J._fix(.33126)) * g + I32(J._fix(.5)) * b + off) >> 16
    cr = (I32(J._fix(.5)) * r - I32(J._fix(.41869)) * g - I32(J._fix(.08131)) * b + off) >> 16
    tl, tc = J.tables(quality)
    out = [_quantised(J._edge(y, H, W), tl)]
    bias = np.tile(np.array([1, 2], dtype=I32), W // 4)
    for c in (cb, cr):
        c = J._edge(c, 2 * ch, W)
        d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        out.append(_quantised(J._edge(d, H // 2, W // 2), tc))
    return tuple(out)


def _value_bits(v, s):
    return (v if v >= 0 else v - 1) & ((1 << s) - 1)


def scan(img, quality=75):
    """uint8 (3,h,w) -> (the entropy-coded bytes between SOS and EOI, counters): counters holds zrl (ZRL codes), no_eob
    (blocks whose coefficient 63 is non-zero), stuffed (0x00 bytes inserted), dummies, dc_cat and ac_cat (the largest
    categories met) and bits (the length before padding and stuffing)"""
    _, h, w = np.asarray(img).shape
    p = plan(h, w)
    y, cb, cr = (c.tolist() for c in coefficients(img, quality))
    n = dict(zrl=0, no_eob=0, stuffed=0, dummies=0, dc_cat=0, ac_cat=0, bits=0)
    pred = [0, 0, 0]
    parts = []

    def put(code, length):
        parts.append(format(code, "0%db" % length) if length else "")

    def block(c, comp, tab):
        diff = c[0] - pred[comp]
        pred[comp] = c[0]
        s = abs(diff).bit_length()
        n["dc_cat"] = max(n["dc_cat"], s)
        put(*_DC[tab][s])
        put(_value_bits(diff, s), s)
        run = 0
        for k in range(1, 64):
            v = c[k]
            if v == 0:
                run += 1
                continue
            for _ in range(run >> 4):
                put(*_AC[tab][0xF0])
                n["zrl"] += 1
            s = abs(v).bit_length()
            n["ac_cat"] = max(n["ac_cat"], s)
            put(*_AC[tab][((run & 15) << 4) | s])
            put(_value_bits(v, s), s)
            run = 0
        if c[63] == 0:
            put(*_AC[tab][0x00])
        else:
            n["no_eob"] += 1

    for my in range(p["mcu_rows"]):
        for mx in range(p["mcu_cols"]):
            for by, bx in ((2 * my, 2 * mx), (2 * my, 2 * mx + 1), (2 * my + 1, 2 * mx), (2 * my + 1, 2 * mx + 1)):
                if by < p["block_rows"] and bx < p["block_cols"]:
                    block(y[by][bx], 0, 0)
                else:                                                 # a dummy: the DC of the block before it, no AC
                    n["dummies"] += 1
                    block([pred[0]] + [0] * 63, 0, 0)
            block(cb[my][mx], 1, 1)
            block(cr[my][mx], 2, 1)
    bits = "".join(parts)
    n["bits"] = len(bits)
    bits += "1" * (-len(bits) % 8)
    raw = int(bits, 2).to_bytes(len(bits) // 8, "big")
    n["stuffed"] = raw.count(b"\xff")
    assert n["dummies"] == p["dummies"]
    return raw.replace(b"\xff", b"\xff\x00"), n


def _segment(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def header(h, w, quality=75):
    """the 623 bytes in front of the scan: SOI, APP0, two DQT, SOF0, four DHT, SOS"""
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    for i, t in enumerate(J.tables(quality)):
        out += _segment(0xDB, bytes([i]) + bytes(t.reshape(64)[ZIGZAG].astype(np.uint8).tolist()))
    out += _segment(0xC0, struct.pack(">BHHB", 8, h, w, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, spec in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, bytes([tc_th]) + bytes(spec[0]) + bytes(spec[1]))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    assert len(out) == HEADER_BYTES
    return out


def jpeg_file(img, quality=75):
    """-> (the whole file, counters)"""
    _, h, w = np.asarray(img).shape
    data, n = scan(img, quality)
    return header(h, w, quality) + data + b"\xff\xd9", n


def pil_file(img, quality=75):
    """uint8 (3,h,w) -> the bytes Pillow writes at its defaults (4:2:0, baseline, the standard tables)"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(np.asarray(img).transpose(1, 2, 0))).save(buf, "JPEG", quality=int(quality))
    return buf.getvalue()


def checkerboard_pixels():
    """16 x 16, alternating pixels at 0 / 255: the largest AC coefficient an 8-bit block can hold"""
    a = np.zeros((16, 16), dtype=np.uint8)
    a[::2, ::2] = 255
    a[1::2, 1::2] = 255
    return np.ascontiguousarray(np.broadcast_to(a, (3, 16, 16)))


def checkerboard_blocks():
    """16 x 32, alternating 8 x 8 blocks at 0 / 255: the largest DC difference"""
    yy, xx = np.mgrid[0:16, 0:32]
    a = ((((yy >> 3) + (xx >> 3)) & 1) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(a, (3, 16, 32)))


def case_image(kind, h, w, quality=75):
    """the image of a named case, the same in every test file (the quality sweep at 50 x 70 is seeded by its quality, as
    tests/test_jpeg_cpu.py seeds its own)"""
    if kind == "checker_pixels":
        return checkerboard_pixels()
    if kind == "checker_blocks":
        return checkerboard_blocks()
    return J.image(kind, h, w, 1000 * h + w if quality == 75 else quality)


def cases():
    """every (kind, h, w, quality) of the contract's list"""
    out = [(k, h, w, 75) for h, w in SIZES for k in KINDS]
    out += [("random", 50, 70, q) for q in (1, 50, 100)]
    out += [("random", h, w, 75) for h, w in TINY]
    out += [("checker_pixels", 16, 16, 100), ("checker_blocks", 16, 32, 100)]
    return out
