"""The oracle of the JPEG round-trip tests (tests/test_jpeg_cpu.py, tests/test_jpeg_gpu.py, tests/test_evaluate_roundtrip_gpu.py).

pil_roundtrip() IS the oracle: Pillow's Image.save(buf, 'JPEG', quality=q) followed by Image.open(buf), what eval.py's output
file decodes to.  roundtrip() restates the lossy stages of that file in numpy int32 (colour conversion, 4:2:0
downsampling, libjpeg's "islow" forward DCT, quantise / dequantise with the scaled Annex K tables, the islow inverse DCT,
"fancy" h2v2 upsampling, colour conversion back); the entropy coder is lossless and is left out.  test_jpeg_cpu.py pins the
restatement to Pillow, so a disagreement is a mistake of the restatement, never of Pillow.  Widths under 5 are out of scope
(the decoder's first / last column cases on a chroma plane narrower than three samples read padded columns).
Images are planar uint8 (3,h,w); all arithmetic is np.int32 and >> is an arithmetic shift."""
import io

import numpy as np

I32 = np.int32
QUALITIES = (1, 50, 100)
KINDS = ("random", "saturated", "ramp", "constant")
CASES = [(1, 5), (7, 9), (8, 8), (15, 17), (16, 16), (18, 34), (24, 24), (31, 33), (40, 56), (50, 70), (64, 96), (97, 131)]
# more MCU columns than one workgroup of pass A takes (8), and three MCU rows: cidnet_metric_jpeg_plan reports 3 x 3 workgroups
WIDE = (35, 277)

# Annex K.1 / K.2 of the JPEG standard, in natural (row-major) order
STD_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=I32).reshape(8, 8)
STD_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                       47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, dtype=I32).reshape(8, 8)


def _fix(x):
    return int(x * 65536 + 0.5)


def tables(quality):
    """-> (luma, chroma) int32 (8,8): the Annex K tables scaled as jpeg_set_quality scales them"""
    q = int(quality)
    assert 1 <= q <= 100, q
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((std * s + 50) // 100, 1, 255).astype(I32) for std in (STD_LUMA, STD_CHROMA))


def _descale(x, n):
    return (x + I32(1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """libjpeg jfdctint.c, one pass along the last axis of d (..., 8) int32"""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[0], out[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * I32(4433)
    out[2] = _descale(z1 + t13 * I32(6270), n)
    out[6] = _descale(z1 - t12 * I32(15137), n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * I32(9633)
    t4, t5, t6, t7 = t4 * I32(2446), t5 * I32(16819), t6 * I32(25172), t7 * I32(12299)
    z1, z2, z3, z4 = z1 * I32(-7373), z2 * I32(-20995), z3 * I32(-16069) + z5, z4 * I32(-3196) + z5
    out[7], out[5] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n)
    out[3], out[1] = _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def _idct_1d(c, n):
    """libjpeg jidctint.c, one pass along the last axis of c (..., 8) int32, descaled by n"""
    c = [c[..., i] for i in range(8)]
    z1 = (c[2] + c[6]) * I32(4433)
    t2, t3 = z1 - c[6] * I32(15137), z1 + c[2] * I32(6270)
    t0, t1 = (c[0] + c[4]) << 13, (c[0] - c[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = c[7], c[5], c[3], c[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * I32(9633)
    t0, t1, t2, t3 = t0 * I32(2446), t1 * I32(16819), t2 * I32(25172), t3 * I32(12299)
    z1, z2, z3, z4 = z1 * I32(-7373), z2 * I32(-20995), z3 * I32(-16069) + z5, z4 * I32(-3196) + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([_descale(v, n) for v in out], axis=-1)


def _blocks(plane):
    """(H,W), both multiples of 8 -> (H/8, W/8, 8, 8)"""
    H, W = plane.shape
    return plane.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)


def _unblocks(b):
    nh, nw = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(nh * 8, nw * 8)


def _codec(plane, table):
    """uint8 samples (H,W) as int32 -> what the decoder's inverse DCT gives back, int32 in 0..255"""
    b = _blocks(plane.astype(I32) - I32(128))
    b = _fdct_1d(b, True)                                              # rows
    b = _fdct_1d(b.swapaxes(-1, -2), False).swapaxes(-1, -2)           # columns
    div = table << 3
    c = np.sign(b) * ((np.abs(b) + (div >> 1)) // div) * table
    c = _idct_1d(c.astype(I32).swapaxes(-1, -2), 11).swapaxes(-1, -2)  # columns first
    c = _idct_1d(c, 18)
    return _unblocks(np.clip(c + I32(128), 0, 255).astype(I32))


def _edge(plane, H, W):
    return np.pad(plane, ((0, H - plane.shape[0]), (0, W - plane.shape[1])), mode="edge")


def roundtrip(img, quality=75):
    """uint8 (3,h,w), w >= 5 -> uint8 (3,h,w)"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[0] == 3 and img.shape[2] >= 5, (img.dtype, img.shape)
    _, h, w = img.shape
    H, W = -(-h // 16) * 16, -(-w // 16) * 16
    ch, cw = (h + 1) // 2, (w + 1) // 2
    r, g, b = (img[i].astype(I32) for i in range(3))
    y = (I32(_fix(.299)) * r + I32(_fix(.587)) * g + I32(_fix(.114)) * b + I32(32768)) >> 16
    off = I32((128 << 16) + 32767)
    cb = (I32(-_fix(.16874)) * r - I32(_fix(.33126)) * g + I32(_fix(.5)) * b + off) >> 16
    cr = (I32(_fix(.5)) * r - I32(_fix(.41869)) * g - I32(_fix(.08131)) * b + off) >> 16
    tl, tc = tables(quality)
    planes = [_codec(_edge(y, H, W), tl)[:h, :w]]
    bias = np.tile(np.array([1, 2], dtype=I32), W // 4)
    for c in (cb, cr):
        c = _edge(c, 2 * ch, W)                                        # right to the MCU, one row down if h is odd
        d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        planes.append(_codec(_edge(d, H // 2, W // 2), tc)[:ch, :cw])  # the DOWNSAMPLED rows are replicated to 8
    yy, (cb, cr) = planes[0], (_upsample(p)[:h, :w] - I32(128) for p in planes[1:])
    out = np.stack([yy + ((I32(_fix(1.402)) * cr + I32(32768)) >> 16),
                    yy + ((I32(-_fix(.34414)) * cb - I32(_fix(.71414)) * cr + I32(32768)) >> 16),
                    yy + ((I32(_fix(1.772)) * cb + I32(32768)) >> 16)])
    return np.clip(out, 0, 255).astype(np.uint8)


def _upsample(c):
    """libjpeg's h2v2 "fancy" (triangle) upsampling of a chroma plane (ch,cw), cw >= 3 -> (2 ch, 2 cw)"""
    ch, cw = c.shape
    up = np.concatenate([c[:1], c[:-1]])
    dn = np.concatenate([c[1:], c[-1:]])
    out = np.empty((2 * ch, 2 * cw), dtype=I32)
    for k, nb in ((0, up), (1, dn)):
        s = I32(3) * c + nb
        left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)           # first column: 3 s + s = 4 s
        right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        out[k::2, 0::2] = (I32(3) * s + left + I32(8)) >> 4
        out[k::2, 1::2] = (I32(3) * s + right + I32(7)) >> 4
    return out


def pil_roundtrip(img, quality=75):
    """uint8 (3,h,w) -> uint8 (3,h,w): the file Pillow writes at its defaults (4:2:0, baseline tables), decoded again"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(np.asarray(img).transpose(1, 2, 0))).save(buf, "JPEG", quality=int(quality))
    buf.seek(0)
    with Image.open(buf) as im:
        return np.ascontiguousarray(np.array(im.convert("RGB")).transpose(2, 0, 1))


def image(kind, h, w, seed):
    """uint8 (3,h,w): "random" bytes; "saturated" 0 / 255 bytes (both clamps); "ramp", a smooth ramp plus +-2 noise (sparse AC
    coefficients); "constant\""""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    if kind == "saturated":
        return (rng.integers(0, 2, (3, h, w)) * 255).astype(np.uint8)
    if kind == "ramp":
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([40 + 1.5 * xx + 0.5 * yy, 200 - 1.0 * xx + 0.7 * yy, 90 + 0.3 * xx + 1.1 * yy])
        return np.clip(np.rint(base) + rng.integers(-2, 3, (3, h, w)), 0, 255).astype(np.uint8)
    if kind == "constant":
        return np.broadcast_to(rng.integers(0, 256, (3, 1, 1), dtype=np.uint8), (3, h, w)).copy()
    raise ValueError(kind)
