"""The PNG writer's stream contract, restated in numpy: interleaved uint8 (h,w,3) -> the complete zlib stream
of one IDAT chunk -- per-row filters, then one dynamic-Huffman deflate block per segment of whole rows, literals only (no
LZ77), every choice the format leaves open pinned by one rule.  csrc/png.hip is held to these bytes; zlib.decompress and
Pillow are held to decode them.  Nothing here imports the package."""
import struct
import zlib

import numpy as np

FILTERS = ("none", "sub", "up", "avg", "paeth")
MODES = ("adaptive",) + FILTERS
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
SIZES = [(1, 1), (1, 5), (2, 3), (7, 9), (33, 47), (40, 56), (17, 300), (64, 96)]
KINDS = ("grain", "random", "constant", "saturated", "ramp")
SEGMENTS = (32768, 512)
HEADER_BITS_MAX = 17 + 19 * 3 + 259 * 7                          # what a block's header can take at most


# ---- images --------------------------------------------------------------------------------------------------------------
def scene(h, w, sigma, seed):
    """a smooth scene (low-frequency cosines per channel) with Gaussian grain of the given sigma, uint8 (h,w,3)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((h, w, 3))
    for c in range(3):
        a, b, p = rng.uniform(0.5, 2.5, 3)
        img[..., c] = 128 + 70 * np.cos(a * np.pi * y / max(h, 2) + p) * np.cos(b * np.pi * x / max(w, 2)) + 30 * np.sin((x + y) / 17.0 + c)
    img += rng.normal(0.0, sigma, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def image(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == "grain":
        return scene(h, w, 4.0, seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "constant":
        return np.full((h, w, 3), 77, np.uint8)
    if kind == "saturated":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    if kind == "ramp":
        return np.broadcast_to((np.arange(w) * 255 // max(w - 1, 1)).astype(np.uint8)[None, :, None], (h, w, 3)).copy()
    raise ValueError(kind)


def fibonacci_image():
    """48 x 47 pixels (one segment of 48 * 142 bytes under filter none) whose byte counts follow Fibonacci numbers, filled up
    with the most frequent value: the unlimited Huffman tree is deeper than 15"""
    h, w = 48, 47
    fib = [1, 2]                                                 # the end of block is the sequence's first 1
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    vals = []
    for i, c in enumerate(fib):                                  # the value 0 is the symbol of count 55: 48 type bytes + 7
        vals.append(np.full(c - h, 0, np.uint8) if c == 55 else np.full(c, 10 + i, np.uint8))
    vals = np.concatenate(vals)
    n = h * w * 3
    assert len(vals) < n
    data = np.concatenate([vals, np.full(n - len(vals), 10 + len(fib) - 1, np.uint8)])
    np.random.default_rng(5).shuffle(data)
    return data.reshape(h, w, 3)


# ---- filtering -----------------------------------------------------------------------------------------------------------
def _candidates(img):
    """-> uint8 (5,h,3w): every row under every filter type, from the raw neighbours"""
    h, w, _ = img.shape
    x = img.reshape(h, 3 * w).astype(np.int32)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - pred]).astype(np.uint8)


def filter_rows(img, mode="adaptive"):
    """-> (types uint8 (h,), filtered uint8 (h, 1 + 3w)): row = type byte + filtered bytes"""
    cand = _candidates(img)
    h = img.shape[0]
    if mode == "adaptive":
        v = cand.astype(np.int64)
        types = np.argmin(np.minimum(v, 256 - v).sum(axis=2), axis=0).astype(np.uint8)   # argmin: the first (lowest) minimum
    else:
        types = np.full(h, FILTERS.index(mode), np.uint8)
    rows = cand[types, np.arange(h)]
    return types, np.concatenate([types[:, None], rows], axis=1)


def unfilter_reference(filtered, h, w):
    """what a PNG decoder does with the filtered bytes (used to cross-check the filters without Pillow)"""
    out = np.zeros((h, 3 * w), np.int32)
    for y in range(h):
        t, row = filtered[y, 0], filtered[y, 1:].astype(np.int32)
        up = out[y - 1] if y else np.zeros(3 * w, np.int32)
        for i in range(3 * w):
            a = out[y, i - 3] if i >= 3 else 0
            b = up[i]
            c = up[i - 3] if i >= 3 else 0
            if t == 0:
                pr = 0
            elif t == 1:
                pr = a
            elif t == 2:
                pr = b
            elif t == 3:
                pr = (a + b) >> 1
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pr = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            out[y, i] = (row[i] + pr) & 255
    return out.astype(np.uint8).reshape(h, w, 3)


# ---- the code-length procedure -------------------------------------------------------------------------------------------
def tree_depths(counts):
    """counts: {symbol: count > 0}, two or more -> {symbol: depth}: sort by (count, symbol), two-queue merge (leaves in that
    order, internal nodes in creation order; the smaller head, the leaf on equal weight), depth = length"""
    order = sorted(counts, key=lambda s: (counts[s], s))
    m = len(order)
    wt = [counts[s] for s in order] + [0] * (m - 1)
    par = [0] * (2 * m - 1)
    li, ni = 0, m
    for nn in range(m, 2 * m - 1):
        pair = []
        for _ in range(2):
            if li < m and (ni >= nn or wt[li] <= wt[ni]):
                pair.append(li)
                li += 1
            else:
                pair.append(ni)
                ni += 1
        wt[nn] = wt[pair[0]] + wt[pair[1]]
        par[pair[0]] = par[pair[1]] = nn
    depth = [0] * (2 * m - 1)
    for i in range(2 * m - 3, -1, -1):
        depth[i] = depth[par[i]] + 1
    return {s: depth[i] for i, s in enumerate(order)}


def code_lengths(freq, maxbits):
    """freq: counts per symbol -> lengths per symbol (0: unused), none above maxbits"""
    counts = {s: int(c) for s, c in enumerate(freq) if c > 0}
    lens = [0] * len(freq)
    if len(counts) == 1:
        lens[next(iter(counts))] = 1
        return lens
    if not counts:
        return lens
    while True:
        d = tree_depths(counts)
        if max(d.values()) <= maxbits:
            break
        counts = {s: (c + 1) >> 1 for s, c in counts.items()}
    for s, v in d.items():
        lens[s] = v
    return lens


def canonical_codes(lens):
    """RFC 1951 3.2.2 -> the codes bit-reversed (deflate packs Huffman codes MSB first into an LSB-first stream)"""
    mx = max(lens)
    bl = [0] * (mx + 2)
    for v in lens:
        if v:
            bl[v] += 1
    nxt, code = [0] * (mx + 2), 0
    for bits in range(1, mx + 1):
        code = (code + bl[bits - 1]) << 1
        nxt[bits] = code
    out = [0] * len(lens)
    for s, v in enumerate(lens):
        if v:
            out[s] = int(format(nxt[v], f"0{v}b")[::-1], 2)
            nxt[v] += 1
    return out


# ---- the stream ----------------------------------------------------------------------------------------------------------
def plan(h, w, segment_bytes=32768):
    row = 1 + 3 * w
    rows = max(1, segment_bytes // row)
    segments = -(-h // rows)
    return dict(rows=rows, segments=segments, last_short=int(h % min(rows, h) != 0), row_exceeds=int(row > segment_bytes), row_bytes=row)


def _block(data, final):
    """one deflate block of the bytes `data` -> (values, bit counts) of its fields in stream order"""
    freq = np.bincount(data, minlength=257).tolist()
    freq[256] = 1
    ll = code_lengths(freq, 15)
    lcode = canonical_codes(ll)
    all_lens = ll + [1, 1]
    clfreq = np.bincount(all_lens, minlength=19).tolist()
    cl = code_lengths(clfreq, 7)
    if sum(1 for v in cl if v) == 1:
        cl[1 if cl[0] else 0] = 1
    clcode = canonical_codes(cl)
    vals = [int(final), 2, 0, 1, 15] + [cl[s] for s in CL_ORDER] + [clcode[v] for v in all_lens]
    bits = [1, 2, 5, 5, 4] + [3] * 19 + [cl[v] for v in all_lens]
    lc, ln = np.asarray(lcode, np.int64), np.asarray(ll, np.int64)
    vals = np.concatenate([np.asarray(vals, np.int64), lc[data], [lcode[256]]])
    bits = np.concatenate([np.asarray(bits, np.int64), ln[data], [ll[256]]])
    return vals, bits


def _pack(vals, bits):
    """fields, LSB first each, concatenated -> (bytes padded with zero bits, total bits)"""
    total = int(bits.sum())
    start = np.cumsum(bits) - bits
    idx = np.repeat(np.arange(len(bits)), bits)
    k = np.arange(total) - np.repeat(start, bits)
    stream = ((np.repeat(vals, bits) >> k) & 1).astype(np.uint8)
    stream = np.concatenate([stream, np.zeros(-total % 8, np.uint8)])
    del idx
    return np.packbits(stream, bitorder="little").tobytes(), total


def zlib_stream(img, mode="adaptive", segment_bytes=32768, info=None):
    """uint8 (h,w,3) -> the zlib stream (bytes).  info: a dict that receives the filtered bytes and the bit count"""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and mode in MODES and segment_bytes >= 1
    h, w, _ = img.shape
    _, filt = filter_rows(img, mode)
    p = plan(h, w, segment_bytes)
    vals, bits = [], []
    for s in range(p["segments"]):
        v, b = _block(filt[s * p["rows"]:(s + 1) * p["rows"]].reshape(-1), s == p["segments"] - 1)
        vals.append(v)
        bits.append(b)
    body, total = _pack(np.concatenate(vals), np.concatenate(bits))
    raw = filt.tobytes()
    if info is not None:
        info.update(filtered=raw, bits=total)
    return b"\x78\x01" + body + struct.pack(">I", zlib.adler32(raw))


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))


def png_file(h, w, stream):
    """signature, IHDR (8-bit RGB, no interlace), one IDAT, IEND"""
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", bytes(stream))
            + _chunk(b"IEND", b""))


def capacity(h, w, segment_bytes=32768):
    """the proven size bound of one stream, restated: per segment of n symbols (its bytes and the end of
    block) the header and 9 n bits where the limiter cannot run (n < 2584: a Huffman tree deeper than 15 needs a total count of
    at least F(18) = 2584), 11 n bits otherwise; 2 + 4 bytes of framing; rounded up to whole dwords"""
    p = plan(h, w, segment_bytes)
    bits = 0
    for s in range(p["segments"]):
        n = min(p["rows"], h - s * p["rows"]) * p["row_bytes"] + 1
        bits += HEADER_BITS_MAX + (9 if n < 2584 else 11) * n
    return (2 + (bits + 7) // 8 + 4 + 3) // 4 * 4
