"""Shared by tests/test_tensor_stats_cpu.py and tests/test_tensor_stats_gpu.py: the fixture of the per-tensor statistics
(csrc/tensor_stats.hip) and two straightforward fp64 statements of its four columns, one in numpy and one in torch."""
import numpy as np
import torch

LENS = [1, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 4095, 4096, 4097, 8191, 8192, 8193, 12289]
BAND = 64                                                # NaN guard band before the first and after the last segment
I4097, I8193 = LENS.index(4097), LENS.index(8193)


def layout(gaps):
    """offsets of the segments from the buffer's start: back to back, or with gaps of 1, 2, 3, 1, ... elements"""
    off, at = [], BAND
    for i, c in enumerate(LENS):
        off.append(at)
        at += c + ((1 + i % 3) if gaps else 0)
    return off, at + BAND


def fixture(gaps, shift, planted=False):
    """-> (buf, off, lens): buf a float32 view that starts `shift` elements into a NaN-filled allocation (so its base
    pointer has 16-byte phase 4 * shift), the segments written with seeded normal values; planted: the special values of
    plant_all()"""
    off, n = layout(gaps)
    full = np.full(n + 3, np.nan, dtype=np.float32)
    assert full.size < 80000
    buf = full[shift:shift + n]
    rng = np.random.default_rng(7)
    for o, c in zip(off, LENS):
        buf[o:o + c] = rng.standard_normal(c).astype(np.float32)
    if planted:
        plant_all(buf, off)
    return buf, off, list(LENS)


def _seg(buf, off, i):
    return buf[off[i]:off[i] + LENS[i]]


def plant_all(buf, off):
    """one special case per segment, all in one buffer"""
    _seg(buf, off, 0)[:] = np.nan                        # a single element, NaN
    _seg(buf, off, 2)[:] = [1e-45, 0.0]                  # a denormal is the maximum
    _seg(buf, off, 3)[:] = -0.0
    _seg(buf, off, 7)[:] = 0.0                           # all zero
    _seg(buf, off, 9)[:] = np.nan                        # all NaN: norm 0, maxabs 0, count len, first 0
    _seg(buf, off, 10)[-1] = -100.0                      # the maximum in the last element
    _seg(buf, off, 11)[5] = 3e38                         # its square overflows fp32
    s = _seg(buf, off, I4097)                            # two in different tiles: first is the smaller index, count 2
    s[4096] = np.inf
    s[4095] = np.nan
    _seg(buf, off, I8193)[-1] = -np.inf
    _seg(buf, off, 19)[2 * 4096 + 17] = np.nan           # third tile of four
    _seg(buf, off, 19)[4096 - 1] = np.inf                # ... and the last element of the first


def planted_cases():
    """[(name, segment, {index: value})]: NaN, +Inf and -Inf at index 0, len - 1, 4095 and 4096 of the 4097- and the
    8193-element segment, one at a time"""
    out = []
    for i in (I4097, I8193):
        for pos in (0, LENS[i] - 1, 4095, 4096):
            for v in (np.nan, np.inf, -np.inf):
                out.append((f"len{LENS[i]}[{pos}]={v}", i, {pos: v}))
    return out


def stats_numpy(buf, off, lens, scale):
    s = float(np.float32(scale))
    rows = []
    for o, c in zip(off, lens):
        x = buf[o:o + c]
        fin = np.isfinite(x)
        xf = x[fin].astype(np.float64)
        bad = np.flatnonzero(~fin)
        rows.append([np.sqrt((xf * xf).sum()) * s, (float(np.abs(x[fin]).max()) if fin.any() else 0.0) * s, float(bad.size),
                     float(bad[0]) if bad.size else -1.0])
    return np.array(rows, dtype=np.float64)


def stats_torch(buf, off, lens, scale):
    """the same in torch fp64, on whatever device buf is on"""
    s = float(np.float32(scale))
    rows = []
    for o, c in zip(off, lens):
        x = buf[o:o + c]
        fin = torch.isfinite(x)
        xf = x[fin]
        bad = torch.nonzero(~fin).flatten()
        rows.append([float(xf.double().pow(2).sum().sqrt()) * s, (float(xf.abs().max()) if xf.numel() else 0.0) * s,
                     float(bad.numel()), float(bad[0]) if bad.numel() else -1.0])
    return np.array(rows, dtype=np.float64)


def check(got, want, lens):
    """maxabs, nonfinite and first exactly; the norm within (2 len + 8) 2^-53 relative -- the worst-case bound of any
    summation order on either side (len - 1 additions of exact squares each side, the square roots and the scaling)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape == (len(lens), 4)
    assert np.array_equal(got[:, 1:], want[:, 1:]), np.flatnonzero((got[:, 1:] != want[:, 1:]).any(axis=1))
    for t, c in enumerate(lens):
        assert abs(got[t, 0] - want[t, 0]) <= (2 * c + 8) * 2.0 ** -53 * want[t, 0], (t, c, got[t, 0], want[t, 0])
