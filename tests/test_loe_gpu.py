"""GPU: LOE on the device (csrc/loe.hip through metrics.loe_counts / loe / evaluate_unpaired(loe=True)) against the oracle of
tests/loe_ref.py.  The value is a ratio of integers: every comparison is exact -- int64 `num` equal to the oracle's count, and
loe equal to num / m in fp64."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loe_ref as R  # noqa: E402
from evaluate_harness import in_child as _in_child, model as _model  # noqa: E402

pytestmark = pytest.mark.gpu
PARAMS = os.path.join(HERE, "golden", "niqe_pris_params.npz")


def _rand(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _check(dev, low, out, sample, want=None):
    """low, out: uint8 numpy (3,h,w) or (B,3,h,w), or device tensors of that layout -> num as a list; asserts num and both
    forms of the value against the oracle (or `want`, a list of counts)"""
    from hvi_cidnet_amd import metrics as M
    a = torch.from_numpy(np.ascontiguousarray(low)).to(dev) if isinstance(low, np.ndarray) else low
    b = torch.from_numpy(np.ascontiguousarray(out)).to(dev) if isinstance(out, np.ndarray) else out
    num, m = M.loe_counts(a, b, sample)
    val = M.loe(a, b, sample)
    nrm = M.loe(a, b, sample, normalized=True)
    assert num.dtype == torch.int64 and val.dtype == torch.float64 and num.device == a.device
    ha, hb = a.cpu().numpy(), b.cpu().numpy()
    if ha.ndim == 3:
        ha, hb = ha[None], hb[None]
    assert num.shape == (ha.shape[0],) and val.shape == num.shape
    if want is None:
        refs = [R.brute(x, y, sample) for x, y in zip(ha, hb)]
        want = [r[0] for r in refs]
        assert all(r[1] == m for r in refs)
    got = num.cpu().tolist()
    print("loe num:", got, "oracle:", want, "m:", m)
    assert got == want
    assert val.cpu().tolist() == [n / m for n in want]
    assert nrm.cpu().tolist() == [n / float(m * m) for n in want]
    return got


def _plan(h, w, step):
    from hvi_cidnet_amd import _lib
    buf = (ctypes.c_int * 6)()
    assert _lib.lib().raw("cidnet_metric_loe_plan")(h, w, step, buf, 6) == 0
    return dict(zip(("rows", "cols", "blocks", "per_block", "bits", "lds"), buf))


def test_degenerate_cases(dev):
    one = _rand(1, 3, 1, 1)
    assert _check(dev, one, _rand(2, 3, 1, 1), None) == [0]                # a single sample: U = 1 on both sides
    assert _check(dev, one, one, 50) == [0]
    low = _rand(3, 3, 33, 67)
    t = torch.from_numpy(low).to(dev)
    assert _check(dev, t, t, None) == [0]                                  # out is low
    half = low // 2                                                        # levels 0..127: a strictly increasing lut on
    lut = (np.arange(256) * 2 + (np.arange(256) > 40)).clip(0, 255).astype(np.uint8)     # them need not be the identity
    assert (np.diff(lut[:128].astype(int)) > 0).all() and (lut[half] != half).any()
    assert _check(dev, half, lut[half], None) == [0]                       # it keeps every order, ties included
    ramp = np.repeat((np.arange(48 * 80).reshape(1, 48, 80) * 255 // (48 * 80 - 1)).astype(np.uint8), 3, axis=0)
    got = _check(dev, ramp, 255 - ramp, None)                              # the grey ramp reversed, against brute force
    assert got[0] > 0


def test_channel_max(dev):
    """each channel in turn carries the maximum, 0 and 255 present: a kernel that read one channel, or summed them, fails"""
    h, w = 24, 40
    for c in range(3):
        low, out = _rand(10 + c, 3, h, w) // 3, _rand(20 + c, 3, h, w) // 3              # the others stay below 86
        low[c] = 86 + _rand(30 + c, h, w) // 2
        out[(c + 1) % 3] = 86 + _rand(40 + c, h, w) // 2
        low[c, 0, 0], low[c, 5, 7], low[:, 3, 3] = 255, 255, 0
        out[(c + 1) % 3, 1, 1], out[:, 9, 9] = 255, 0
        assert low.max(axis=0).min() == 0 and low.max() == 255 and out.max(axis=0).min() == 0 and out.max() == 255
        _check(dev, low, out, None)


@pytest.mark.parametrize("h,w", [(7, 13), (33, 67), (50, 78)])
def test_tails_and_addressing(dev, h, w):
    low, out = _rand(h, 3, h, w), _rand(w, 3, h, w)
    want = _check(dev, low, out, None)
    _check(dev, low, out, 5)
    # the same images inside a larger byte buffer, at an odd byte offset
    n = 3 * h * w
    buf = torch.zeros(2 * n + 64, dtype=torch.uint8, device=dev)
    buf[13:13 + n] = torch.from_numpy(low).to(dev).reshape(-1)
    ob = (n + 30) | 1
    buf[ob:ob + n] = torch.from_numpy(out).to(dev).reshape(-1)
    a, b = buf[13:13 + n].view(3, h, w), buf[ob:ob + n].view(3, h, w)
    assert a.data_ptr() % 2 == 1 and b.data_ptr() % 2 == 1 and a.is_contiguous()
    assert _check(dev, a, b, None, want) == want
    # a non-contiguous view: the middle of a wider and taller image, and a channel-last one
    big = torch.from_numpy(_rand(5, 3, h + 4, w + 6)).to(dev)
    big[:, 1:1 + h, 3:3 + w] = torch.from_numpy(low).to(dev)
    va = big[:, 1:1 + h, 3:3 + w]
    vb = torch.from_numpy(np.ascontiguousarray(out.transpose(1, 2, 0))).to(dev).permute(2, 0, 1)
    assert not va.is_contiguous() and not vb.is_contiguous()
    assert _check(dev, va, vb, None, want) == want


@pytest.mark.parametrize("h,w,step", [(101, 157, 2), (149, 100, 2), (30, 40, 1)])
def test_stride_reads_the_grid_only(dev, h, w, step):
    from hvi_cidnet_amd import metrics as M
    assert M.loe_grid(h, w, 50)[0] == step
    low, out = _rand(h + 1, 3, h, w), _rand(w + 1, 3, h, w)
    want = _check(dev, low, out, 50)
    if step > 1:                                                           # poison every pixel off the sampling grid
        _, rows, cols = M.loe_grid(h, w, 50)
        on = np.zeros((h, w), bool)
        on[:rows * step:step, :cols * step:step] = True
        assert on.sum() == rows * cols < h * w
        low2, out2 = low.copy(), out.copy()
        low2[:, ~on] = _rand(7, 3, int((~on).sum()))
        out2[:, ~on] = _rand(8, 3, int((~on).sum()))
        assert (low2 != low).any() and (out2 != out).any()
        assert _check(dev, low2, out2, 50, want) == want


def test_batch_isolation_and_workspace_reuse(dev):
    from hvi_cidnet_amd import _lib, ops
    h, w = 33, 67
    low, out = _rand(50, 3, 3, h, w), _rand(51, 3, 3, h, w)
    out[1] = low[1]                                                        # image 1 scores 0 between two that do not
    low[2] //= 4
    batch = _check(dev, low, out, None)
    singles = [_check(dev, low[i], out[i], None)[0] for i in range(3)]
    assert batch == singles and batch[1] == 0 and batch[0] > 0 and batch[2] > 0
    # the C entry point twice on ONE workspace, other data the second time: the bins are zeroed inside the call
    L = _lib.lib()
    nws = L.raw("cidnet_metric_loe_ws_bytes")(3)
    ws = torch.full((nws,), 0xA5, dtype=torch.uint8, device=dev)           # starts dirty
    num, val = torch.empty(3, dtype=torch.int64, device=dev), torch.empty(3, dtype=torch.float64, device=dev)
    for a, b in ((low, out), (out[::-1].copy(), low)):
        ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        L.call("cidnet_metric_loe_u8", ops._p(ta), ops._p(tb), 3, h, w, 1, ops._p(num), ops._p(val), ops._p(ws), nws, ops._stream())
        want = [R.brute(x, y, None)[0] for x, y in zip(a, b)]
        assert num.cpu().tolist() == want and val.cpu().tolist() == [n / (h * w) for n in want]
    with pytest.raises(RuntimeError, match="CIDNET_ERR_WS"):
        L.call("cidnet_metric_loe_u8", ops._p(ta), ops._p(tb), 3, h, w, 1, ops._p(num), ops._p(val), ops._p(ws), nws - 1, ops._stream())


def test_contention_and_the_counter_cap(dev):
    """256 x 257 at full resolution: m = 65792 samples, more than a 16-bit counter holds, nearly all in one or two bins"""
    h, w = 256, 257
    m = h * w
    p = _plan(h, w, 1)
    assert p["rows"] * p["cols"] == m > 65535
    assert p["blocks"] > 1 and p["per_block"] < 2 ** p["bits"] and p["blocks"] * p["per_block"] >= m, p
    low = np.full((3, h, w), 77, np.uint8)
    out = np.full((3, h, w), 5, np.uint8)
    out.reshape(3, -1)[:, m // 2:] = 200
    want = (m // 2) * (m - m // 2)
    assert want == 1082146816 == R.by_hist(low, out, None)[0]
    assert _check(dev, low, out, None, [want]) == [want]
    assert _check(dev, low, np.full((3, h, w), 9, np.uint8), None, [0]) == [0]           # everything in one bin
    low2, out2 = _rand(60, 3, h, w), _rand(61, 3, h, w)                                   # and spread over all bins
    _check(dev, low2, out2, None, [R.by_hist(low2, out2, None)[0]])


def test_invalid_arguments(dev):
    from hvi_cidnet_amd import metrics as M
    a = torch.zeros((2, 3, 8, 8), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        M.loe(a, a[:1])
    with pytest.raises(ValueError):
        M.loe(a, a[..., :7])
    with pytest.raises(ValueError):
        M.loe(a, a.float())
    with pytest.raises(ValueError):
        M.loe(a[:, :2], a[:, :2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.loe(a, a.cpu())


def test_determinism(dev):
    from hvi_cidnet_amd import metrics as M
    a, b = torch.from_numpy(_rand(70, 2, 3, 64, 96)).to(dev), torch.from_numpy(_rand(71, 2, 3, 64, 96)).to(dev)
    n1, _ = M.loe_counts(a, b, None)
    v1 = M.loe(a, b, None)
    n2, _ = M.loe_counts(a, b, None)
    v2 = M.loe(a, b, None)
    assert torch.equal(n1, n2) and torch.equal(v1, v2) and int(n1[0]) > 0
    assert n1.cpu().tolist() == [R.brute(x, y, None)[0] for x, y in zip(a.cpu().numpy(), b.cpu().numpy())]


# ---- evaluate_unpaired(loe=True): in a fresh spawned process, as in tests/test_evaluate_unpaired_gpu.py ------------------
SIZES = [(104, 120), (104, 120), (96, 136)]
GAMMA = 0.8


def _images():
    rng = np.random.default_rng(12)
    out = []
    for h, w in SIZES:
        yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
        base = np.stack([0.3 + 0.25 * np.sin(9 * xx + c) * np.cos(7 * yy - c) for c in range(3)])
        out.append(torch.from_numpy(np.clip(base + rng.normal(0, 0.05, (3, h, w)), 0.0, 1.0).astype(np.float32)))
    return out


def _bits(values):
    return np.array(values, dtype=np.float64).view(np.uint64).tolist()


def test_evaluate_unpaired_with_loe(dev):
    _in_child(_case_evaluate)


def _case_evaluate():
    import hvi_cidnet_amd as P
    M = P.metrics
    m = _model()
    images = _images()
    prm = P.load_niqe_params(PARAMS)
    plain = P.evaluate_unpaired(m, images, prm, alpha=0.9, gamma=GAMMA, batch_size=2)
    with_loe = P.evaluate_unpaired(m, images, prm, alpha=0.9, gamma=GAMMA, batch_size=2, loe=True)
    assert math.isnan(plain.loe) and "loe" not in plain.per_image and list(plain.per_image) == ["niqe"]
    # bit-identical, NaN included: images of one 96 x 96 block have no NIQE (fewer than two blocks: metrics.niqe_score)
    assert _bits(with_loe.per_image["niqe"]) == _bits(plain.per_image["niqe"]) and _bits([with_loe.niqe]) == _bits([plain.niqe])

    def chain(alpha):
        """the hand-written chain, one image at a time -> the oracle's LOE per image"""
        t = m.trans
        old = (m.training, t.gated2, t.alpha)
        m.eval()
        t.gated2, t.alpha = True, alpha
        vals = []
        with torch.no_grad():
            for img in images:
                x = img.cuda()
                xp, (h, w) = P.pad_to_multiple(x.unsqueeze(0), 8)
                q = M.to_uint8(m(xp ** GAMMA), (h, w))[0]
                num, n = R.brute(M.to_uint8(x).cpu().numpy(), q.cpu().numpy(), 50)             # the input as supplied
                assert n == M.loe_grid(h, w, 50)[1] * M.loe_grid(h, w, 50)[2]
                vals.append(num / n)
        m.train(old[0])
        t.gated2, t.alpha = old[1:]
        return vals
    want = chain(0.9)
    print("loe per image:", with_loe.per_image["loe"], "oracle:", want)
    assert with_loe.per_image["loe"] == want and min(want) > 0
    acc = 0.0
    for v in want:
        acc += v
    assert with_loe.loe == acc / len(want)
    sweep = P.evaluate_unpaired(m, images, prm, alpha=[0.9, 0.6], gamma=GAMMA, batch_size=2, loe=True)
    assert len(sweep) == 2 and [r.alpha for r in sweep] == [0.9, 0.6]
    assert sweep[0].per_image["loe"] == with_loe.per_image["loe"] and sweep[0].loe == with_loe.loe
    assert _bits(sweep[0].per_image["niqe"]) == _bits(plain.per_image["niqe"]) and sweep[0].names == with_loe.names
    assert sweep[1].per_image["loe"] == chain(0.6)
    assert sweep[1].per_image["loe"] != sweep[0].per_image["loe"]
    assert P.evaluate_unpaired(m, images, prm, alpha=0.9, gamma=GAMMA, batch_size=2, loe=True, loe_sample=None).per_image["loe"] \
        != want
    assert m.training
