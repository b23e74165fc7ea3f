"""GPU: the batch kernel's second instantiation (cidnet_augment_crop_flip_raw, csrc/augment.hip: x, gt and the un-powered
low image from one launch) bit for bit against the restatement of the reference's transform (tests/data_ref.py) and against
the plain entry point; guard bands; TrainBatches(sampling="scene", raw=True) against the restatement driven by its own plan;
ResidentPairs.from_scene_folders against PIL's bytes."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import data_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GAMMAS = (0.6, 1.2, None)                                        # None: table == NULL through crop_flip(raw=True, gamma=1.0)


def _D():
    from hvi_cidnet_amd import data
    return data


def _set(dev, sizes, seed, gt_index=None, n_high=None, groups=None):
    lows = R.random_images(seed, sizes)
    if gt_index is None:
        highs = R.random_images(seed + 1000, sizes)
    else:
        hs = [None] * n_high
        for i, k in enumerate(gt_index):
            hs[k] = sizes[i]
        highs = R.random_images(seed + 1000, hs)
    return _D().ResidentPairs(lows, highs, dev, gt_index=gt_index, groups=groups), lows, highs


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _restated(lows, highs, gt_index, rows, size, g):
    """(x, gt, raw) of the restatement: raw and gt are its gamma-off batch; x is gamma_table(g) indexed by its cropped BYTES
    (raw * 255 is exact: raw is a correctly rounded q / 255 and rounds back to q)"""
    raw, gt = R.batch(lows, highs, gt_index, *rows, size, gamma=None)
    if g is None:
        return raw, gt, raw
    q = torch.round(raw * 255).long()
    assert _same(q.float() / 255, raw)
    return torch.from_numpy(_D().gamma_table(g))[q], gt, raw


def _check(pairs, lows, highs, rows, size, gt_index=None, gammas=GAMMAS):
    D = _D()
    plain_raw, plain_gt = D.crop_flip(pairs, *rows, size, gamma=1.0)
    for g in gammas:
        x, gt, raw = D.crop_flip(pairs, *rows, size, gamma=1.0 if g is None else g, raw=True)
        wx, wgt, wraw = _restated(lows, highs, gt_index, rows, size, g)
        what = f"gamma {g} size {size} rows {rows}"
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (x, gt, raw))
        assert x.data_ptr() != raw.data_ptr()
        assert _same(raw, wraw), "raw differs from the restatement: " + what
        assert _same(gt, wgt), "gt differs from the restatement: " + what
        assert _same(x, wx), "x differs from the table of the restatement's bytes: " + what
        px, pgt = D.crop_flip(pairs, *rows, size, gamma=1.0 if g is None else g)
        assert _same(x, px) and _same(gt, pgt) and _same(raw, plain_raw) and _same(gt, plain_gt), \
            "differs from the plain entry point: " + what


def _rows(rng, sizes, size, b):
    sh, sw = (size, size) if isinstance(size, int) else size
    index = rng.integers(0, len(sizes), size=b).tolist()
    y0 = [int(rng.integers(0, sizes[i][0] - sh + 1)) for i in index]
    x0 = [int(rng.integers(0, sizes[i][1] - sw + 1)) for i in index]
    return index, y0, x0, rng.integers(0, 2, size=b).tolist(), rng.integers(0, 2, size=b).tolist()


# ---- the kernel, bit for bit ---------------------------------------------------------------------------------------------
MIXED = [(37, 51), (401, 603), (33, 49), (32, 48)]


@pytest.fixture(scope="module")
def mixed(dev):
    return _set(dev, MIXED, 41)


@pytest.mark.parametrize("b", [1, 5, 16])
def test_mixed_sizes_random_rows(dev, mixed, b):
    pairs, lows, highs = mixed
    rng = np.random.default_rng(200 + b)
    _check(pairs, lows, highs, _rows(rng, MIXED, (32, 48), b), (32, 48))
    # all four flip combinations of one window; the same low image several times in a batch
    _check(pairs, lows, highs, ([0] * 4, [3] * 4, [2] * 4, [0, 1, 0, 1], [0, 0, 1, 1]), (32, 48))


def test_every_alignment_under_every_flip(dev, mixed):
    pairs, lows, highs = mixed
    x0 = [130 + k for k in range(16)] * 4
    hf = [0] * 16 + [1] * 16 + [0] * 16 + [1] * 16
    vf = [0] * 32 + [1] * 32
    _check(pairs, lows, highs, ([1] * 64, [(7 * k) % 370 for k in range(64)], x0, hf, vf), (32, 48))


@pytest.mark.parametrize("sw", [1, 3, 33])
def test_widths_that_are_not_multiples_of_four(dev, mixed, sw):
    pairs, lows, highs = mixed
    size = (17, sw)
    rng = np.random.default_rng(sw)
    _check(pairs, lows, highs, _rows(rng, MIXED, size, 5), size)
    _check(pairs, lows, highs, ([1] * 8, [3] * 8, [200, 201, 202, 203, 570, 569, 568, 567], [0, 1] * 4, [0, 0, 1, 1] * 2), size)


def test_two_blocks_per_plane_the_second_partial(dev):
    """crop (33, 100) of a (40, 120) image: 33 * 25 = 825 groups, 512 per block"""
    sizes = [(40, 120), (40, 120)]
    pairs, lows, highs = _set(dev, sizes, 42)
    for hflip in (0, 1):
        for vflip in (0, 1):
            _check(pairs, lows, highs, ([0, 1, 1], [0, 7, 3], [0, 20, 11], [hflip] * 3, [vflip] * 3), (33, 100))


@pytest.mark.parametrize("size", [(32, 48), (31, 47), (1, 1)])
def test_windows_at_the_ends_of_the_arena(dev, size):
    """the first image at its top-left corner (mirrored: the window's last pixel is the arena's first byte) and the arena's
    last image, a ground truth, at its bottom-right corner; 3 * 40 * 64 is a multiple of 16, so the window ends with the arena"""
    sizes = [(40, 64)] * 3
    pairs, lows, highs = _set(dev, sizes, 43)
    assert pairs.layout.gt_offset(2) + 3 * 40 * 64 == pairs.layout.total_bytes == pairs.arena.numel()
    sh, sw = size
    for hflip in (0, 1):
        for vflip in (0, 1):
            _check(pairs, lows, highs, ([0, 2], [0, 40 - sh], [0, 64 - sw], [hflip] * 2, [vflip] * 2), size)


def test_shared_ground_truths(dev):
    sizes = [(40, 60), (40, 60), (37, 51), (37, 51), (40, 60)]
    gt_index = [0, 0, 1, 1, 0]
    pairs, lows, highs = _set(dev, sizes, 44, gt_index=gt_index, n_high=2)
    rng = np.random.default_rng(7)
    for b in (1, 5, 16):
        _check(pairs, lows, highs, _rows(rng, sizes, (32, 48), b), (32, 48), gt_index=gt_index)


def test_null_table_by_the_c_abi(dev, mixed):
    """the entry point itself: table == NULL gives the quotient in x and raw; null pointers and oversize batches are refused"""
    from hvi_cidnet_amd import ops
    from hvi_cidnet_amd._lib import lib
    D = _D()
    pairs, lows, highs = mixed
    rows = ([0, 3], [2, 0], [1, 0], [1, 0], [0, 1])
    plan = D.plan_rows(pairs.layout, *rows, (32, 48)).to(dev)
    x, raw, gt = (torch.full((2, 3, 32, 48), -1.0, device=dev) for _ in range(3))
    lib().call("cidnet_augment_crop_flip_raw", ops._p(pairs.arena), ops._p(plan), None, ops._p(x), ops._p(raw), ops._p(gt),
               2, 32, 48, ops._stream())
    wraw, wgt = R.batch(lows, highs, None, *rows, (32, 48))
    assert _same(x, wraw) and _same(raw, wraw) and _same(gt, wgt)
    f = lib().raw("cidnet_augment_crop_flip_raw")
    assert f(ops._p(pairs.arena), ops._p(plan), None, ops._p(x), None, ops._p(gt), 2, 32, 48, ops._stream()) == -1
    assert f(ops._p(pairs.arena), ops._p(plan), None, ops._p(x), ops._p(raw), ops._p(gt), 21846, 32, 48, ops._stream()) == -2
    assert f(ops._p(pairs.arena), ops._p(plan), None, ops._p(x), ops._p(raw), ops._p(gt), 2, 0, 48, ops._stream()) == -1


# ---- guard bands ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(32, 48), (17, 33), (17, 3), (5, 1)])
def test_nothing_outside_the_three_tensors_is_written(dev, mixed, size):
    from hvi_cidnet_amd import ops
    from hvi_cidnet_amd._lib import lib
    D = _D()
    pairs, lows, highs = mixed
    sh, sw = size
    b, guard = 3, 4096
    rows = ([1, 0, 3], [401 - sh, 0, 32 - sh], [603 - sw, 0, 48 - sw], [1, 0, 1], [0, 1, 1])
    n = b * 3 * sh * sw
    pad = -n % 4                                                 # keep every tensor 16-byte aligned inside the buffer
    table = torch.from_numpy(D.gamma_table(0.6)).to(dev)
    plan = D.plan_rows(pairs.layout, *rows, size).to(dev)
    poison = float.fromhex("0x1.8p+100")
    buf = torch.full((4 * guard + 3 * (n + pad),), poison, device=dev)
    starts = [guard + k * (n + pad + guard) for k in range(3)]
    x, raw, gt = (buf[s:s + n].view(b, 3, sh, sw) for s in starts)
    lib().call("cidnet_augment_crop_flip_raw", ops._p(pairs.arena), ops._p(plan), ops._p(table), ops._p(x), ops._p(raw),
               ops._p(gt), b, sh, sw, ops._stream())
    wx, wgt, wraw = _restated(lows, highs, None, rows, size, 0.6)
    assert _same(x, wx) and _same(raw, wraw) and _same(gt, wgt)
    outside = torch.ones_like(buf, dtype=torch.bool)
    for s in starts:
        outside[s:s + n] = False
    assert int(outside.sum()) == 4 * guard + 3 * pad and bool((buf[outside] == poison).all())


# ---- TrainBatches(sampling="scene", raw=True) ------------------------------------------------------------------------------
SCENE_SIZES = [(37, 51), (401, 603), (33, 49), (32, 48), (40, 60), (64, 64), (37, 51), (40, 60)]
SCENE_GROUPS = [("one", [0]), ("three", [1, 2, 3]), ("four", [4, 5, 6, 7])]


def _copies_and_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    # device-side events, so that launches made outside any ATen op (the batch kernel, through ctypes) are listed as well
    from torch.autograd import DeviceType
    copies, kernels = [], []
    for ev in prof.events():
        if ev.device_type == DeviceType.CUDA and "memset" not in ev.name.lower():
            (copies if "memcpy" in ev.name.lower() else kernels).append(ev.name)
    return copies, kernels


def test_scene_batches_with_raw_follow_their_plan(dev):
    D = _D()
    pairs, lows, highs = _set(dev, SCENE_SIZES, 45, groups=SCENE_GROUPS)
    tb = D.TrainBatches(pairs, 5, (32, 48), seed=4, gamma=(60, 120), sampling="scene", raw=True)
    assert len(tb) == 2 and tb.plan(0).index.numel() == 8
    drawn = set()
    for e in (0, 1, 5):
        p = tb.plan(e)
        want = D.scene_epoch_plan(SCENE_GROUPS, SCENE_SIZES, (32, 48), 5, seed=4, epoch=e, gamma=(60, 120))
        assert p.index.tolist() == want.index.tolist() and p.gammas == want.gammas
        assert [hi - lo for lo, hi in p.batches] == [5, 3]
        got = list(tb.epoch(e))
        assert len(got) == 2
        for k, (lo, hi) in enumerate(p.batches):
            rows = [c[lo:hi].tolist() for c in (p.index, p.y0, p.x0, p.hflip, p.vflip)]
            wx, wgt, wraw = _restated(lows, highs, None, rows, (32, 48), p.gammas[k])
            x, gt, raw = got[k]
            assert x.shape == (hi - lo, 3, 32, 48) and _same(x, wx) and _same(gt, wgt) and _same(raw, wraw)
        drawn |= set(p.index.tolist())
    assert drawn <= set(range(8))
    # more draws than images, and another count per epoch than the set's length
    assert len(D.TrainBatches(pairs, 5, (32, 48), sampling="scene", samples=23)) == 5
    # gamma off: the third element IS the first, and the values are the restatement's
    off = D.TrainBatches(pairs, 5, (32, 48), seed=4, sampling="scene", raw=True)
    p = off.plan(2)
    for k, (x, gt, raw) in enumerate(off.epoch(2)):
        assert raw is x
        lo, hi = p.batches[k]
        wraw, wgt = R.batch(lows, highs, None, *[c[lo:hi].tolist() for c in (p.index, p.y0, p.x0, p.hflip, p.vflip)], (32, 48))
        assert _same(x, wraw) and _same(gt, wgt)
    # the defaults are today's: two tensors from the permutation sampler
    plain = D.TrainBatches(pairs, 5, (32, 48), seed=4, gamma=(60, 120))
    assert plain.plan(0).index.tolist() == D.epoch_plan(SCENE_SIZES, (32, 48), 5, seed=4, gamma=(60, 120)).index.tolist()
    assert all(len(batch) == 2 for batch in plain.epoch(0))

    keep = []

    def loop():
        for batch in tb.epoch(3):
            keep.append(batch)
    copies, kernels = _copies_and_kernels(loop)
    assert len(copies) == 1 and "htod" in copies[0].lower(), copies
    assert len(kernels) == 2 and all("cidnet::" in k and "crop_flip_kernel" in k for k in kernels), kernels


def test_train_batches_argument_errors(dev):
    D = _D()
    flat, _, _ = _set(dev, SCENE_SIZES, 45)
    with pytest.raises(ValueError, match="scene"):
        D.TrainBatches(flat, 5, (32, 48), sampling="scene")
    with pytest.raises(ValueError, match="samples"):
        D.TrainBatches(flat, 5, (32, 48), samples=10)
    with pytest.raises(ValueError, match="sampling"):
        D.TrainBatches(flat, 5, (32, 48), sampling="uniform")
    lows = R.random_images(1, SCENE_SIZES)
    for bad in ([("a", [])], [("a", [0]), ("b", [0])], [("a", [8])]):
        with pytest.raises(ValueError, match="groups"):
            D.ResidentPairs(lows, lows, dev, groups=bad)
    small, _, _ = _set(dev, SCENE_SIZES, 45, groups=SCENE_GROUPS)
    small.names = [f"s/{i}.png" for i in range(8)]
    with pytest.raises(ValueError, match=r"'s/2\.png' is 33 x 49"):
        D.TrainBatches(small, 5, (33, 50), sampling="scene")


# ---- from disk -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gt", ["label", "first", "name"])
def test_from_scene_folders_keeps_pil_bytes(dev, tmp_path, gt):
    from PIL import Image
    D = _D()
    low, high = tmp_path / "low", tmp_path / "high"
    scenes = {"s1": (["a.png", "b.png", "c.png"], (37, 51)), "s2": (["a.png"], (40, 60)), "s0": (["k.jpg", "j.png"], (33, 49))}
    seed = 0
    for sub, (files, hw) in scenes.items():
        (low / sub).mkdir(parents=True)
        for f in files:
            seed += 1
            Image.fromarray(R.random_images(seed, [hw])[0], "RGB").save(low / sub / f)
        if gt == "label":
            high.mkdir(exist_ok=True)
            Image.fromarray(R.random_images(seed + 50, [hw])[0], "RGB").save(high / (sub + (".JPG" if sub == "s1" else ".png")),
                                                                             **({"format": "JPEG"} if sub == "s1" else {}))
        else:
            (high / sub).mkdir(parents=True)
            for f in (files if gt == "name" else ["z_long.png", "long.png"]):
                seed += 1
                Image.fromarray(R.random_images(seed + 50, [hw])[0], "RGB").save(high / sub / f)
    (low / "lonely").mkdir()
    Image.fromarray(R.random_images(99, [(20, 20)])[0], "RGB").save(low / "lonely" / "x.png")
    with pytest.warns(UserWarning, match="lonely/x.png"):
        fp = D.scene_pairs(str(low), str(high), gt)
    with pytest.warns(UserWarning, match="lonely/x.png"):
        pairs = D.ResidentPairs.from_scene_folders(str(low), str(high), dev, gt=gt)
    assert pairs.names == fp.names == ["s0/j.png", "s0/k.jpg", "s1/a.png", "s1/b.png", "s1/c.png", "s2/a.png"]
    assert pairs.groups == fp.groups == [("s0", [0, 1]), ("s1", [2, 3, 4]), ("s2", [5])]
    assert pairs.skipped == fp.skipped == ["lonely/x.png"]
    assert len(pairs.layout.high_offsets) == (6 if gt == "name" else 3)      # a shared label is stored once
    if gt != "name":
        assert pairs.layout.gt_index == [0, 0, 1, 1, 1, 2]
    if gt == "first":
        assert all(gp.endswith("long.png") for _, gp in fp.paths)
    for i, (lp, gp) in enumerate(fp.paths):
        with Image.open(lp) as im:
            assert np.array_equal(pairs.low(i).cpu().numpy(), np.array(im.convert("RGB")).transpose(2, 0, 1))
        with Image.open(gp) as im:
            assert np.array_equal(pairs.high(i).cpu().numpy(), np.array(im.convert("RGB")).transpose(2, 0, 1))
    x, g, raw = next(iter(D.TrainBatches(pairs, 4, (32, 48), sampling="scene", raw=True, gamma=(60, 120)).epoch(0)))
    assert x.shape == g.shape == raw.shape == (4, 3, 32, 48)
