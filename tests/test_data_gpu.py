"""GPU: on-device training batches (hvi-cidnet_amd/data.py, csrc/augment.hip) against the restatement of the reference's
transform through PIL (tests/data_ref.py): bit for bit with gamma off, within the reference's own distance from the fp64
yardstick with gamma on; determinism; TrainBatches against crop_flip on epoch_plan's rows; one upload per epoch; a training
step fed by TrainBatches launches nothing but cidnet:: kernels and trains exactly as one fed from the host."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import cidnet_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import data_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _D():
    from hvi_cidnet_amd import data
    return data


def _set(dev, sizes, seed, gt_index=None, n_high=None):
    """(ResidentPairs, lows, highs): seeded uint8 images; with gt_index, high k has the size of a low image that names it"""
    lows = R.random_images(seed, sizes)
    if gt_index is None:
        highs = R.random_images(seed + 1000, sizes)
    else:
        hs = [None] * n_high
        for i, k in enumerate(gt_index):
            hs[k] = sizes[i]
        highs = R.random_images(seed + 1000, hs)
    return _D().ResidentPairs(lows, highs, dev, gt_index=gt_index), lows, highs


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _check(pairs, lows, highs, index, y0, x0, hf, vf, size, gt_index=None):
    x, gt = _D().crop_flip(pairs, index, y0, x0, hf, vf, size)
    rx, rgt = R.batch(lows, highs, gt_index, index, y0, x0, hf, vf, size)
    assert x.dtype == gt.dtype == torch.float32 and x.is_contiguous() and gt.is_contiguous()
    assert _same(x, rx), f"x differs: {size} {index} {y0} {x0} {hf} {vf}"
    assert _same(gt, rgt), f"gt differs: {size} {index} {y0} {x0} {hf} {vf}"
    return x, gt


def _rows(rng, sizes, size, b, n=None):
    sh, sw = (size, size) if isinstance(size, int) else size
    index = rng.integers(0, n or len(sizes), size=b).tolist()
    y0 = [int(rng.integers(0, sizes[i][0] - sh + 1)) for i in index]
    x0 = [int(rng.integers(0, sizes[i][1] - sw + 1)) for i in index]
    return index, y0, x0, rng.integers(0, 2, size=b).tolist(), rng.integers(0, 2, size=b).tolist()


# ---- 6: gamma off, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [256, (400, 600)])
@pytest.mark.parametrize("b", [1, 5, 16])
def test_uniform_set_is_bit_equal(dev, size, b):
    sizes = [(400, 600)] * 6
    pairs, lows, highs = _set(dev, sizes, 11)
    rng = np.random.default_rng(100 + b)
    _check(pairs, lows, highs, *_rows(rng, sizes, size, b), size)
    # all four flip combinations of one window, the same low image several times in one batch
    _check(pairs, lows, highs, [2, 2, 2, 2], [7] * 4 if size == 256 else [0] * 4, [137] * 4 if size == 256 else [0] * 4,
           [0, 1, 0, 1], [0, 0, 1, 1], size)


def test_mixed_sizes_every_alignment_and_flip(dev):
    sizes = [(37, 51), (401, 603), (400, 600), (33, 49), (32, 48)]
    pairs, lows, highs = _set(dev, sizes, 12)
    size = (32, 48)
    rng = np.random.default_rng(5)
    for b in (1, 5, 16):
        _check(pairs, lows, highs, *_rows(rng, sizes, size, b), size)
    # every x0 mod 16 under every flip combination, on the image whose rows are 603 bytes
    x0 = [130 + k for k in range(16)] * 4
    hf = [0] * 16 + [1] * 16 + [0] * 16 + [1] * 16
    vf = [0] * 32 + [1] * 32
    _check(pairs, lows, highs, [1] * 64, [(7 * k) % 370 for k in range(64)], x0, hf, vf, size)
    # the image one pixel larger than the crop: its four origins, all flips; the image that is the crop
    for hflip in (0, 1):
        for vflip in (0, 1):
            _check(pairs, lows, highs, [3, 3, 3, 3, 4], [0, 0, 1, 1, 0], [0, 1, 0, 1, 0], [hflip] * 5, [vflip] * 5, size)


@pytest.mark.parametrize("sw", [1, 3, 33, 255])
def test_widths_that_are_not_multiples_of_four(dev, sw):
    sizes = [(400, 600), (37, 51) if sw <= 33 else (300, 255)]
    pairs, lows, highs = _set(dev, sizes, 13)
    size = (17, sw)
    rng = np.random.default_rng(sw)
    for _ in range(3):
        _check(pairs, lows, highs, *_rows(rng, sizes, size, 5), size)
    for k in range(16):                                          # every source alignment, every flip
        _check(pairs, lows, highs, [0] * 4, [3] * 4, [200 + k] * 4, [0, 1, 0, 1], [0, 0, 1, 1], size)


@pytest.mark.parametrize("size", [256, (31, 255), (400, 600), (1, 1)])
def test_windows_at_the_ends_of_the_arena(dev, size):
    """the first image cropped at its top-left corner (mirrored: the window's last pixel is the arena's first byte) and the
    last image of the arena, a ground truth, cropped at its bottom-right corner, where 3 h w is a multiple of 16 so the
    window ends with the arena"""
    sizes = [(400, 600)] * 3
    pairs, lows, highs = _set(dev, sizes, 14)
    assert pairs.layout.gt_offset(2) + 3 * 400 * 600 == pairs.layout.total_bytes == pairs.arena.numel()
    sh, sw = (size, size) if isinstance(size, int) else size
    for hflip in (0, 1):
        for vflip in (0, 1):
            _check(pairs, lows, highs, [0, 2], [0, 400 - sh], [0, 600 - sw], [hflip] * 2, [vflip] * 2, size)


def test_shared_ground_truths(dev):
    sizes = [(40, 60), (40, 60), (37, 51), (37, 51), (40, 60)]
    gt_index = [0, 0, 1, 1, 0]
    pairs, lows, highs = _set(dev, sizes, 15, gt_index=gt_index, n_high=2)
    assert len(pairs) == 5 and len(pairs.layout.high_offsets) == 2
    rng = np.random.default_rng(6)
    for b in (1, 5, 16):
        _check(pairs, lows, highs, *_rows(rng, sizes, (32, 48), b), (32, 48), gt_index=gt_index)
    for i in range(5):
        assert np.array_equal(pairs.low(i).cpu().numpy(), lows[i].transpose(2, 0, 1))
        assert np.array_equal(pairs.high(i).cpu().numpy(), highs[gt_index[i]].transpose(2, 0, 1))


def _levels_image():
    return np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2)


def test_all_levels_divide_exactly(dev):
    """gt of a 16 x 16 image holding all 256 levels is torch.arange(256) / 255 (CPU, a true division) bit for bit, and so is
    x with gamma off"""
    im = _levels_image()
    pairs = _D().ResidentPairs([im], [im], dev)
    x, gt = _D().crop_flip(pairs, [0], [0], [0], [0], [0], 16)
    want = (torch.arange(256, dtype=torch.float32) / 255).view(1, 1, 16, 16).expand(1, 3, 16, 16)
    assert _same(gt, want) and _same(x, want)


# ---- 7: gamma on, exhaustively ------------------------------------------------------------------------------------------
def test_gamma_all_levels_all_gammas(dev):
    """All 256 levels x the 61 gammas of --start_gamma 60 --end_gamma 120 against fp32(pow(fp64(fp32(q) / 255), gamma)).  The
    reference's own fp32 `x ** gamma` is up to 4 ulps from that yardstick on this domain, and the kernel may not be further:
    <= 4 ulps, 0 -> 0 and 255 -> 1.0 exact, gamma 1.0 bit-equal to gamma off.  Measured on an MI355X: 0 ulps (the table is
    built on the host in fp64)."""
    D = _D()
    im = _levels_image()
    pairs = D.ResidentPairs([im], [im], dev)
    off = D.crop_flip(pairs, [0], [0], [0], [0], [0], 16)
    worst, differing = 0, 0
    for k in range(60, 121):
        g = k / 100
        x, gt = D.crop_flip(pairs, [0], [0], [0], [0], [0], 16, gamma=g)
        assert _same(gt, off[1])
        got = x.cpu().numpy()
        assert np.array_equal(got[0, 0], got[0, 1]) and np.array_equal(got[0, 0], got[0, 2])
        u = R.ulps(got[0, 0].reshape(-1), R.gamma_yardstick(g))
        worst, differing = max(worst, int(u.max())), differing + int((u != 0).sum())
        assert got[0, 0, 0, 0] == 0.0 and got[0, 0, 15, 15] == 1.0
        if k == 100:
            assert _same(x, off[0])
    print(f"gamma on: max {worst} ulps from the yardstick, {differing} of {61 * 256} values differ")
    assert worst <= 4
    # gamma 1.0 through the table (TrainBatches always uploads one when gamma is on) is the quotient as well
    a = next(iter(D.TrainBatches(pairs, 1, 16, gamma=(100, 100), shuffle=False).epoch(0)))
    assert a[0].shape == (1, 3, 16, 16) and _same(a[0], a[1])
    # a flipped window reads the table the same way
    x, _ = D.crop_flip(pairs, [0], [0], [0], [1], [1], 16, gamma=0.6)
    want = torch.from_numpy(R.gamma_yardstick(0.6)).view(16, 16).flip(0, 1)
    assert int(R.ulps(x[0, 1].cpu().numpy(), want.numpy()).max()) <= 4


def test_bad_rows_are_refused_before_a_launch(dev):
    D = _D()
    pairs, _, _ = _set(dev, [(40, 60), (37, 51)], 16)
    ok = dict(index=[1], y0=[5], x0=[3], hflip=[0], vflip=[0])
    for bad in (dict(index=[2]), dict(index=[-1]), dict(y0=[6]), dict(x0=[4]), dict(y0=[-1]), dict(x0=[-1])):
        with pytest.raises(ValueError):
            D.crop_flip(pairs, size=(32, 48), **{**ok, **bad})
    for g in (0.0, -0.5):
        with pytest.raises(ValueError, match="gamma"):
            D.crop_flip(pairs, size=(32, 48), gamma=g, **ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.ResidentPairs(R.random_images(0, [(16, 16)]), R.random_images(1, [(16, 16)]), "cpu")
    with pytest.raises(ValueError, match="max_bytes"):
        D.ResidentPairs(R.random_images(0, [(16, 16)]), R.random_images(1, [(16, 16)]), dev, max_bytes=1000)
    with pytest.raises(ValueError, match="ground truth"):
        D.ResidentPairs(R.random_images(0, [(16, 16)]), R.random_images(1, [(16, 17)]), dev)


# ---- 8: determinism -----------------------------------------------------------------------------------------------------
def test_values_depend_on_the_row_alone(dev):
    D = _D()
    sizes = [(400, 600), (401, 603), (300, 500)]
    pairs, _, _ = _set(dev, sizes, 17)
    rng = np.random.default_rng(8)
    rows = _rows(rng, sizes, 256, 16)
    for gamma in (1.0, 0.73):
        a = D.crop_flip(pairs, *rows, 256, gamma=gamma)
        b = D.crop_flip(pairs, *rows, 256, gamma=gamma)
        assert _same(a[0], b[0]) and _same(a[1], b[1])
        for k in (0, 7, 15):                                     # sample k alone, and at another position of a batch of 5
            one = D.crop_flip(pairs, *[[c[k]] for c in rows], 256, gamma=gamma)
            assert _same(one[0][0], a[0][k]) and _same(one[1][0], a[1][k])
            five = [[c[(k + 3 + m) % 16] for m in range(5)] for c in rows]
            for col in range(5):
                five[col][3] = rows[col][k]
            got = D.crop_flip(pairs, *five, 256, gamma=gamma)
            assert _same(got[0][3], a[0][k]) and _same(got[1][3], a[1][k])


# ---- 9: TrainBatches ------------------------------------------------------------------------------------------------------
def _copies(fn):
    """names of the memory-copy activities the profiler attributes to fn()"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = []
    for ev in prof.events():
        names += [k.name for k in (getattr(ev, "kernels", []) or []) if "memcpy" in k.name.lower()]
    return names


@pytest.mark.parametrize("gamma", [None, (60, 120)])
def test_train_batches_follow_the_epoch_plan(dev, gamma):
    """epoch(e) yields what crop_flip gives for epoch_plan's rows, batch by batch, the short last one included (a crop that is
    not a multiple of 8 is legal here; the model refuses it, as it always has); two objects with the same seed agree.  The
    loop makes one host-to-device copy per epoch and no device-to-host copy, counted from the memory-copy activities of a
    torch.profiler run (a control run checks that the profiler lists both directions on this stack)."""
    D = _D()
    sizes = [(37, 51), (401, 603), (400, 600), (33, 49)] * 2 + [(64, 64)] * 3
    pairs, lows, highs = _set(dev, sizes, 18)
    size = (30, 44)
    tb = D.TrainBatches(pairs, 4, size, seed=7, gamma=gamma)
    assert len(tb) == 3
    for e in (0, 3):
        p = D.epoch_plan(sizes, size, 4, seed=7, epoch=e, gamma=gamma)
        assert [hi - lo for lo, hi in p.batches] == [4, 4, 3]
        got = list(tb.epoch(e))
        again = list(D.TrainBatches(pairs, 4, size, seed=7, gamma=gamma).epoch(e))
        assert len(got) == len(again) == 3
        for k, (lo, hi) in enumerate(p.batches):
            cols = [c[lo:hi] for c in (p.index, p.y0, p.x0, p.hflip, p.vflip)]
            want = D.crop_flip(pairs, *cols, size, gamma=p.gammas[k] if gamma else 1.0)
            for t in range(2):
                assert got[k][t].shape == (hi - lo, 3, 30, 44)
                assert _same(got[k][t], want[t]) and _same(again[k][t], want[t])
            if gamma is None:
                rx, rgt = R.batch(lows, highs, None, *[c.tolist() for c in cols], size)
                assert _same(got[k][0], rx) and _same(got[k][1], rgt)
    assert D.TrainBatches(pairs, 4, size, seed=8, gamma=gamma).plan(0).index.tolist() != tb.plan(0).index.tolist()
    assert len(D.TrainBatches(pairs, 4, size, seed=7, gamma=gamma, drop_last=True)) == 2

    keep = []

    def control():
        keep.append(torch.arange(64).to(dev).cpu())
    listed = [n.lower() for n in _copies(control)]
    assert any("htod" in n for n in listed) and any("dtoh" in n for n in listed), \
        f"the profiler does not list memory copies here: {listed}"

    def loop():
        for x, gt in tb.epoch(1):
            keep.append((x, gt))
    names = [n.lower() for n in _copies(loop)]
    assert len(names) == 1 and "htod" in names[0], names


def test_model_refuses_a_crop_that_is_not_a_multiple_of_8(dev):
    import hvi_cidnet_amd as P
    pairs, _, _ = _set(dev, [(64, 64)] * 2, 19)
    x, _ = next(iter(P.TrainBatches(pairs, 2, (30, 44)).epoch(0)))
    with pytest.raises(RuntimeError, match="multiples of 8"):
        P.CIDNet(channels=[12, 12, 24, 48]).to(dev)(x)


# ---- 10 / 11: in front of the trainer ---------------------------------------------------------------------------------------
def _foreign_kernels():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    try:
        from foreign_kernels_in_step import foreign_kernels
    finally:
        sys.path.pop(0)
    return foreign_kernels


def _model(dev, chans):
    import hvi_cidnet_amd as P
    m = P.CIDNet(channels=list(chans))
    p = O.make_params(21, channels=chans)
    m.load_state_dict({k: p[k] for k in m.state_dict().keys()})
    return m.to(dev)


class _FedTrainer:
    """what a training loop does per step: draw the batch, run the step"""

    def __init__(self, trainer, batches):
        self.trainer, self.batches = trainer, batches

    def step(self, x=None, gt=None):
        x, gt = next(self.batches)
        return self.trainer.step(x, gt)


@pytest.mark.parametrize("two_streams", [True, False])
def test_batch_and_training_step_launch_only_cidnet_kernels(dev, two_streams):
    """The point of the resident set: `x, gt = next(batches); trainer.step(x, gt)` on the full-width model, gamma on, launches
    nothing but cidnet:: kernels -- the batch for step n + 1 runs beside the split-product convolutions of step n, where
    ATen's packed-fp32 elementwise kernels may not."""
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd.dp import DataParallelTrainer
    foreign_kernels = _foreign_kernels()
    pairs, _, _ = _set(dev, [(80, 120), (70, 100)] * 6, 20)
    tb = P.TrainBatches(pairs, 2, (64, 96), seed=1, gamma=(60, 120))
    assert len(tb) == 6
    m = _model(dev, (36, 36, 72, 144))
    m.two_streams = two_streams
    fed = _FedTrainer(DataParallelTrainer(m, lr=1e-3, wgrad_stream=two_streams), tb.epoch(0))
    for _ in range(3):
        fed.step()
    fk = foreign_kernels(fed, None, None, steps=2)
    assert not fk, {k: [(op, shp) for op, shp, _ in v][:3] for k, v in fk.items()}


def test_trainer_fed_from_the_device_equals_trainer_fed_from_the_host(dev):
    """three steps fed by TrainBatches (gamma off) leave flat_p bit-identical to three steps fed by the same batches built by
    the restatement on the host and copied over"""
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd.dp import DataParallelTrainer
    chans, size = (12, 12, 24, 48), (32, 48)
    sizes = [(37, 51), (40, 60), (64, 64)] * 2
    pairs, lows, highs = _set(dev, sizes, 21)
    tb = P.TrainBatches(pairs, 2, size, seed=3)
    p = tb.plan(0)
    finals = []
    for source in ("device", "host"):
        tr = DataParallelTrainer(_model(dev, chans), lr=1e-3)
        it = tb.epoch(0)
        for lo, hi in p.batches[:3]:
            if source == "device":
                x, gt = next(it)
            else:
                x, gt = R.batch(lows, highs, None, *[c[lo:hi].tolist() for c in (p.index, p.y0, p.x0, p.hflip, p.vflip)], size)
                x, gt = x.to(dev), gt.to(dev)
            tr.step(x, gt)
        torch.cuda.synchronize()
        finals.append(tr.flat_p.clone())
    assert len(p.batches) == 3 and torch.equal(_bits(finals[0]), _bits(finals[1]))


# ---- 12: from disk --------------------------------------------------------------------------------------------------------
def test_from_folders_keeps_pil_bytes(dev, tmp_path):
    from PIL import Image
    import hvi_cidnet_amd as P
    low, high = tmp_path / "low", tmp_path / "high"
    low.mkdir()
    high.mkdir()
    sizes = {"b.png": (37, 51), "a.png": (40, 60), "c.png": (33, 49), "orphan.png": (20, 20)}
    for k, (name, hw) in enumerate(sizes.items()):
        lo_im, hi_im = R.random_images(30 + k, [hw, hw])
        Image.fromarray(lo_im, "RGB").save(low / name)
        if name != "orphan.png":
            Image.fromarray(hi_im, "RGB").save(high / name)
    Image.fromarray(np.full((9, 9), 7, dtype=np.uint8), "L").save(low / "gray.png")       # .convert('RGB') applies
    Image.fromarray(R.random_images(40, [(9, 9)])[0], "RGB").save(high / "gray.png")
    with pytest.warns(UserWarning, match="orphan.png"):
        fp = P.folder_pairs(str(low), str(high))
    with pytest.warns(UserWarning, match="orphan.png"):
        pairs = P.ResidentPairs.from_folders(str(low), str(high), dev)
    assert pairs.names == fp.names == ["a.png", "b.png", "c.png", "gray.png"] and pairs.skipped == fp.skipped == ["orphan.png"]
    assert len(pairs) == 4
    for i, (lp, gp) in enumerate(fp.paths):
        with Image.open(lp) as im:
            want = np.array(im.convert("RGB")).transpose(2, 0, 1)
        assert np.array_equal(pairs.low(i).cpu().numpy(), want)
        with Image.open(gp) as im:
            want = np.array(im.convert("RGB")).transpose(2, 0, 1)
        assert np.array_equal(pairs.high(i).cpu().numpy(), want)
    x, gt = next(iter(P.TrainBatches(pairs, 4, 9, shuffle=False).epoch(0)))
    assert x.shape == gt.shape == (4, 3, 9, 9)
    assert float(x[3].min()) == float(x[3].max()) == float(np.float32(7) / np.float32(255))
