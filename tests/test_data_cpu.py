"""CPU: the host side of the on-device training batches (hvi-cidnet_amd/data.py) -- the arena layout, epoch_plan (a pure
function of its arguments: permutation, rank shares, crop origins, flips, gammas), the gamma table and the errors raised
before anything reaches a device."""
import collections
import math
import os
import sys

import numpy as np
import pytest
import torch

from hvi_cidnet_amd import data as D

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import data_ref as R  # noqa: E402


def _cols(p):
    return [t.tolist() for t in (p.index, p.y0, p.x0, p.hflip, p.vflip)] + [p.batches, p.gammas]


def test_arena_layout_places_every_image_once():
    low = [(400, 600), (37, 51), (401, 603), (8, 8), (37, 51)]
    lay = D.arena_layout(low, low)
    spans = sorted((o, o + 3 * h * w) for o, (h, w) in zip(lay.low_offsets + lay.high_offsets, low + low))
    assert spans[0][0] == 0 and all(o % D.ARENA_ALIGN == 0 for o, _ in spans)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))           # no overlap
    assert spans[-1][1] <= lay.total_bytes < spans[-1][1] + D.ARENA_ALIGN
    assert lay.sizes == low and lay.gt_index == list(range(5))
    # fill an arena on the host as ResidentPairs fills it on the device and read every image back from the table
    imgs = R.random_images(3, low + low)
    arena = np.zeros(lay.total_bytes, dtype=np.uint8)
    for im, off in zip(imgs, lay.low_offsets + lay.high_offsets):
        arena[off:off + im.size] = im.transpose(2, 0, 1).reshape(-1)
    for i, (h, w) in enumerate(low):
        assert np.array_equal(arena[lay.low_offsets[i]:][:3 * h * w].reshape(3, h, w), imgs[i].transpose(2, 0, 1))
        assert np.array_equal(arena[lay.gt_offset(i):][:3 * h * w].reshape(3, h, w), imgs[5 + i].transpose(2, 0, 1))


def test_arena_layout_stores_shared_ground_truths_once():
    low = [(40, 60)] * 5 + [(37, 51)] * 2
    high = [(40, 60), (37, 51), (40, 60)]
    gt_index = [0, 0, 2, 0, 2, 1, 1]
    lay = D.arena_layout(low, high, gt_index)
    assert len(lay.high_offsets) == 3 and len(set(lay.high_offsets)) == 3
    assert [lay.gt_offset(i) for i in range(7)] == [lay.high_offsets[k] for k in gt_index]
    assert lay.total_bytes == sum(-(-3 * h * w // 16) * 16 for h, w in low + high)


def test_epoch_plan_is_a_function_of_its_arguments():
    sizes = [(400, 600)] * 20 + [(300, 500)] * 11
    kw = dict(crop=256, batch_size=4, gamma=(60, 120))
    for rank, world in ((0, 1), (1, 3)):
        a = D.epoch_plan(sizes, seed=5, epoch=2, rank=rank, world=world, **kw)
        b = D.epoch_plan(sizes, seed=5, epoch=2, rank=rank, world=world, **kw)
        assert _cols(a) == _cols(b)
    base = D.epoch_plan(sizes, seed=5, epoch=2, **kw)
    assert D.epoch_plan(sizes, seed=5, epoch=3, **kw).index.tolist() != base.index.tolist()
    assert D.epoch_plan(sizes, seed=6, epoch=2, **kw).index.tolist() != base.index.tolist()
    assert sorted(base.index.tolist()) == list(range(31))
    # without shuffling the order is the set's, the other draws stay random
    plain = D.epoch_plan(sizes, seed=5, epoch=2, shuffle=False, **kw)
    assert plain.index.tolist() == list(range(31))
    # the ranks of a world cut one permutation: rank r holds positions r, r + world, ...
    whole = D.epoch_plan(sizes, seed=5, epoch=2, **kw)
    parts = [D.epoch_plan(sizes, seed=5, epoch=2, rank=r, world=3, **kw) for r in range(3)]
    inter = [parts[k % 3].index[k // 3].item() for k in range(33)]
    assert inter[:31] == whole.index.tolist() and inter[31:] == whole.index.tolist()[:2]


@pytest.mark.parametrize("world", [1, 2, 3, 5])
@pytest.mark.parametrize("n", [1, 7, 485])
def test_epoch_plan_covers_the_set_over_the_ranks(n, world):
    sizes = [(64, 96)] * n
    bs = 4
    per_rank = -(-n // world)
    plans = [D.epoch_plan(sizes, 32, bs, seed=1, epoch=0, rank=r, world=world) for r in range(world)]
    drawn = collections.Counter(i for p in plans for i in p.index.tolist())
    assert set(drawn) == set(range(n))
    extra = world * per_rank - n
    assert sum(drawn.values()) == n + extra
    if extra <= n:
        assert sorted(drawn.values()) == [1] * (n - extra) + [2] * extra     # wrapped repeats: each at most once more
    shapes = [[hi - lo for lo, hi in p.batches] for p in plans]
    assert all(s == shapes[0] for s in shapes)
    assert shapes[0] == [bs] * (per_rank // bs) + ([per_rank % bs] if per_rank % bs else [])
    assert all(p.index.numel() == per_rank for p in plans)
    dropped = [D.epoch_plan(sizes, 32, bs, seed=1, epoch=0, rank=r, world=world, drop_last=True) for r in range(world)]
    for p, q in zip(plans, dropped):
        assert [hi - lo for lo, hi in q.batches] == [bs] * (per_rank // bs)
        k = (per_rank // bs) * bs
        assert _cols(q)[:5] == [c[:k] for c in _cols(p)[:5]]               # only the short batch is gone


def test_epoch_plan_ranges_on_mixed_sizes():
    sizes = [(400, 600), (37, 51), (401, 603), (33, 49), (32, 48)]
    sh, sw = 32, 48
    seen_small = set()
    for epoch in range(40):
        p = D.epoch_plan(sizes, (sh, sw), 2, seed=9, epoch=epoch)
        for i, y, x in zip(p.index.tolist(), p.y0.tolist(), p.x0.tolist()):
            h, w = sizes[i]
            assert 0 <= y <= h - sh and 0 <= x <= w - sw
            if i == 4:
                assert (y, x) == (0, 0)                                     # crop == image
            if i == 3:
                seen_small.add((y, x))
    assert seen_small == {(0, 0), (0, 1), (1, 0), (1, 1)}                  # the 1-pixel-larger image uses both origins per axis
    p = D.epoch_plan([(64, 64)] * 9, 64, 4, seed=0, epoch=0)
    assert set(p.y0.tolist()) == {0} and set(p.x0.tolist()) == {0}


def test_epoch_plan_reaches_every_origin_and_flip_combination():
    """37 x 51 image, 32 x 48 crop: 6 x 4 origins and the four flip combinations all occur within 40 seeded epochs of 64
    samples (2 560 draws over 24 and over 4 equally likely outcomes: a miss has probability < 24 (23/24)^2560 < 1e-45)"""
    origins, flips = set(), set()
    for epoch in range(40):
        p = D.epoch_plan([(37, 51)] * 64, (32, 48), 8, seed=3, epoch=epoch)
        origins |= set(zip(p.y0.tolist(), p.x0.tolist()))
        flips |= set(zip(p.hflip.tolist(), p.vflip.tolist()))
    assert origins == {(y, x) for y in range(6) for x in range(4)}
    assert flips == {(a, b) for a in (False, True) for b in (False, True)}


def test_epoch_plan_gammas_include_both_ends():
    """--start_gamma 60 --end_gamma 120 through random.randint: 61 values, both ends included (40 epochs x 61 batches = 2 440
    draws; an end is missed with probability (60/61)^2440 < 1e-17)"""
    seen = set()
    for epoch in range(40):
        p = D.epoch_plan([(32, 32)] * 61, 32, 1, seed=2, epoch=epoch, gamma=(60, 120))
        assert len(p.gammas) == len(p.batches) == 61
        seen |= set(p.gammas)
    allowed = {k / 100 for k in range(60, 121)}
    assert seen <= allowed and 0.6 in seen and 1.2 in seen
    assert D.epoch_plan([(32, 32)] * 4, 32, 2, gamma=None).gammas is None
    # ranks draw their own gammas
    a = D.epoch_plan([(32, 32)] * 64, 32, 1, seed=2, rank=0, world=2, gamma=(60, 120)).gammas
    b = D.epoch_plan([(32, 32)] * 64, 32, 1, seed=2, rank=1, world=2, gamma=(60, 120)).gammas
    assert a != b


def test_gamma_table_against_the_fp64_yardstick():
    """the table that rides in the plan: fp32(pow(fp64(fp32(q) / 255), gamma)) for all 256 levels x 61 gammas; exact ends;
    gamma 1 is the quotient itself.  The bound is the issue's: the reference's own fp32 `x ** gamma` is up to 4 ulps from the
    yardstick on this domain, and the table may not be further away than that."""
    quot = (torch.arange(256, dtype=torch.float32) / 255).numpy()
    assert np.array_equal(D.gamma_table(1.0).view(np.int32), quot.view(np.int32))
    worst = 0
    for k in range(60, 121):
        t = D.gamma_table(k / 100)
        assert t.dtype == np.float32 and t.shape == (256,)
        assert t[0] == 0.0 and t[255] == 1.0
        worst = max(worst, int(R.ulps(t, R.gamma_yardstick(k / 100)).max()))
    print("gamma_table: max ulps from the yardstick", worst)
    assert worst <= 4
    with pytest.raises(ValueError, match="gamma"):
        D.gamma_table(0.0)
    with pytest.raises(ValueError, match="gamma"):
        D.gamma_table(-1.0)


def test_true_division_differs_from_the_reciprocal_product():
    """why neither the kernel nor the table may use q * fl(1 / 255): it is wrong on 126 of the 256 levels"""
    q = np.arange(256, dtype=np.float32)
    assert int((q / np.float32(255) != q * (np.float32(1) / np.float32(255))).sum()) == 126
    assert np.array_equal(q / np.float32(255), (torch.arange(256, dtype=torch.float32) / 255).numpy())


def test_plan_errors_are_raised_on_the_host():
    with pytest.raises(ValueError, match=r"'small\.png' is 37 x 51, smaller than the 64 x 64 crop"):
        D.epoch_plan([(400, 600), (37, 51)], 64, 2, names=["big.png", "small.png"])
    with pytest.raises(ValueError, match=r"#1 is 37 x 51"):
        D.epoch_plan([(400, 600), (37, 51)], (32, 64), 2)
    with pytest.raises(ValueError, match=r"low image is 40 x 60, its ground truth \(#1\) is 40 x 61"):
        D.arena_layout([(40, 60), (40, 60)], [(40, 60), (40, 61)])
    with pytest.raises(ValueError, match=r"needs 14400 bytes .* max_bytes = 14399"):
        D.arena_layout([(40, 60)], [(40, 60)], max_bytes=14399)
    assert D.arena_layout([(40, 60)], [(40, 60)], max_bytes=14400).total_bytes == 14400
    with pytest.raises(ValueError, match="gt_index"):
        D.arena_layout([(40, 60)], [(40, 60)], gt_index=[1])
    lay = D.arena_layout([(40, 60), (37, 51)], [(40, 60), (37, 51)])
    ok = D.plan_rows(lay, [1, 0], [5, 8], [3, 12], [1, 0], [0, 1], (32, 48))
    assert ok.dtype == torch.int64 and ok.shape == (2, D.PLAN_WORDS)
    assert ok.tolist() == [[lay.low_offsets[1], lay.high_offsets[1], 37, 51, 5, 3, 1, 0],
                           [lay.low_offsets[0], lay.high_offsets[0], 40, 60, 8, 12, 2, 0]]
    for bad in (dict(index=[2]), dict(index=[-1]), dict(y0=[6]), dict(x0=[4]), dict(y0=[-1]), dict(x0=[-1])):
        args = dict(index=[1], y0=[5], x0=[3], hflip=[0], vflip=[0])
        args.update(bad)
        with pytest.raises(ValueError):
            D.plan_rows(lay, crop=(32, 48), **args)


def test_data_path_refuses_the_cpu():
    imgs = R.random_images(0, [(16, 16)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.ResidentPairs(imgs, imgs, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.ResidentPairs.from_folders("unused", "unused", torch.device("cpu"))


def test_restatement_is_crop_then_flips_then_division():
    """the restatement itself, against plain indexing on a small image"""
    im = R.random_images(4, [(9, 11)])[0]
    t = R.transform(im, 2, 3, True, True, (4, 5))
    want = torch.from_numpy(im[2:6, 3:8][::-1, ::-1].copy()).permute(2, 0, 1).float() / 255
    assert torch.equal(t, want)
    assert math.isclose(R.gamma_yardstick(0.6)[51], 0.2 ** 0.6, rel_tol=1e-6)
