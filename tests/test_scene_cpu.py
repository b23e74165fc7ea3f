"""No GPU: the scene-folder training sets (hvi-cidnet_amd/data.py) -- scene_epoch_plan's two-stage distribution, determinism,
rank shares, drop_last and errors, and scene_pairs' pairing of name / first / label layouts on trees of tiny image files."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import data_ref as R  # noqa: E402


def _D():
    from hvi_cidnet_amd import data
    return data


GROUPS = [("a", [0]), ("b", [1, 2, 3]), ("c", list(range(4, 16)))]
SIZES = [(40, 60)] * 16


# ---- distribution --------------------------------------------------------------------------------------------------------
def test_scene_then_member_distribution():
    """Scenes of 1, 3 and 12 images, 48000 draws: image i of a scene of k images is drawn with p = 1 / (3 k), expected counts
    16000, 5333.3 and 1333.3; every count within 5 binomial standard deviations (sqrt(n p (1 - p)) = 103.3, 68.9, 36.0).
    A sampler uniform over the 16 images gives 3000 +- 53 each: 13000, 2333 and 1667 away, so it fails every cell (the
    nearest, 1333.3 + 5 * 36.0 = 1513, is still 28 of ITS standard deviations below 3000)."""
    n = 48000
    p = _D().scene_epoch_plan(GROUPS, SIZES, (32, 48), 8, samples=n, seed=5, epoch=2)
    assert p.index.numel() == n and sum(hi - lo for lo, hi in p.batches) == n
    counts = np.bincount(p.index.numpy(), minlength=16)
    for _, members in GROUPS:
        prob = 1.0 / (3 * len(members))
        want, sd = n * prob, math.sqrt(n * prob * (1 - prob))
        for i in members:
            print(f"image {i}: {counts[i]} drawn, expected {want:.1f} +- {sd:.1f}")
            assert abs(counts[i] - want) <= 5 * sd, (i, counts[i], want, sd)
            assert abs(3000 - want) > 5 * sd + 5 * math.sqrt(n / 16 * 15 / 16)      # the uniform sampler cannot pass this cell
    # the crop origins are legal and reach both ends of their ranges, the flips are fair
    assert int(p.y0.min()) == 0 and int(p.y0.max()) == 8 and int(p.x0.min()) == 0 and int(p.x0.max()) == 12
    for f in (p.hflip, p.vflip):
        assert abs(int(f.sum()) - n / 2) <= 5 * math.sqrt(n / 4)


def test_default_samples_is_the_number_of_images_in_the_scenes():
    D = _D()
    p = D.scene_epoch_plan(GROUPS[:2], SIZES, 32, 3)            # 4 images in the scenes, 12 in none: never drawn
    assert p.index.numel() == 4 and [hi - lo for lo, hi in p.batches] == [3, 1]
    many = D.scene_epoch_plan(GROUPS[:2], SIZES, 32, 3, samples=500)
    assert set(many.index.tolist()) == {0, 1, 2, 3}


# ---- determinism ---------------------------------------------------------------------------------------------------------
def _cols(p):
    return [c.tolist() for c in (p.index, p.y0, p.x0, p.hflip, p.vflip)]


def test_plan_is_a_pure_function_of_seed_and_epoch():
    D = _D()
    kw = dict(samples=200, gamma=(60, 120))
    a = D.scene_epoch_plan(GROUPS, SIZES, (32, 48), 8, seed=3, epoch=4, **kw)
    b = D.scene_epoch_plan(GROUPS, SIZES, (32, 48), 8, seed=3, epoch=4, **kw)
    assert _cols(a) == _cols(b) and a.batches == b.batches and a.gammas == b.gammas
    assert all(0.6 <= g <= 1.2 for g in a.gammas) and len(a.gammas) == len(a.batches) == 25
    assert D.scene_epoch_plan(GROUPS, SIZES, (32, 48), 8, seed=3, epoch=5, **kw).index.tolist() != a.index.tolist()
    assert D.scene_epoch_plan(GROUPS, SIZES, (32, 48), 8, seed=4, epoch=4, **kw).index.tolist() != a.index.tolist()


# ---- rank shares ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
def test_rank_shares_interleave_to_the_single_rank_plan(world):
    D = _D()
    samples = 100                                                # divisible by neither 2 * 8 nor 3
    samples += 1 if samples % world == 0 else 0
    assert samples % world != 0
    total = world * -(-samples // world)
    kw = dict(seed=9, epoch=1, gamma=(60, 120))
    ranks = [D.scene_epoch_plan(GROUPS, SIZES, (32, 48), 8, samples=samples, rank=r, world=world, **kw) for r in range(world)]
    one = D.scene_epoch_plan(GROUPS, SIZES, (32, 48), 8, samples=total, **kw)
    assert len({len(p) for p in ranks}) == 1 and len({tuple(p.batches) for p in ranks}) == 1
    assert all(p.index.numel() == total // world for p in ranks)
    for col in range(5):
        inter = [None] * total
        for r, p in enumerate(ranks):
            inter[r::world] = _cols(p)[col]
        assert inter == _cols(one)[col], col
    assert len({tuple(p.gammas) for p in ranks}) > 1             # drawn per batch AND rank, as epoch_plan does
    # the same rule as epoch_plan's: rank r of `world` reads column r of one (steps, world) draw
    assert all(len(p.gammas) == len(p.batches) for p in ranks)


# ---- drop_last -----------------------------------------------------------------------------------------------------------
def test_drop_last_drops_the_short_batch_and_nothing_else():
    D = _D()
    kw = dict(samples=21, seed=2, epoch=0, gamma=(60, 120))
    full = D.scene_epoch_plan(GROUPS, SIZES, 32, 8, **kw)
    cut = D.scene_epoch_plan(GROUPS, SIZES, 32, 8, drop_last=True, **kw)
    assert [hi - lo for lo, hi in full.batches] == [8, 8, 5] and cut.batches == full.batches[:2]
    assert cut.index.numel() == 16 and [c[:16] for c in _cols(full)] == _cols(cut) and cut.gammas == full.gammas[:2]
    even = D.scene_epoch_plan(GROUPS, SIZES, 32, 7, drop_last=True, **kw)
    assert [hi - lo for lo, hi in even.batches] == [7, 7, 7]
    none = D.scene_epoch_plan(GROUPS, SIZES, 32, 8, samples=5, drop_last=True)
    assert len(none) == 0 and none.index.numel() == 0


# ---- errors --------------------------------------------------------------------------------------------------------------
def test_errors():
    D = _D()
    names = [f"{sub}/{k}.png" for sub, m in GROUPS for k in range(len(m))]
    sizes = list(SIZES)
    sizes[2] = (31, 60)
    with pytest.raises(ValueError, match=r"'b/1\.png' is 31 x 60, smaller than the 32 x 48 crop"):
        D.scene_epoch_plan(GROUPS, sizes, (32, 48), 8, names=names)
    D.scene_epoch_plan([GROUPS[0], GROUPS[2]], sizes, (32, 48), 8, names=names)       # the small image is in no scene
    for bad in ([("a", [0]), ("b", [])], [("a", [0, 1]), ("b", [1, 2])], [("a", [0, 0])], [("a", [16])], [("a", [-1])], []):
        with pytest.raises(ValueError, match="groups"):
            D.scene_epoch_plan(bad, SIZES, 32, 8)
        with pytest.raises(ValueError, match="groups"):
            D.check_groups(bad, 16)
    for samples in (0, -3):
        with pytest.raises(ValueError, match="samples"):
            D.scene_epoch_plan(GROUPS, SIZES, 32, 8, samples=samples)
    for kw in (dict(batch_size=0), dict(batch_size=8, world=0), dict(batch_size=8, rank=2, world=2)):
        with pytest.raises(ValueError):
            D.scene_epoch_plan(GROUPS, SIZES, 32, **kw)
    with pytest.raises(ValueError, match="gamma"):
        D.scene_epoch_plan(GROUPS, SIZES, 32, 8, gamma=(0, 50))


# epoch_plan(sizes, (32, 48), 3, seed=11, epoch=7, rank=r, world=2, gamma=(60, 120)) as the code gave it BEFORE the draws that
# follow the index list moved into the function it now shares with scene_epoch_plan: index, y0, x0, hflip, vflip, gammas
PINNED_SIZES = [(40, 60), (37, 51), (64, 64), (33, 49), (40, 60), (48, 50), (37, 51)]
PINNED = {0: ([4, 5, 2, 6], [8, 1, 21, 0], [4, 1, 7, 1], [1, 1, 0, 0], [1, 0, 0, 1], [0.8, 0.84]),
          1: ([3, 1, 0, 4], [0, 5, 2, 8], [1, 1, 2, 0], [0, 0, 1, 1], [1, 1, 0, 0], [1.02, 1.19])}


def test_epoch_plan_is_unchanged_by_the_shared_tail():
    """A regression guard for the permutation sampler: epoch_plan and scene_epoch_plan share what follows the index list
    (_rest_of_plan), and epoch_plan's plans must be, value for value, the ones recorded before that was factored out -- both
    through epoch_plan and through the shared function fed the permutation by hand"""
    D = _D()
    for rank, want in PINNED.items():
        p = D.epoch_plan(PINNED_SIZES, (32, 48), 3, seed=11, epoch=7, rank=rank, world=2, gamma=(60, 120))
        g = torch.Generator(device="cpu")
        g.manual_seed(D._epoch_seed(11, 7))
        padded = torch.randperm(7, generator=g).repeat(2)[:8]
        q = D._rest_of_plan(g, padded, PINNED_SIZES, 32, 48, 4, rank, 2, 3, False, (60, 120))
        for got in (p, q):
            assert [c.long().tolist() for c in (got.index, got.y0, got.x0, got.hflip, got.vflip)] == list(want[:5])
            assert got.gammas == want[5] and got.batches == [(0, 3), (3, 4)] and got.crop == (32, 48)


# ---- scene_pairs ---------------------------------------------------------------------------------------------------------
def _save(path, seed, hw=(9, 11)):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(R.random_images(seed, [hw])[0], "RGB").save(path)


def _tree(tmp_path, low_files, high_files):
    low, high = str(tmp_path / "low"), str(tmp_path / "high")
    os.makedirs(low)
    os.makedirs(high)
    for k, f in enumerate(low_files):
        _save(os.path.join(low, f), k)
    for k, f in enumerate(high_files):
        _save(os.path.join(high, f), 100 + k)
    return low, high


def test_scene_pairs_by_name(tmp_path):
    D = _D()
    low, high = _tree(tmp_path, ["s2/b.png", "s2/a.png", "s1/x.jpg", "s2/orphan.png", "s3/q.png"],
                      ["s2/a.png", "s2/b.png", "s1/x.jpg"])
    os.makedirs(os.path.join(low, "empty"))
    with pytest.warns(UserWarning, match="s2/orphan.png"):
        fp = D.scene_pairs(low, high, "name")
    assert fp.names == ["s1/x.jpg", "s2/a.png", "s2/b.png"] and fp.groups == [("s1", [0]), ("s2", [1, 2])]
    assert sorted(fp.skipped) == ["s2/orphan.png", "s3/q.png"]
    assert fp.paths[1] == (os.path.join(low, "s2", "a.png"), os.path.join(high, "s2", "a.png"))


def test_scene_pairs_first(tmp_path):
    D = _D()
    low, high = _tree(tmp_path, ["s1/0.1.png", "s1/0.04.png", "s2/k.png"], ["s1/long_b.png", "s1/long_a.png", "s2/only.png"])
    fp = D.scene_pairs(low, high, "first")
    assert fp.names == ["s1/0.04.png", "s1/0.1.png", "s2/k.png"] and fp.groups == [("s1", [0, 1]), ("s2", [2])]
    assert fp.paths[0][1] == fp.paths[1][1] == os.path.join(high, "s1", "long_a.png")
    assert fp.paths[2][1] == os.path.join(high, "s2", "only.png") and fp.skipped == []


def test_scene_pairs_label(tmp_path):
    D = _D()
    low, high = _tree(tmp_path, ["7/1.JPG", "7/2.JPG", "7/3.JPG", "12/1.png", "30/1.JPG", "30/2.JPG", "both/1.png"],
                      ["7.JPG", "12.png", "both.png", "both.jpg", "unused.JPG"])
    os.makedirs(os.path.join(low, "empty"))                      # an empty sub-folder is no scene
    _save(os.path.join(high, "empty.JPG"), 77)
    with pytest.warns(UserWarning, match="30/1.JPG, 30/2.JPG"):
        fp = D.scene_pairs(low, high, "label")
    assert fp.names == ["12/1.png", "7/1.JPG", "7/2.JPG", "7/3.JPG", "both/1.png"]
    assert fp.groups == [("12", [0]), ("7", [1, 2, 3]), ("both", [4])]
    assert fp.skipped == ["30/1.JPG", "30/2.JPG"]
    assert [gp for _, gp in fp.paths] == [os.path.join(high, "12.png")] + [os.path.join(high, "7.JPG")] * 3 + \
        [os.path.join(high, "both.jpg")]                         # the first extension of GT_EXTENSIONS that exists
    assert len(fp) == 5
    low_t, gt = fp[1]
    assert low_t.shape == (3, 9, 11) and gt.shape == (9, 11, 3)
    with pytest.raises(ValueError, match="gt must be"):
        D.scene_pairs(low, high, "stem")
    # the plan over these scenes draws nothing else
    p = D.scene_epoch_plan(fp.groups, [(9, 11)] * 5, (8, 8), 4, samples=64, names=fp.names)
    assert set(p.index.tolist()) == {0, 1, 2, 3, 4}


def test_public_names():
    import hvi_cidnet_amd as P
    assert P.scene_pairs is _D().scene_pairs and P.scene_epoch_plan is _D().scene_epoch_plan
    assert {"scene_pairs", "scene_epoch_plan"} <= set(P.__all__)
