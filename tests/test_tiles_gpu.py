"""GPU: the tiled mode of hvi_cidnet_amd.image_io -- the window ingest and blended egress kernels (csrc/imageio.hip) alone, then
enhance_u8(tile=) and enhance_folder(tile=) with the reduced-width model.

ingest_tiles compares exactly with a torch restatement (table lookup, F.pad reflect, a slice per origin); a plan of one tile makes
egress_tiles the plain egress, exactly.  The blend is compared with an fp64 restatement built here from plan.wy / plan.wx under
one rule (_check_blend):
  * a pixel covered by one tile is bit-equal to trunc(clamp(v) * 255.0f);
  * a blended value whose covers all clamp to 0, or all to 1, is 0 or 255: acc is then 0, or the very sum den is;
  * every other blended value equals floor(fp64 value * 255) wherever that product is farther than 1e-3 from an integer, and is
    within +-1 of it elsewhere.  1e-3: at most 9 covers, so at most 9 weight products, 9 value products, 8 + 8 sums and one
    division in fp32 -- the issue counts fewer than 20 roundings on the value's path -- each 6e-8 relative, times 255: 3e-4;
  * the share of blended values inside that band stays below 1 %, so that the band cannot hide a failure.  Uniform inputs put
    about 0.2 % there.  The all-0 / all-1 values of the second rule are held to equality instead and do not count: with inputs
    uniform in [-0.1, 1.1] they alone are 1.4 % of the doubly covered values.
The model cases run in a fresh spawned process each, as tests/test_enhance_gpu.py does."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from evaluate_harness import in_child as _in_child, model as _model  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
CIDNET_ERR_ARG, CIDNET_ERR_SHAPE = -1, -2
BAND = 1e-3


def _half(h, w, tile):
    from hvi_cidnet_amd import image_io as IO
    Hp, Wp = IO.padded_size(h, w)
    return min(tile, Hp, Wp) // 2


def _embedded(h, w, seed, dev):
    """a random (h,w,3) uint8 image holding all 256 levels, inside a larger buffer of random bytes at an odd address"""
    g = torch.Generator().manual_seed(seed)
    n = 3 * h * w
    buf = torch.randint(0, 256, (n + 131,), dtype=torch.uint8, generator=g)
    flat = buf[67:67 + n]
    where = torch.randperm(n, generator=g)[:min(256, n)]
    flat[where] = torch.arange(256, dtype=torch.int64)[:len(where)].to(torch.uint8)
    buf = buf.to(dev)
    view = buf[67:67 + n].view(h, w, 3)
    assert view.data_ptr() % 2 == 1
    return buf, view


def _windows(img, table, plan):
    """the restatement: F.pad(..., 'reflect') of the table lookup, sliced at each origin -> (n,3,th,tw)"""
    h, w = plan.size
    Hp, Wp = plan.padded
    th, tw = plan.tile
    full = F.pad(table[img.long()].permute(2, 0, 1).unsqueeze(0), (0, Wp - w, 0, Hp - h), "reflect")[0]
    return torch.stack([full[:, y:y + th, x:x + tw] for y, x in plan.origins.tolist()]).contiguous()


def _table(gamma, dev):
    import hvi_cidnet_amd as P
    if gamma == 1.0:
        return torch.arange(256, dtype=torch.float32).div(255).to(dev)
    return torch.from_numpy(P.gamma_table(gamma)).to(dev)


# the last two: origins that are no multiples of 4 (S = 10), and a rectangular tile
INGEST = [(hw, tile, ov) for hw in ((37, 53), (100, 150), (24, 200)) for tile in (16, 64) for ov in (0, 8, "half")] + \
         [((100, 150), 16, 6), ((37, 53), (16, 32), 5)]


@pytest.mark.parametrize("hw,tile,ov", INGEST)
def test_ingest_tiles_is_the_padded_table_lookup_sliced(dev, hw, tile, ov):
    import hvi_cidnet_amd as P
    h, w = hw
    plan = P.tile_plan(h, w, tile, _half(h, w, tile) if ov == "half" else ov)
    buf, view = _embedded(h, w, seed=h * 1000 + w, dev=dev)
    before = buf.clone()
    for gamma in (1.0, 0.6):
        x = P.ingest_tiles(view, plan, gamma=gamma)
        assert x.shape == (len(plan), 3, *plan.tile) and x.dtype == torch.float32
        assert torch.equal(x, _windows(view, _table(gamma, dev), plan)), (hw, tile, ov, gamma)
    assert torch.equal(P.ingest_tiles(view.contiguous().unsqueeze(0), plan), P.ingest_tiles(view, plan))    # (1,h,w,3), aligned
    if len(plan) == 1:                                           # one tile of the padded image's own shape: ingest itself
        assert torch.equal(P.ingest_tiles(view, plan), P.ingest(view)[0])
    assert torch.equal(buf, before)                              # the source is only read


def _tiles_input(plan, seed, dev):
    """(n,3,th,tw): uniform in [-0.1, 1.1] with NaN, +-0, 1 and some q / 255 with their fp32 neighbours planted"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((len(plan), 3, *plan.tile), generator=g) * 1.2 - 0.1
    q = (torch.arange(0, 256, 5, dtype=torch.float32) / 255).numpy()
    levels = np.stack([q, np.nextafter(q, np.float32(2)), np.nextafter(q, np.float32(-1))], axis=1).reshape(-1)
    special = np.concatenate([np.array([np.nan, 0.0, -0.0, 1.0] * 8, dtype=np.float32), levels]).astype(np.float32)
    flat = x.reshape(-1)
    n = min(special.size, flat.numel() // 8)
    flat[torch.randperm(flat.numel(), generator=g)[:n]] = torch.from_numpy(special)[:n]
    return x.to(dev)


def _quant32(v):
    """trunc(clamp(v, 0, 1) * 255.0f) of fp32 values, NaN -> 0"""
    v = np.nan_to_num(np.asarray(v, dtype=np.float32), nan=0.0)
    return (np.clip(v, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)


def _blend64(tiles, plan):
    """the fp64 restatement from plan.wy / plan.wx: tiles (n,3,th,tw) fp32 numpy -> per value of the (h, w) crop: the weighted mean
    of the clamped covers, the number of covers, trunc(clamp * 255.0f) of the last cover (what a single cover must give), and
    the smallest / largest clamped cover"""
    h, w = plan.size
    Hp, Wp = plan.padded
    th, tw = plan.tile
    cl32 = np.clip(np.nan_to_num(tiles, nan=0.0), np.float32(0), np.float32(1))
    acc, den = np.zeros((3, Hp, Wp)), np.zeros((Hp, Wp))
    cnt = np.zeros((Hp, Wp), dtype=np.int64)
    one = np.zeros((3, Hp, Wp), dtype=np.uint8)
    lo, hi = np.full((3, Hp, Wp), np.inf), np.full((3, Hp, Wp), -np.inf)
    t = 0
    for ky, y in enumerate(plan.ys):
        for kx, x in enumerate(plan.xs):
            wgt = np.outer(plan.wy[ky].astype(np.float64), plan.wx[kx].astype(np.float64))
            s = (slice(None), slice(y, y + th), slice(x, x + tw))
            acc[s] += wgt * cl32[t].astype(np.float64)
            den[s[1:]] += wgt
            cnt[s[1:]] += 1
            one[s] = _quant32(cl32[t])
            lo[s], hi[s] = np.minimum(lo[s], cl32[t]), np.maximum(hi[s], cl32[t])
            t += 1
    assert cnt.min() >= 1
    crop = (slice(None), slice(0, h), slice(0, w))
    return (acc / den)[crop], np.broadcast_to(cnt, (3, Hp, Wp))[crop], one[crop], lo[crop], hi[crop]


def _check_blend(got, tiles, plan, what):
    """got: (h,w,3) uint8 numpy against the rule of the module docstring -> the figures"""
    val, cnt, one, lo, hi = _blend64(tiles, plan)
    got = got.transpose(2, 0, 1).astype(np.int64)
    single = cnt == 1
    exact = ~single & (lo == hi) & ((lo == 0) | (lo == 1))
    d = val * 255.0
    fl = np.floor(d).astype(np.int64)
    near = np.abs(d - np.rint(d)) <= BAND
    far, band = ~single & ~exact & ~near, ~single & ~exact & near
    blended = int((~single).sum())
    fig = dict(what=what, values=int(got.size), single=int(single.sum()), blended=blended, exact=int(exact.sum()), band=int(band.sum()),
               band_share=float(band.sum()) / max(1, blended), max_cover=int(cnt.max()),
               single_wrong=int((got != one)[single].sum()), exact_wrong=int((got != np.rint(d))[exact].sum()),
               far_wrong=int((got != fl)[far].sum()), band_worst=int(np.abs(got - fl)[band].max()) if band.any() else 0)
    print(fig)
    assert fig["single_wrong"] == 0, fig
    assert fig["exact_wrong"] == 0, fig
    assert fig["far_wrong"] == 0, fig
    assert fig["band_worst"] <= 1, fig
    assert fig["band_share"] < 0.01, fig
    return fig


@pytest.mark.parametrize("hw", [(37, 53), (100, 150), (24, 200), (9, 13)])
def test_a_plan_of_one_tile_is_egress(dev, hw):
    import hvi_cidnet_amd as P
    h, w = hw
    plan = P.tile_plan(h, w, 256)
    assert len(plan) == 1
    x = _tiles_input(plan, seed=h + w, dev=dev)
    assert torch.equal(P.egress_tiles(x, plan), P.egress(x[0], (h, w))[0])


# (104-high padded image, tile 64, overlap 32): rows 40..63 under three tiles; S = 10: groups of four that straddle a tile's edge;
# overlap 0: only the flush tiles overlap their neighbours; a rectangular tile; one axis with a single tile
BLEND = [((100, 150), 64, 32), ((37, 53), 16, 8), ((37, 53), 16, 0), ((100, 150), 16, 6), ((100, 150), (32, 64), 12), ((24, 200), 64, 12),
         ((100, 151), (24, 40), 7)]


@pytest.mark.parametrize("hw,tile,ov", BLEND)
def test_egress_tiles_against_the_fp64_blend_and_writes_nothing_else(dev, hw, tile, ov):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib, image_io as IO, ops
    h, w = hw
    plan = P.tile_plan(h, w, tile, ov)
    x = _tiles_input(plan, seed=h * 7 + w, dev=dev)
    q = P.egress_tiles(x, plan)
    assert q.shape == (h, w, 3) and q.dtype == torch.uint8
    fig = _check_blend(q.cpu().numpy(), x.cpu().numpy(), plan, (hw, tile, ov))
    assert fig["blended"] > 0 and fig["single"] > 0
    if (hw, tile, ov) == ((100, 150), 64, 32):
        assert plan.padded[0] == 104 and fig["max_cover"] == 9   # the triple cover, on both axes
    # through the raw ABI into a sentinel-filled buffer at an odd address: the same bytes, and not one more
    buf = torch.full((1 + 3 * h * w + 64,), SENTINEL, dtype=torch.uint8, device=dev)
    dst = buf[1:]
    assert dst.data_ptr() % 2 == 1
    _, ys, xs, wy, wx = IO._plan_on(plan, x.device)
    _lib.lib().call("cidnet_image_egress_tiles", ops._p(x), ops._p(ys), len(plan.ys), ops._p(xs), len(plan.xs), ops._p(wy), ops._p(wx),
                    ops._p(dst), h, w, *plan.tile, ops._stream())
    assert torch.equal(dst[:3 * h * w].view(h, w, 3), q)
    assert bool(buf[0] == SENTINEL) and bool((dst[3 * h * w:] == SENTINEL).all()), "bytes outside the image written"
    assert torch.equal(P.egress_tiles(x, plan), q)               # bit-identical from call to call


def test_rejections(dev):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib, image_io as IO, ops
    plan = P.tile_plan(37, 53, 16, 8)
    img = torch.zeros((37, 53, 3), dtype=torch.uint8, device=dev)
    x = torch.zeros((len(plan), 3, 16, 16), dtype=torch.float32, device=dev)
    q = torch.zeros((37, 53, 3), dtype=torch.uint8, device=dev)
    origins, ys, xs, wy, wx = IO._plan_on(plan, dev)
    assert IO._plan_on(plan, dev)[0] is origins                  # uploaded once per plan
    st = ops._stream()
    ing, egr = _lib.lib().raw("cidnet_image_ingest_tiles"), _lib.lib().raw("cidnet_image_egress_tiles")
    n, ny, nx = len(plan), len(plan.ys), len(plan.xs)
    assert ing(ops._p(img), 37, 53, None, ops._p(origins), ops._p(x), n, 16, 16, st) == 0
    assert ing(None, 37, 53, None, ops._p(origins), ops._p(x), n, 16, 16, st) == CIDNET_ERR_ARG
    assert ing(ops._p(img), 37, 53, None, None, ops._p(x), n, 16, 16, st) == CIDNET_ERR_ARG
    assert ing(ops._p(img), 37, 53, None, ops._p(origins), None, n, 16, 16, st) == CIDNET_ERR_ARG
    for bad in ((0, 53, n, 16, 16), (37, 0, n, 16, 16), (37, 53, 0, 16, 16), (37, 53, n, 0, 16), (37, 53, n, 16, -4)):
        assert ing(ops._p(img), bad[0], bad[1], None, ops._p(origins), ops._p(x), *bad[2:], st) == CIDNET_ERR_ARG, bad
    for bad in ((n, 18, 16), (n, 16, 18), (65536, 16, 16)):
        assert ing(ops._p(img), 37, 53, None, ops._p(origins), ops._p(x), *bad, st) == CIDNET_ERR_SHAPE, bad
    good = [ops._p(x), ops._p(ys), ny, ops._p(xs), nx, ops._p(wy), ops._p(wx), ops._p(q), 37, 53, 16, 16]
    assert egr(*good, st) == 0
    for i in (0, 1, 3, 5, 6, 7):
        assert egr(*good[:i], None, *good[i + 1:], st) == CIDNET_ERR_ARG, i
    for i in (2, 4, 8, 9, 10, 11):
        assert egr(*good[:i], 0, *good[i + 1:], st) == CIDNET_ERR_ARG, i
    for i, v in ((10, 18), (11, 18), (2, 1025), (4, 1025)):
        assert egr(*good[:i], v, *good[i + 1:], st) == CIDNET_ERR_SHAPE, (i, v)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="plan is for one"):
        P.ingest_tiles(torch.zeros((36, 53, 3), dtype=torch.uint8, device=dev), plan)
    with pytest.raises(RuntimeError, match="plan is for one"):
        P.ingest_tiles(torch.zeros((2, 37, 53, 3), dtype=torch.uint8, device=dev), plan)
    with pytest.raises(RuntimeError, match="for this plan"):
        P.egress_tiles(x[:-1], plan)
    with pytest.raises(RuntimeError, match="fp32"):
        P.egress_tiles(x.double(), plan)
    with pytest.raises(ValueError, match="gamma"):
        P.ingest_tiles(img, plan, gamma=0.0)
    with pytest.raises(ValueError, match="tile_batch"):
        P.enhance_u8(torch.nn.Identity(), img, tile=16, overlap=8, tile_batch=0)
    with pytest.raises(ValueError, match="multiple"):
        P.enhance_u8(torch.nn.Identity(), img, tile=20, overlap=8)
    with pytest.raises(ValueError, match="overlap"):
        P.enhance_u8(torch.nn.Identity(), img, tile=16)          # the default overlap of 32 is more than half of this tile


# ---- with a model ---------------------------------------------------------------------------------------------------------
CFG = dict(gamma=0.6, gated=True, alpha_s=1.2, gated2=True, alpha=0.9)


def _image(h, w, seed=21):
    return np.random.default_rng(seed).integers(0, 160, size=(h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("cls_name", ["CIDNet", "CIDNet_TNSM"])
def test_enhance_u8_tiled(dev, cls_name):
    _in_child(_case_enhance_u8_tiled, cls_name)


def _case_enhance_u8_tiled(cls_name):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import metrics as M
    dev = torch.device("cuda:0")
    m = _model(cls_name)
    t = m.trans
    t.gated, t.alpha_s, t.gated2, t.alpha = False, 1.1, False, 0.7
    m.train()
    m.HV_LCA1.eval()                                             # a mixed-mode module tree comes back as it was
    modes = [mod.training for mod in m.modules()]
    img = torch.from_numpy(_image(100, 150)).to(dev)

    def unchanged():
        return [mod.training for mod in m.modules()] == modes and (t.gated, t.alpha_s, t.gated2, t.alpha) == (False, 1.1, False, 0.7)

    # a tile no smaller than the padded image: one tile, the whole-image path's bytes
    assert torch.equal(P.enhance_u8(m, img, tile=256, **CFG), P.enhance_u8(m, img, **CFG)) and unchanged()

    plan = P.tile_plan(100, 150, 64, 16)
    assert len(plan) == 6                                        # chunks of 4 and 2: the last one is short
    q = P.enhance_u8(m, img, tile=64, overlap=16, tile_batch=4, **CFG)
    assert q.shape == (1, 100, 150, 3) and q.dtype == torch.uint8 and unchanged()
    # windows cut by torch -> the model per chunk -> fp64 blend -> quantise
    x = _windows(img, torch.from_numpy(P.gamma_table(CFG["gamma"])).to(dev), plan)
    attrs = {k: CFG[k] for k in ("gated", "alpha_s", "gated2", "alpha")}
    with torch.no_grad(), M._eval_state(m, attrs):
        outs = [m(x[lo:lo + 4]) for lo in range(0, 6, 4)]
    y = torch.cat([o[0] if isinstance(o, tuple) else o for o in outs])
    assert y.shape == x.shape and unchanged()
    _check_blend(q[0].cpu().numpy(), y.cpu().numpy(), plan, cls_name)
    assert torch.equal(P.egress_tiles(y, plan), q[0])            # and exactly the egress of those tiles
    if cls_name == "CIDNet":                                     # a batch of two images: each on its own
        two = torch.stack([img, torch.from_numpy(_image(100, 150, seed=3)).to(dev)])
        q2 = P.enhance_u8(m, two, tile=64, overlap=16, tile_batch=4, **CFG)
        assert torch.equal(q2[0], q[0]) and torch.equal(q2[1:], P.enhance_u8(m, two[1], tile=64, overlap=16, tile_batch=4, **CFG))
    assert m.training and not m.HV_LCA1.training


def test_enhance_folder_tiled(dev, tmp_path):
    _in_child(_case_folder_tiled, str(tmp_path))


def _case_folder_tiled(tmp):
    from PIL import Image
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd.metrics import _read_rgb
    dev = torch.device("cuda:0")
    m = _model()
    sizes = [(100, 150), (70, 90), (64, 200)]
    src, out_a, out_b = (os.path.join(tmp, d) for d in ("in", "out_a", "out_b"))
    os.makedirs(src)
    names = [f"im{i}.png" for i in range(len(sizes))]
    for i, (n, (h, w)) in enumerate(zip(names, sizes)):
        Image.fromarray(_image(h, w, seed=i)).save(os.path.join(src, n))
    rep = P.enhance_folder(m, src, out_a, batch_size=4, threads=4, depth=2, tile=64, **CFG)
    assert rep.names == names and rep.sizes == sizes
    assert rep.batches == [[0], [1], [2]]                        # each image on its own, whatever batch_size says
    assert rep.tiles == [len(P.tile_plan(h, w, 64)) for h, w in sizes] == [12, 4, 6]
    assert sorted(os.listdir(out_a)) == names
    for n in names:
        ref = P.enhance_u8(m, torch.from_numpy(_read_rgb(os.path.join(src, n))).to(dev), tile=64, **CFG)[0].cpu().numpy()
        assert np.array_equal(_read_rgb(os.path.join(out_a, n)), ref), n
    rep_b = P.enhance_folder(m, src, out_b, threads=1, depth=1, tile=64, **CFG)               # the serial order
    assert rep_b.tiles == rep.tiles and rep_b.batches == rep.batches
    for n in names:
        with open(os.path.join(out_a, n), "rb") as fa, open(os.path.join(out_b, n), "rb") as fb:
            assert fa.read() == fb.read(), n
    assert P.enhance_folder(m, src, os.path.join(tmp, "out_c"), **CFG).tiles == []             # untiled: no tile counts
    for kw in (dict(tile=20), dict(tile=64, overlap=-1), dict(tile=64, tile_batch=0)):          # refused before anything starts
        with pytest.raises(ValueError) as e:
            P.enhance_folder(m, src, os.path.join(tmp, "out_d"), **kw)
        assert "im0" not in str(e.value) and not os.path.exists(os.path.join(tmp, "out_d"))
    with pytest.raises(ValueError, match="im0.png"):                                             # this one depends on the image
        P.enhance_folder(m, src, os.path.join(tmp, "out_d"), tile=64, overlap=40)
    assert m.training and m.trans.alpha == 1.0
