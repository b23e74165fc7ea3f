"""GPU: BRISQUE on the device (csrc/brisque.hip through metrics.brisque_gray / brisque_half / brisque_mscn / brisque_fit /
brisque_features / brisque_score / brisque) against the scipy restatement tests/brisque_ref.py, stage by stage and whole.

Both sides are fp64 and differ in summation order only, over at most about 1e4 terms.  Gray, MSCN and half size: 1e-12
absolute.  Moments and features: 1e-9 relative -- looser would hide a dropped pair or a miscounted element; the counts are
exact.  The score with BrisqueParams.random(): 1e-9 relative.  The shapes sit where the tiling can go wrong: the minimum, odd
sizes with the half-to-even rounding, exactly one tile, one tile plus a pixel on either axis and on both (a 1-wide ragged tile
whose pairs cross the tile edge), one tile less a pixel, and 130 x 70 in a batch of three.  Every input is clear of flat
regions (min |Y - mu| >= 1e-9 over both scales in the restatement): there a pixel's side of zero would follow the summation
order, on the host as here.  The observed maxima are printed."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import brisque_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ABS = 1e-12
REL = 1e-9
MARGIN = 1e-9
T = R.TILE
# (h, w, seed, kind): kind 0 = uint8 noise, 1 = a smooth ramp plus uint8 noise.  The seeds were checked on the CPU: clear of
# flat regions, and a root for every map of both scales (the 49 .. 64 elements of the smallest half-size maps do not always
# have one).
SHAPES = [(16, 16, 7, 0), (17, 23, 3, 1), (T, T, 2, 0), (T + 1, T, 1, 1), (T, T + 1, 1, 0), (T + 1, T + 1, 1, 1), (T - 1, T - 1, 1, 0),
          (130, 70, 1, 1)]


@functools.lru_cache(maxsize=None)
def _image(h, w, seed, kind):
    """uint8 (3,h,w), read-only, clear of flat regions and with a finite fit on every map of both scales"""
    rng = np.random.default_rng(seed)
    if kind == 0:
        img = np.clip(rng.normal(128, 45, (3, h, w)), 0, 255).astype(np.uint8)
    else:
        yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
        base = np.stack([40 + 150 * (0.5 * xx + 0.5 * yy) * (1 - 0.2 * c) for c in range(3)])
        img = np.clip(base + rng.normal(0, 25, (3, h, w)), 0, 255).astype(np.uint8)
    assert R.min_margin(img) >= MARGIN, (h, w, seed, kind)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _ref(h, w, seed, kind):
    """the restatement's stages of one image, computed once and shared"""
    img = _image(h, w, seed, kind)
    y = R.gray(img)
    y2 = R.half(y)
    m, m2 = R.mscn(y), R.mscn(y2)
    out = dict(y=y, y2=y2, m=m, m2=m2, tm=R.tile_moments(m), tm2=R.tile_moments(m2), f=R.features(img))
    assert np.isfinite(out["f"]).all(), (h, w, seed, kind)
    return out


def _plan(h, w):
    from hvi_cidnet_amd import _lib
    buf = (ctypes.c_int * 9)()
    assert _lib.lib().raw("cidnet_metric_brisque_plan")(h, w, buf, 9) == 0
    return dict(zip(("tile", "tiles_y", "tiles_x", "h2", "w2", "tiles_y2", "tiles_x2", "lds", "ws_floats"), buf))


def _rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(want).all() and np.isfinite(got).all()
    nz = want != 0
    assert np.array_equal(got[~nz], want[~nz])
    return float((np.abs(got[nz] - want[nz]) / np.abs(want[nz])).max()) if nz.any() else 0.0


def _moments_check(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got[..., (0, 2)], want[..., (0, 2)]), what          # the counts are exact
    e = _rel(got[..., (1, 3, 4, 5)], want[..., (1, 3, 4, 5)])
    print(f"brisque {what}: max relative moment error {e:.3e}")
    assert e <= REL, (what, e)


@pytest.mark.parametrize("h,w,seed,kind", SHAPES)
def test_stages_and_whole_match_the_restatement(dev, h, w, seed, kind):
    from hvi_cidnet_amd import metrics as M
    img, ref = _image(h, w, seed, kind), _ref(h, w, seed, kind)
    p = _plan(h, w)
    assert p["tile"] == T and (p["tiles_y"], p["tiles_x"]) == (-(-h // T), -(-w // T))
    assert (p["h2"], p["w2"]) == R.half_shape(h, w) and (p["tiles_y2"], p["tiles_x2"]) == (-(-p["h2"] // T), -(-p["w2"] // T))
    q = torch.from_numpy(np.array(img)).to(dev).unsqueeze(0)                 # a writable copy of the shared image
    y = M.brisque_gray(q)
    assert y.dtype == torch.float64 and tuple(y.shape) == (1, h, w)
    e_gray = np.abs(y[0].cpu().numpy() - ref["y"]).max()
    y_ref = torch.from_numpy(ref["y"]).to(dev)
    y2 = M.brisque_half(y_ref)
    assert tuple(y2.shape) == (1, p["h2"], p["w2"])
    e_half = np.abs(y2[0].cpu().numpy() - ref["y2"]).max()
    print(f"brisque {h} x {w}: max |gray - ref| = {e_gray:.3e}, max |half - ref| = {e_half:.3e}")
    assert e_gray <= ABS and e_half <= ABS
    # MSCN and the tile moments: the fp64 plane path on the restatement's own planes, the uint8 path on the image
    for plane, key, tiles in ((y_ref, "", p["tiles_y"] * p["tiles_x"]), (torch.from_numpy(ref["y2"]).to(dev), "2", p["tiles_y2"] * p["tiles_x2"])):
        m, mom = M.brisque_mscn(plane)
        assert tuple(mom.shape) == (1, tiles, 5, 6) and m.dtype == torch.float64
        e = np.abs(m[0].cpu().numpy() - ref["m" + key]).max()
        print(f"brisque {h} x {w} scale {key or 1}: max |mscn - ref| = {e:.3e}")
        assert e <= ABS
        _moments_check(mom[0].cpu().numpy(), ref["tm" + key], f"{h} x {w} scale {key or 1} tiles")
        f18 = M.brisque_fit(mom)[0].cpu().numpy()
        e = _rel(f18, ref["f"][18:] if key else ref["f"][:18])
        print(f"brisque {h} x {w} scale {key or 1}: max relative feature error of the fit stage {e:.3e}")
        assert e <= REL
    m8, mom8 = M.brisque_mscn(q)
    assert np.abs(m8[0].cpu().numpy() - ref["m"]).max() <= ABS
    _moments_check(mom8[0].cpu().numpy(), ref["tm"], f"{h} x {w} uint8 staging")
    f = M.brisque_features(q)
    assert f.dtype == torch.float64 and tuple(f.shape) == (1, 36) and f.device == q.device
    e_f = _rel(f[0].cpu().numpy(), ref["f"])
    prm = M.BrisqueParams.random(seed)
    s = M.brisque(q, prm)
    assert s.dtype == torch.float64 and tuple(s.shape) == (1,)
    want = R.svr(ref["f"], prm.sv, prm.coef, prm.rho, prm.gamma, prm.fmin, prm.fmax)
    e_s = abs(s.item() - want) / abs(want)
    print(f"brisque {h} x {w}: max relative feature error {e_f:.3e}, score {s.item():.12g} against {want:.12g}: {e_s:.3e}")
    assert e_f <= REL and e_s <= REL
    assert torch.equal(M.brisque_score(f, prm), s)
    assert torch.equal(M.brisque(q[0], prm), s)                    # a (3,h,w) image is a batch of one


def test_batch_rows_equal_their_batch_of_one_bit_for_bit(dev):
    from hvi_cidnet_amd import metrics as M
    h, w = 130, 70
    imgs = [_image(h, w, s, k) for s, k in ((1, 1), (2, 0), (3, 1))]
    assert not np.array_equal(imgs[0], imgs[1]) and not np.array_equal(imgs[1], imgs[2])
    q = torch.from_numpy(np.stack(imgs)).to(dev)
    prm = M.BrisqueParams.random(4, n_sv=1500)                     # more than one chunk of the SVR kernel
    f, s = M.brisque_features(q), M.brisque(q, prm)
    p = _plan(h, w)
    assert (p["tiles_y"], p["tiles_x"], p["tiles_y2"], p["tiles_x2"]) == (5, 3, 3, 2) and (p["h2"], p["w2"]) == (65, 35)
    assert _lib_ws(3, h, w) == 3 * p["ws_floats"]
    for i in range(3):
        assert torch.equal(M.brisque_features(q[i:i + 1])[0], f[i]), i
        assert torch.equal(M.brisque(q[i:i + 1], prm)[0], s[i]), i
        ref = R.features(imgs[i])
        want = R.svr(ref, prm.sv, prm.coef, prm.rho, prm.gamma, prm.fmin, prm.fmax)
        e_f, e_s = _rel(f[i].cpu().numpy(), ref), abs(s[i].item() - want) / abs(want)
        print(f"brisque batch row {i}: feature error {e_f:.3e}, score error {e_s:.3e}")
        assert e_f <= REL and e_s <= REL
    # two calls are bit-identical
    assert torch.equal(M.brisque_features(q), f) and torch.equal(M.brisque(q, prm), s)


def _lib_ws(B, h, w):
    from hvi_cidnet_amd import _lib
    return _lib.lib().raw("cidnet_metric_brisque_ws_floats")(B, h, w)


def test_flat_images_give_nan_and_do_not_fault(dev):
    from hvi_cidnet_amd import metrics as M
    prm = M.BrisqueParams.random(0)
    for h, w in ((16, 16), (40, 33)):
        q = torch.zeros((2, 3, h, w), dtype=torch.uint8, device=dev)
        f, s = M.brisque_features(q), M.brisque(q, prm)
        assert torch.isnan(f).all() and torch.isnan(s).all() and tuple(s.shape) == (2,)
    # an all-equal image that is not black: the zero fill gives its border real values and its interior rounding noise, whose
    # sides follow the summation order -- nothing is compared with the host; it runs, and runs the same twice
    q = torch.full((1, 3, 40, 33), 128, dtype=torch.uint8, device=dev)
    a, b = M.brisque_features(q), M.brisque_features(q)
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    torch.cuda.synchronize()


def test_bad_inputs_raise(dev):
    from hvi_cidnet_amd import metrics as M
    prm = M.BrisqueParams.random(0)
    cpu = torch.zeros((1, 3, 16, 16), dtype=torch.uint8)
    for fn in (lambda: M.brisque(cpu, prm), lambda: M.brisque_features(cpu), lambda: M.brisque_gray(cpu),
               lambda: M.brisque_half(torch.zeros((16, 16), dtype=torch.float64)),
               lambda: M.brisque_mscn(torch.zeros((16, 16), dtype=torch.float64)),
               lambda: M.brisque_score(torch.zeros((1, 36), dtype=torch.float64), prm)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    with pytest.raises(RuntimeError, match="uint8"):
        M.brisque(torch.zeros((1, 3, 16, 16), device=dev), prm)
    with pytest.raises(ValueError, match="16 x 16"):
        M.brisque(torch.zeros((1, 3, 15, 16), dtype=torch.uint8, device=dev), prm)
    with pytest.raises(ValueError, match="not shipped|is shipped"):
        M.brisque(torch.zeros((1, 3, 16, 16), dtype=torch.uint8, device=dev), None)
    with pytest.raises(RuntimeError, match="36"):
        M.brisque_score(torch.zeros((1, 35), dtype=torch.float64, device=dev), prm)
