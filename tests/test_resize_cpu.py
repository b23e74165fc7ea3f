"""CPU: the host side of the resized evaluation -- metrics.resize_plan against Pillow itself (the numpy restatement of the
two fixed-point passes, driven by the plan's tables, reproduces Image.resize byte for byte), the tables' shape at both
borders, the resize entry point's argument and size checks (host only: nothing is launched), and the nested folder sets."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_ref as R  # noqa: E402


@pytest.mark.parametrize("src,dst", R.CASES + [R.WIDE])
def test_plan_reproduces_pil(src, dst):
    from hvi_cidnet_amd import metrics as M
    for kind in R.KINDS:
        img = R.image(kind, *src)
        got, ref = R.restated(img, dst, M.resize_plan), R.pil_resize(img, dst)
        assert got.shape == ref.shape and np.array_equal(got, ref), (kind, int((got != ref).sum()))


def test_plan_tables_at_the_borders():
    from hvi_cidnet_amd import metrics as M
    # 300 -> 7: scale 42.86, support 85.71, ksize = 86 * 2 + 1
    bounds, coeffs = M.resize_plan(300, 7)
    assert bounds.dtype == np.int32 and coeffs.dtype == np.int32
    assert bounds.shape == (7, 2) and coeffs.shape == (7, 173)
    assert bounds[0, 0] == 0 and bounds[0, 1] == int(21.428571428571427 + 85.71428571428571 + 0.5)      # clipped at the left
    assert bounds[-1, 0] + bounds[-1, 1] == 300                                                      # clipped at the right
    assert bounds[3].tolist() == [64, 172]                     # the middle row is whole: 172 taps
    for (first, count), row in zip(bounds, coeffs):
        assert 0 <= first and first + count <= 300 and 0 < count <= 173
        assert not row[count:].any()                           # padded with zeros
        assert abs(int(row.sum()) - (1 << 22)) <= count        # normalised: each tap rounds by at most a half
    # 9 -> 12: an enlargement keeps the filter's own support of 2, ksize = 5
    bounds, coeffs = M.resize_plan(9, 12)
    assert bounds.shape == (12, 2) and coeffs.shape == (12, 5)
    assert bounds[0].tolist() == [0, 2] and bounds[-1].tolist() == [7, 2]
    assert bounds[:, 1].max() == 4 and (bounds[:, 0] + bounds[:, 1]).max() == 9
    assert not coeffs[0, 2:].any() and not coeffs[-1, 2:].any()
    assert (coeffs < 0).any()                                  # the negative lobes are there
    assert M.resize_plan(9, 12)[1] is coeffs                   # cached
    with pytest.raises(ValueError):
        coeffs[0, 0] = 1                                       # and read-only
    with pytest.raises(ValueError):
        M.resize_plan(0, 4)


def test_entry_point_checks_before_it_launches():
    """cidnet_metric_resize_ws_bytes, and the argument / size checks of cidnet_metric_resize_u8, which come before any
    launch: the pointers here are never dereferenced"""
    from hvi_cidnet_amd import _lib
    L = _lib.lib()
    ws, rs = L.raw("cidnet_metric_resize_ws_bytes"), L.raw("cidnet_metric_resize_u8")
    assert ws(2, 24, 40, 17, 29) == 2 * 3 * 24 * 29
    assert ws(2, 24, 40, 24, 31) == 0 and ws(2, 24, 40, 13, 40) == 0 and ws(1, 8, 8, 8, 8) == 0 and ws(0, 8, 8, 4, 4) == 0
    p = ctypes.c_void_p(4096)
    assert rs(None, p, p, p, p, 5, p, p, 5, 1, 8, 8, 4, 4, None) == -1
    assert rs(p, p, None, p, p, 5, p, p, 5, 1, 8, 8, 4, 4, None) == -1           # both passes need tmp
    assert rs(p, p, p, None, p, 5, p, p, 5, 1, 8, 8, 4, 4, None) == -1           # a running pass needs its tables
    assert rs(p, p, p, p, p, 5, p, p, 0, 1, 8, 8, 4, 4, None) == -1
    assert rs(p, p, p, p, p, 5, p, p, 5, 1, 8, 0, 4, 4, None) == -1
    # 2^31 bytes or more on either side, or in tmp: refused, not wrapped
    assert rs(p, p, p, p, p, 5, p, p, 5, 1, 32768, 21846, 4, 4, None) == -2      # src: 3 * 32768 * 21846 >= 2^31
    assert rs(p, p, p, p, p, 5, p, p, 5, 1, 4, 4, 32768, 21846, None) == -2      # dst
    assert rs(p, p, p, p, p, 5, p, p, 5, 1, 1000000, 4, 4, 1000, None) == -2     # tmp (B,3,h_in,w_out)
    assert rs(p, p, None, None, None, 0, p, p, 5, 2, 32768, 10923, 4, 10923, None) == -2    # B counts


def _tree(root, layout, rng):
    from PIL import Image
    for sub, files in layout.items():
        os.makedirs(os.path.join(root, sub))
        for f in files:
            Image.fromarray(rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)).save(os.path.join(root, sub, f))


def test_nested_folder_pairs_and_group_means(tmp_path):
    from hvi_cidnet_amd import metrics as M
    rng = np.random.default_rng(0)
    low, high = str(tmp_path / "low"), str(tmp_path / "high")
    _tree(low, {"0002": ["b.png", "a.png"], "0001": ["x.png", "y.png", "z.png"], "0003": ["q.png"], "0004": ["a.png"]}, rng)
    _tree(high, {"0001": ["y.png", "x.png", "z.png"], "0002": ["a.png"], "0004": ["m.png", "k.png"]}, rng)
    open(os.path.join(low, "stray.png"), "wb").close()          # files beside the sub-folders are not part of the set
    open(os.path.join(low, "0001", "notes.txt"), "w").close()

    with pytest.warns(UserWarning, match="no ground truth"):
        by_name = M.nested_folder_pairs(low, high, gt="name")
    assert by_name.names == ["0001/x.png", "0001/y.png", "0001/z.png", "0002/a.png"]
    assert by_name.skipped == ["0002/b.png", "0003/q.png", "0004/a.png"]
    assert by_name.groups == [("0001", [0, 1, 2]), ("0002", [3])]
    assert by_name.paths[1] == (os.path.join(low, "0001", "y.png"), os.path.join(high, "0001", "y.png"))
    x, g = by_name[3]
    assert tuple(x.shape) == (3, 6, 7) and g.shape == (6, 7, 3) and g.dtype == np.uint8

    with pytest.warns(UserWarning, match="0003/q.png"):
        first = M.nested_folder_pairs(low, high, gt="first")
    assert first.names == ["0001/x.png", "0001/y.png", "0001/z.png", "0002/a.png", "0002/b.png", "0004/a.png"]
    assert first.skipped == ["0003/q.png"]                       # the sub-folder is missing on the high side
    assert first.groups == [("0001", [0, 1, 2]), ("0002", [3, 4]), ("0004", [5])]
    assert [os.path.relpath(p[1], high) for p in first.paths] == ["0001/x.png"] * 3 + ["0002/a.png"] * 2 + ["0004/k.png"]
    with pytest.raises(ValueError):
        M.nested_folder_pairs(low, high, gt="last")

    vals = {k: [float(v) for v in rng.random(6) * 30] for k in ("psnr", "ssim", "psnr_gt_mean", "ssim_gt_mean")}
    res = M.EvalResult(alpha=1.0, psnr=0.0, ssim=0.0, psnr_gt_mean=0.0, ssim_gt_mean=0.0, per_image=vals, names=first.names)
    assert res.resized == []
    per, overall = M.group_means(res, first)
    assert list(per) == ["0001", "0002", "0004"] and [per[s]["n"] for s in per] == [3, 2, 1] and overall["n"] == 6
    for k, v in vals.items():
        assert per["0001"][k] == pytest.approx(sum(v[:3]) / 3, rel=1e-15)
        assert per["0002"][k] == pytest.approx(sum(v[3:5]) / 2, rel=1e-15)
        assert per["0004"][k] == v[5]
        assert overall[k] == pytest.approx(sum(v) / 6, rel=1e-15)                # weighted by images, not by folders
        assert overall[k] != pytest.approx(sum(per[s][k] for s in per) / 3, rel=1e-6)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert M.nested_folder_pairs(high, high).skipped == []
