"""CPU: the host side of BRISQUE -- metrics.load_brisque_params against a model that scikit-learn's SVR (libsvm itself) has
fitted and predicts from, the loader's errors, and the restatement tests/brisque_ref.py held against the scipy routines the
contract names (the even-size identity and the odd-size shapes of the half-size stage, the root against scipy.optimize.root).
No kernel is launched here."""
import os
import pickle
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import brisque_ref as R  # noqa: E402


def _write_model(path, sv, coef, rho, gamma, svm_type="epsilon_svr", kernel_type="rbf", drop=0, total=None):
    """a libsvm text model, exact zeros left out (the sparse form), the last `drop` support vectors missing"""
    n = len(coef)
    lines = [f"svm_type {svm_type}", f"kernel_type {kernel_type}", f"gamma {gamma!r}", "nr_class 2",
             f"total_sv {n if total is None else total}", f"rho {rho!r}", "SV"]
    for v, c in list(zip(sv, coef))[:n - drop]:
        lines.append(" ".join([repr(float(c))] + [f"{k + 1}:{float(x)!r}" for k, x in enumerate(v) if x != 0.0]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def _fitted():
    from sklearn.svm import SVR
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (60, 36))
    x[rng.random(x.shape) < 0.2] = 0.0                              # exact zeros: absent indices in the file
    y = np.sin(x[:, :5].sum(axis=1)) * 20 + 30 + rng.normal(0, 1, 60)
    return SVR(kernel="rbf", gamma=0.05, C=10.0, epsilon=0.5).fit(x, y), rng


def test_loader_reproduces_libsvm_predictions(tmp_path):
    from hvi_cidnet_amd import metrics as M
    svr, rng = _fitted()
    sv, coef, rho = svr.support_vectors_, svr.dual_coef_[0], -float(svr.intercept_[0])
    assert (sv == 0.0).any() and len(coef) > 10
    model, rng_npz, rng_pkl = tmp_path / "m.model", tmp_path / "r.npz", tmp_path / "normalize.pickle"
    _write_model(model, sv, coef, rho, 0.05)
    lo, hi = -rng.uniform(0.5, 2.0, 36), rng.uniform(0.5, 2.0, 36)
    np.savez(rng_npz, min_=lo, max_=hi)
    with open(rng_pkl, "wb") as f:
        pickle.dump({"min_": list(lo), "max_": list(hi)}, f)
    for rp in (rng_npz, rng_pkl):
        prm = M.load_brisque_params(str(model), str(rp))
        assert prm.sv.shape == sv.shape and prm.sv.dtype == np.float64
        assert np.array_equal(prm.sv, sv) and np.array_equal(prm.coef, coef)     # repr round-trips fp64 exactly
        assert prm.rho == rho and prm.gamma == 0.05
        assert np.array_equal(prm.fmin, lo) and np.array_equal(prm.fmax, hi)
    # the reference SVR on the loaded parameters is libsvm's own prediction: z is taken as the input, so the ranges are (-1, 1)
    q = rng.uniform(-1, 1, (25, 36))
    one, neg = np.ones(36), -np.ones(36)
    got = np.array([R.svr(v, prm.sv, prm.coef, prm.rho, prm.gamma, neg, one) for v in q])
    want = svr.predict(q)
    err = np.abs(got - want).max()
    print(f"numpy SVR on the loaded model against sklearn's predict: max |diff| = {err:.3e}")
    assert err <= 1e-12
    assert isinstance(M._brisque_params((str(model), str(rng_npz))), M.BrisqueParams)


def test_loader_errors(tmp_path):
    from hvi_cidnet_amd import metrics as M
    rng = np.random.default_rng(0)
    sv, coef = rng.uniform(-1, 1, (5, 36)), rng.normal(size=5)
    rp = tmp_path / "r.npz"
    np.savez(rp, min_=-np.ones(36), max_=np.ones(36))
    p = tmp_path / "m.model"
    _write_model(p, sv, coef, 0.5, 0.05)
    M.load_brisque_params(str(p), str(rp))
    for kw in (dict(svm_type="c_svc"), dict(kernel_type="linear"), dict(drop=2), dict(total=7)):
        _write_model(p, sv, coef, 0.5, 0.05, **kw)
        with pytest.raises(ValueError, match="load_brisque_params"):
            M.load_brisque_params(str(p), str(rp))
    _write_model(p, sv, coef, 0.5, 0.05)
    text = open(p).read()
    for bad in (text.replace(" 36:", " 37:", 1), text.replace(" 1:", " 0:", 1), text.replace("SV\n", ""),
                text.replace("rho 0.5\n", ""), text.replace("gamma", "degree 3\ngamma"), text.replace(" 2:", " 2=", 1)):
        assert bad != text
        with open(p, "w") as f:
            f.write(bad)
        with pytest.raises(ValueError, match="load_brisque_params"):
            M.load_brisque_params(str(p), str(rp))
    _write_model(p, sv, coef, 0.5, 0.05)
    np.savez(rp, min_=-np.ones(36))
    with pytest.raises(ValueError, match="max_"):
        M.load_brisque_params(str(p), str(rp))
    np.savez(rp, min_=-np.ones(35), max_=np.ones(35))
    with pytest.raises(ValueError, match="36"):
        M.load_brisque_params(str(p), str(rp))
    with pytest.raises(ValueError, match="neither file is shipped"):
        M.load_brisque_params(None, None)
    with pytest.raises(ValueError):
        M.BrisqueParams(sv[:, :30], coef, 0.0, 0.05, -np.ones(36), np.ones(36))
    r = M.BrisqueParams.random(1)
    assert r.sv.shape == (64, 36) and np.array_equal(r.sv, M.BrisqueParams.random(1).sv) and (r.fmax > r.fmin).all()
    assert np.isnan(M.UnpairedResult(alpha=1.0, niqe=4.0).brisque)


def test_half_size_even_identity_and_odd_shapes():
    rng = np.random.default_rng(5)
    y = rng.random((18, 26))
    s = R.smooth(y)
    want = s.reshape(9, 2, 13, 2).mean(axis=(1, 3))
    err = np.abs(R.half(y) - want).max()
    print(f"even sizes: zoom against the 2 x 2 mean of the filtered image: {err:.3e}")
    assert err <= 1e-15
    assert R.half_shape(17, 23) == (8, 12) and R.half(rng.random((17, 23))).shape == (8, 12)
    assert R.half_shape(16, 16) == (8, 8) and R.half_shape(33, 31) == (16, 16) and R.half_shape(130, 70) == (65, 35)
    # the filter is the 5-tap mirror Gaussian of the header, columns then rows
    e = np.exp(-0.5 / 0.25 * np.arange(3) ** 2)
    k = e / (e[0] + 2 * e[1] + 2 * e[2])
    z = np.pad(y, 2, mode="reflect")
    v = k[0] * z[2:-2] + k[1] * (z[1:-3] + z[3:-1]) + k[2] * (z[:-4] + z[4:])
    hh = k[0] * v[:, 2:-2] + k[1] * (v[:, 1:-3] + v[:, 3:-1]) + k[2] * (v[:, :-4] + v[:, 4:])
    assert np.abs(hh - s).max() <= 1e-15


def test_root_against_scipy_root():
    """imquality solves phi(alpha) = R with scipy.optimize.root from 0.2; where that converges it finds the bracketed root"""
    from scipy import optimize
    hits = 0
    for alpha in (0.3, 0.5, 0.8, 1.0, 1.5, 2.0, 3.0, 5.0):
        big_r = R.phi(alpha)
        got = R.root(big_r)
        assert abs(got - alpha) <= 1e-9 * alpha, (alpha, got)
        sol = optimize.root(lambda a: R.phi(a) - big_r, [0.2])
        if sol.success and abs(R.phi(sol.x[0]) - big_r) <= 1e-12:
            hits += 1
            assert abs(sol.x[0] - got) <= 1e-6 * got, (alpha, sol.x[0], got)
    assert hits >= 3
    assert np.isnan(R.root(np.nan)) and np.isnan(R.root(0.75)) and np.isnan(R.root(R.phi(R.LO)))
    assert 0 < R.phi(R.LO) < 1e-4 and 0.74 < R.phi(R.HI) < 0.75


def test_moments_of_tiles_add_up_and_inputs_are_clear_of_flat_regions():
    """the tile ownership of the restatement covers every pair exactly once"""
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (3, 37, 70), dtype=np.uint8)
    m = R.mscn(R.gray(img))
    t = R.tile_moments(m)
    assert t.shape == (2 * 3, 5, 6)
    whole = R.moments(m)
    assert np.array_equal(t[:, :, (0, 2)].sum(axis=0), whole[:, (0, 2)])
    assert whole[:, (0, 2)].sum(axis=1).tolist() == [37 * 70, 37 * 69, 36 * 70, 36 * 69, 36 * 69]
    assert np.allclose(t.sum(axis=0), whole, rtol=1e-12, atol=0)
    assert R.min_margin(img) >= 1e-9
    f = R.features(img)
    assert f.shape == (36,) and np.isfinite(f).all()
    assert np.isnan(R.features(np.zeros((3, 16, 16), dtype=np.uint8))).all()


def test_plan_and_argument_checks_on_the_host():
    """cidnet_metric_brisque_plan and _ws_floats launch nothing; the staged entry points refuse bad arguments before a launch"""
    import ctypes
    from hvi_cidnet_amd import _lib, metrics as M
    L = _lib.lib()
    plan, ws = L.raw("cidnet_metric_brisque_plan"), L.raw("cidnet_metric_brisque_ws_floats")
    out = (ctypes.c_int * 10)(*([-7] * 10))
    assert plan(17, 23, out, 9) == 0
    assert list(out) == [32, 1, 1, 8, 12, 1, 1, 8 * (40 * 40 + 33 * 34 + 49 + 4 * 30), 2 * (2 * 30 + 3 * 17 * 23 + 8 * 12), -7]
    assert M.brisque_plan(130, 70) == dict(tile=32, tiles_y=5, tiles_x=3, h2=65, w2=35, tiles_y2=3, tiles_x2=2, lds=out[7],
                                           ws_floats=2 * ((15 + 6) * 30 + 3 * 130 * 70 + 65 * 35))
    assert ws(3, 130, 70) == 3 * M.brisque_plan(130, 70)["ws_floats"] and ws(1, 1728, 2304) == M.brisque_plan(1728, 2304)["ws_floats"]
    out = (ctypes.c_int * 10)(*([-7] * 10))
    assert plan(16, 16, out, 8) == -1 and plan(16, 16, None, 9) == -1 and plan(0, 16, out, 9) == -1
    assert plan(15, 16, out, 9) == -2 and plan(16, 15, out, 9) == -2 and plan(8192, 8193, out, 9) == -2
    assert list(out) == [-7] * 10                                 # nothing written on an error
    assert ws(1, 15, 16) == 0 and ws(0, 16, 16) == 0 and ws(65536, 16, 16) == 0
    buf = (ctypes.c_double * 64)()
    assert L.raw("cidnet_metric_brisque_gray")(None, buf, 1, 16, 16, None) == -1
    assert L.raw("cidnet_metric_brisque_gray")(buf, buf, 1, 15, 16, None) == -2
    assert L.raw("cidnet_metric_brisque_half")(buf, buf, None, 1, 16, 16, None) == -1
    assert L.raw("cidnet_metric_brisque_moments")(buf, 1, None, None, 1, 16, 16, None) == -1
    assert L.raw("cidnet_metric_brisque_moments")(buf, 1, None, buf, 1, 7, 16, None) == -2
    assert L.raw("cidnet_metric_brisque_fit")(buf, 1, buf, 17, 1, None) == -2
    assert L.raw("cidnet_metric_brisque_fit")(buf, 0, buf, 18, 1, None) == -1
    assert L.raw("cidnet_metric_brisque_svr")(buf, buf, buf, buf, buf, buf, 0, buf, 1, None) == -1
    assert L.raw("cidnet_metric_brisque_features")(buf, buf, buf, 10, 1, 16, 16, None) == -3
    assert L.raw("cidnet_metric_brisque_features")(buf, buf, buf, 1 << 20, 1, 15, 16, None) == -2
