"""CPU: the frequency-domain training loss's references against each other (tests/fft_loss_ref.py), the host-only plan query
of csrc/fft_loss.hip, the constructors of losses.FFTLoss / CIDNetLoss(fft_weight=), and the condition the fixtures of
tests/test_fft_loss_gpu.py section D must meet."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fft_loss_ref as FR  # noqa: E402

import hvi_cidnet_amd as P  # noqa: E402
from hvi_cidnet_amd import ops  # noqa: E402
from hvi_cidnet_amd._lib import lib  # noqa: E402

NFIELDS = 17


def _tile():
    out = (ctypes.c_long * NFIELDS)()
    assert lib().raw("cidnet_fft_loss_plan")(1, 1, 1, out, NFIELDS) == 0
    return tuple(out[:3])


SHAPES = FR.shapes(*_tile())


# ---- the references -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 8, 12, 63, 64, 65, 600])
def test_table64_is_the_reduced_angle_and_exact_at_the_quarter_turns(N):
    t = FR.table64(N, N)
    n, k = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    want = np.exp(-2j * np.pi * ((n * k) % N) / N)
    # either side's angle below 2 pi carries up to three roundings of half an ulp of 2 pi, 4.4e-16 each
    assert np.abs(t[..., 0] + 1j * t[..., 1] - want).max() <= 2e-15
    q = (4 * n * k) % N == 0
    assert set(np.unique(t[q])) <= {-1.0, 0.0, 1.0}
    assert np.array_equal(t[:, :N // 2 + 1], FR.table64(N, N // 2 + 1))
    assert np.array_equal(t[..., 0], t[..., 0].T) and np.array_equal(t[..., 1], t[..., 1].T)     # symmetric in (n, k)


@pytest.mark.parametrize("norm", FR.NORMS)
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 4), (3, 5, 7), (1, 16, 31), (5, 13, 20), (2, 32, 48)])
def test_reference_equals_the_closed_form(shape, norm):
    a, b = FR.noise(*shape, 3), FR.noise(*shape, 4)
    loss, ga, gb = FR.reference(a, b, FR.WEIGHT, norm, FR.G_UP)
    want_loss, want_g, D = FR.closed_form(a, b, FR.WEIGHT, norm, FR.G_UP)
    D64 = FR.spectrum64(a.double() - b.double())
    assert np.abs(D - D64.numpy()).max() <= 1e-12 * max(1.0, np.abs(D).max())
    assert abs(float(loss) - want_loss) <= 1e-13 * want_loss
    # a part that is exactly 0 by symmetry may come out as 1e-17 on either side, and sign() makes +-1 of it: each such part
    # may move a gradient element by 2 c
    tiny = int(((D64.abs() > 0) & (D64.abs() < 1e-9)).sum()) + int(((np.abs(D) > 0) & (np.abs(D) < 1e-9)).sum())
    c = abs(FR.G_UP * FR.scale_of(FR.WEIGHT, norm, *shape))
    assert np.abs(ga.numpy() - want_g).max() <= 1e-12 * np.abs(want_g).max() + 1e-18 + 2 * c * tiny
    assert torch.equal(gb, -ga)
    # the adjoint alone, on an arbitrary cotangent
    S = torch.randn((shape[0], shape[1], shape[2] // 2 + 1, 2), generator=torch.Generator().manual_seed(9)).double()
    x = torch.randn(shape, generator=torch.Generator().manual_seed(8)).double()
    lhs = float((FR.spectrum64(x) * S).sum())
    rhs = float((x * FR.adjoint64(S, shape[2])).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_against_the_reference(shape):
    """the worst case of an fp32 accumulator: every one of the K additions loses at most 2^-24 of the sum of magnitudes, and
    that sum is at most sum |x| in the row pass and 2 sum |x| in the column pass (|twiddle| <= 1, two terms per row)"""
    P_, H, W = shape
    x, D64, e32 = FR.spectrum_case(*shape)
    rms = float(D64.pow(2).mean().sqrt())
    print(f"spectrum {shape}: E32 {e32:.3e} ({e32 / rms:.2e} rms)")
    u = 2.0 ** -24
    assert e32 <= (W + 2 * H + 4) * u * 2 * float(x.abs().sum(dim=(1, 2)).max())
    for kind in ("normal", "signs"):
        S, g64, ea = FR.adjoint_case(*shape, kind)
        assert ea <= (2 * H + W + 6) * u * 2 * float(S.abs().sum(dim=(1, 2, 3)).max())
    if shape == (1, 1, 1):
        assert e32 == 0.0
    # the purely real bins: the restatement's imaginary part is exactly 0 there (the fp64 transform's is 0 or 1e-17, by host)
    D32 = FR.restate_spectrum(x.numpy())
    for ky in {0, H // 2 if H % 2 == 0 else 0}:
        for kx in {0, W // 2 if W % 2 == 0 else 0}:
            assert np.count_nonzero(D32[:, ky, kx, 1]) == 0 and float(D64[:, ky, kx, 1].abs().max()) <= 1e-12 * rms


@pytest.mark.parametrize("shape", SHAPES)
def test_fixtures_keep_clear_of_zero(shape):
    pc = FR.pair_case(*shape)
    parts = pc["D64"].numel()
    print(f"pair {shape}: seed {pc['seed']} E32 {pc['e32']:.3e} n_near {pc['n_near']} of {parts}")
    assert pc["n_near"] <= FR.near_limit(parts)
    assert parts >= 2000 or pc["n_near"] == 0
    assert float((pc["a"] - pc["b"]).abs().max()) > 0
    for norm in FR.NORMS:
        lc = FR.loss_case(*shape, norm)
        assert float(lc["loss"]) > 0 and lc["e32"] < 1e-3 * float(lc["ga"].abs().max())


# ---- the plan query -------------------------------------------------------------------------------------------------------
def _plan(P_, H, W, n=NFIELDS + 3):
    out = (ctypes.c_long * (NFIELDS + 3))(*([-7] * (NFIELDS + 3)))
    rc = lib().raw("cidnet_fft_loss_plan")(P_, H, W, out, n)
    return rc, list(out)


@pytest.mark.parametrize("shape", SHAPES + [(24, 256, 256), (1, 2048, 2048)])
def test_plan_fields(shape):
    P_, H, W = shape
    rc, f = _plan(*shape)
    assert rc == 0 and f[NFIELDS:] == [-7, -7, -7]            # nothing behind its own fields
    MT, NT, KC = f[:3]
    assert MT > 0 and NT > 0 and KC > 0 and MT % 32 == 0 and NT % 32 == 0
    N2 = 2 * (W // 2 + 1)
    up = lambda a, b: -(-a // b)  # noqa: E731
    assert f[3:6] == [up(P_ * H, MT), up(N2, NT), 1]          # row forward: planes share row tiles
    assert f[6:9] == [up(H, MT), up(N2, NT), P_]              # column forward: a plane to itself
    assert f[9:12] == f[6:9]
    assert f[12:15] == [up(P_ * H, MT), up(W, NT), 1]
    assert f[15] == f[6] * f[7] * f[8]                        # one fp64 partial per block of the column forward
    assert f[16] == 2 * f[15] + P_ * H * N2                   # the partials, and R or G behind them
    assert f[16] == lib().raw("cidnet_fft_loss_ws_floats")(P_, H, W)


def test_plan_refusals():
    ARG, SHAPE = -1, -2
    for args, code in [((0, 4, 4), ARG), ((1, 0, 4), ARG), ((1, 4, 0), ARG), ((1, -3, 4), ARG), ((1, 2049, 4), SHAPE),
                       ((1, 4, 2049), SHAPE), ((65536, 4, 4), SHAPE), ((600, 2048, 2048), SHAPE)]:
        rc, f = _plan(*args)
        assert rc == code and f == [-7] * (NFIELDS + 3), args
        assert lib().raw("cidnet_fft_loss_ws_floats")(*args) == 0
    rc, f = _plan(1, 4, 4, n=NFIELDS - 1)                     # a short output
    assert rc == ARG and f == [-7] * (NFIELDS + 3)
    assert lib().raw("cidnet_fft_loss_plan")(1, 4, 4, None, NFIELDS) == ARG
    assert lib().raw("cidnet_abi_version")() >= 29


def test_entry_points_refuse_before_touching_anything():
    """the argument checks come before any launch, so they can be exercised without a device: host memory stands in for
    the buffers and must stay untouched"""
    buf = (ctypes.c_float * 64)(*([7.0] * 64))
    p = ctypes.addressof(buf)
    vp, f = ctypes.c_void_p, ctypes.c_float
    L = lib().raw
    assert L("cidnet_dft_table")(0, 1, vp(p), None) == -1
    assert L("cidnet_dft_table")(4, 0, vp(p), None) == -1
    assert L("cidnet_dft_table")(4, 3, None, None) == -1
    assert L("cidnet_dft_table")(4, 3, vp(p + 2), None) == -1
    assert L("cidnet_dft_table")(2049, 3, vp(p), None) == -2
    assert L("cidnet_dft_table")(4, 5, vp(p), None) == -2
    ws = lib().raw("cidnet_fft_loss_ws_floats")(1, 2, 2)
    fwd = lambda **k: L("cidnet_fft_loss_fwd")(*[k.get(n, d) for n, d in (  # noqa: E731
        ("a", vp(p)), ("b", vp(p)), ("th", vp(p)), ("tw", vp(p)), ("weight", f(1.0)), ("norm", 0), ("loss", vp(p)), ("S", None),
        ("ws", vp(p)), ("n", ws), ("P", 1), ("H", 2), ("W", 2), ("st", None))])
    for bad, code in [(dict(a=None), -1), (dict(b=None), -1), (dict(th=None), -1), (dict(tw=None), -1), (dict(loss=None), -1),
                      (dict(ws=None), -1), (dict(ws=vp(p + 4)), -1), (dict(a=vp(p + 1)), -1), (dict(S=vp(p + 2)), -1),
                      (dict(norm=2), -1), (dict(norm=-1), -1), (dict(weight=f(-0.5)), -1), (dict(weight=f(float("nan"))), -1),
                      (dict(weight=f(float("inf"))), -1), (dict(n=ws - 1), -3), (dict(H=0), -1), (dict(W=2049), -2)]:
        assert fwd(**bad) == code, bad
    assert list(buf) == [7.0] * 64


# ---- the modules ----------------------------------------------------------------------------------------------------------
class _Model:
    @staticmethod
    def HVIT(x):
        return x


def test_constructors():
    assert P.CIDNetLoss(_Model()).fft is None
    assert P.CIDNetLoss(_Model(), fft_weight=0.0).fft is None
    crit = P.CIDNetLoss(_Model(), fft_weight=0.1, fft_norm="ortho")
    assert isinstance(crit.fft, P.FFTLoss) and crit.fft.loss_weight == 0.1 and crit.fft.norm == "ortho"
    assert P.CIDNetLoss(_Model(), fft_weight=0.1).fft.norm == "backward"
    assert P.FFTLoss().loss_weight == 1.0 and P.FFTLoss().norm == "backward"
    assert "FFTLoss" in P.__all__
    with pytest.raises(ValueError):
        P.CIDNetLoss(_Model(), fft_weight=-0.1)
    with pytest.raises(ValueError):
        P.CIDNetLoss(_Model(), fft_weight=0.1, fft_norm="forward")
    with pytest.raises(ValueError):
        P.FFTLoss(norm="forward")
    for w in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            P.FFTLoss(loss_weight=w)


def test_cpu_tensors_and_mismatched_shapes_are_refused():
    x = torch.rand(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="ROCm device"):
        P.FFTLoss()(x, x.clone())
    with pytest.raises(RuntimeError, match="same shape"):
        P.FFTLoss()(x, torch.rand(1, 3, 8, 9))
    with pytest.raises(RuntimeError, match="same shape"):
        P.FFTLoss()(x[0], x[0])
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.rfft2_parts(x)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.rfft2_parts_adjoint(torch.zeros(1, 8, 5, 2), 8)
    with pytest.raises(ValueError):
        ops.FFTLossFn.apply(x, x, 1.0, "forward")
