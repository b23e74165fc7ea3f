"""GPU: geometric self-ensemble -- the two kernels of csrc/ensemble.hip alone, then enhance_u8(ensemble=), inference.enhance and
evaluate(ensemble=) with the seeded, jittered full-width model.

Every comparison is exact.  ensemble_views is a permutation: it is compared as int32 bit patterns (NaN payloads and the sign
of zero included) with torch's flip(-1), flip(-2), transpose(-1, -2).contiguous().  ensemble_merge is a fixed-order fp32 sum:
the restatement below adds the inverse-mapped views one by one on the host (IEEE fp32 additions, then one division by an fp32
divisor held in a tensor, so that no reciprocal is multiplied instead); values are compared with torch.equal where neither
side is NaN, and the NaN positions must be the same.  The restatement is computed once per shape and shared.
The model cases run in a fresh spawned process each, as tests/test_enhance_gpu.py does."""
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from evaluate_harness import in_child as _in_child  # noqa: E402

pytestmark = pytest.mark.gpu
CIDNET_ERR_ARG, CIDNET_ERR_SHAPE = -1, -2
GUARD = 64
CANARY = -12345.5
SHAPES = [(1, 3, 8, 8), (2, 3, 16, 24), (1, 3, 40, 72), (3, 1, 5, 7), (1, 3, 1, 9), (1, 3, 9, 1), (1, 2, 33, 65), (1, 3, 64, 64),
          (2, 3, 96, 130)]
RANGES = [(0, 4), (4, 4), (0, 1), (1, 2), (5, 3), (7, 1)]
COUNTS = [(1, 0), (2, 0), (4, 0), (4, 4), (3, 2), (1, 1)]


def _view(x, k):
    """view k of (...,H,W), in the order include/cidnet_hip.h gives"""
    v = x
    if k & 1:
        v = v.flip(-1)
    if k & 2:
        v = v.flip(-2)
    if k & 4:
        v = v.transpose(-1, -2)
    return v.contiguous()


def _unview(v, k):
    """the inverse: the transpose undone first, then the flips"""
    if k & 4:
        v = v.transpose(-1, -2)
    if k & 2:
        v = v.flip(-2)
    if k & 1:
        v = v.flip(-1)
    return v.contiguous()


def _views(x, first, count):
    """(B,C,H,W) -> (B * count, C, Ho, Wo), image-major as ensemble_views lays them out"""
    return torch.stack([_view(x, first + v) for v in range(count)], dim=1).flatten(0, 1).contiguous()


def _merge(ya, yb, na, nb):
    """acc = v0; acc = acc + v_k, k ascending, A before B, in fp32; acc / n.  Host tensors."""
    B = ya.shape[0] // na
    a = ya.reshape(B, na, *ya.shape[1:])
    acc = a[:, 0].clone()
    for k in range(1, na):
        acc = acc + _unview(a[:, k], k)
    if nb:
        b = yb.reshape(B, nb, *yb.shape[1:])
        for s in range(nb):
            acc = acc + _unview(b[:, s], 4 + s)
    return acc / torch.full((), float(na + nb), dtype=torch.float32)


def _special(shape, seed):
    """random fp32 with +-0, NaN (two payloads) and +-inf planted; a host tensor"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    flat = x.reshape(-1)
    n = flat.numel()
    vals = torch.tensor([0.0, -0.0, float("nan"), float("inf"), float("-inf"), 1.0, -1.5], dtype=torch.float32)
    where = torch.randperm(n, generator=g)[:max(3, n // 6)]
    flat[where] = vals[torch.arange(len(where)) % len(vals)]
    flat.view(torch.int32)[where[2]] = 0x7FC12345                                   # a NaN with a payload
    return x


@functools.lru_cache(maxsize=None)
def _case(shape):
    """the inputs and the restated results of one shape, computed once on the host: x, its views per range, the merge inputs
    and the merged results per (na, nb)"""
    B, C, H, W = shape
    x = _special(shape, seed=H * 1000 + W)
    views = {r: _views(x, *r) for r in RANGES}
    ya = _special((B * 4, C, H, W), seed=H * 1000 + W + 1)
    yb = _special((B * 4, C, W, H), seed=H * 1000 + W + 2)
    merged = {}
    for na, nb in COUNTS:
        a = ya.reshape(B, 4, C, H, W)[:, :na].reshape(B * na, C, H, W).contiguous()
        b = yb.reshape(B, 4, C, W, H)[:, :nb].reshape(B * nb, C, W, H).contiguous() if nb else None
        merged[na, nb] = (a, b, _merge(a, b, na, nb))
    return x, views, merged


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same_values(got, want):
    """equal where neither is NaN (so -0 == +0 would pass: signs are checked by the bit comparison of the views and by
    signbit here), NaN in the same places"""
    nan = torch.isnan(want)
    return got.shape == want.shape and torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan], want[~nan]) and \
        torch.equal(torch.signbit(got[~nan]), torch.signbit(want[~nan]))


def _guarded(shape, dev):
    """an output buffer of `shape` with GUARD canary floats on both sides -> (whole buffer, the view to write)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.float32, device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _canary_ok(buf):
    return bool((buf[:GUARD] == CANARY).all()) and bool((buf[-GUARD:] == CANARY).all())


def _raw(name):
    from hvi_cidnet_amd import _lib
    return _lib.lib().raw(name)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@pytest.mark.parametrize("shape", SHAPES)
def test_views_are_torch_flips_and_transposes_bit_for_bit(dev, shape):
    import hvi_cidnet_amd as P
    x_host, views, _ = _case(shape)
    B, C, H, W = shape
    x = x_host.to(dev)
    before = x.clone()
    for first, count in RANGES:
        want = views[first, count].to(dev)
        got = P.image_io.ensemble_views(x, first, count)
        assert got.dtype == torch.float32 and got.is_contiguous()
        assert _same_bits(got, want), (shape, first, count)
        assert _same_bits(P.image_io.ensemble_views(x, first, count), got)                  # call to call
        buf, y = _guarded(tuple(want.shape), dev)                                           # nothing beside y is written
        rc = _raw("cidnet_ensemble_views")(_ptr(x), _ptr(y), B, C, H, W, first, count, None)
        torch.cuda.synchronize()
        assert rc == 0 and _same_bits(y, want) and _canary_ok(buf), (shape, first, count)
    assert _same_bits(x, before)                                                            # the source is only read


@pytest.mark.parametrize("shape", SHAPES)
def test_merge_is_the_sequential_fp32_sum_of_the_inverse_mapped_views(dev, shape):
    import hvi_cidnet_amd as P
    _, _, merged = _case(shape)
    B, C, H, W = shape
    for (na, nb), (a, b, want) in merged.items():
        ya, yb = a.to(dev), (b.to(dev) if nb else None)
        got = P.image_io.ensemble_merge(ya, yb, na=na)
        assert got.shape == (B, C, H, W) and got.dtype == torch.float32
        assert _same_values(got.cpu(), want), (shape, na, nb)
        assert _same_bits(P.image_io.ensemble_merge(ya, yb, na=na), got)                    # call to call
        buf, out = _guarded((B, C, H, W), dev)
        rc = _raw("cidnet_ensemble_merge")(_ptr(ya), na, _ptr(yb), nb, _ptr(out), B, C, H, W, None)
        torch.cuda.synchronize()
        assert rc == 0 and _same_bits(out, got) and _canary_ok(buf), (shape, na, nb)


@pytest.mark.parametrize("shape", SHAPES)
def test_round_trip_of_integer_valued_input_is_the_input(dev, shape):
    """merge(views(x, 0, 4), views(x, 4, 4)) = ((((x + x) + x) + ...) + x) / 8: exact for integer-valued x, so x itself"""
    import hvi_cidnet_amd as P
    g = torch.Generator().manual_seed(shape[2] * 100 + shape[3])
    x = torch.randint(-4096, 4097, shape, generator=g).float().to(dev)
    out = P.image_io.ensemble_merge(P.image_io.ensemble_views(x, 0, 4), P.image_io.ensemble_views(x, 4, 4))
    assert _same_bits(out, x), shape
    for na in (1, 2, 4):                                                                    # the flips alone
        assert _same_bits(P.image_io.ensemble_merge(P.image_io.ensemble_views(x, 0, na), None, na=na), x), (shape, na)


def test_argument_errors_leave_the_output_untouched(dev):
    """every CIDNET_ERR_SHAPE case of the header's block, and the NULL pointers (CIDNET_ERR_ARG)"""
    views, merge = _raw("cidnet_ensemble_views"), _raw("cidnet_ensemble_merge")
    B, C, H, W = 2, 3, 8, 16
    x = torch.rand((B, C, H, W), device=dev)
    buf, y = _guarded((B * 4, C, H, W), dev)
    ok = (B, C, H, W, 0, 4)
    assert views(_ptr(x), _ptr(y), *ok, None) == 0
    torch.cuda.synchronize()
    y.fill_(CANARY)
    bad = [(B, C, H, W, 0, 0), (B, C, H, W, 2, -1),                                         # count < 1
           (B, C, H, W, 2, 3), (B, C, H, W, 0, 5), (B, C, H, W, 3, 2), (B, C, H, W, 0, 8),   # crosses the group boundary
           (B, C, H, W, -1, 2), (B, C, H, W, 6, 3), (B, C, H, W, 8, 1), (B, C, H, W, 7, 2),  # leaves 0..7
           (16384, C, H, W, 0, 4), (65536, C, H, W, 5, 1), (21846, C, H, W, 4, 3),           # B * count > 65535
           (0, C, H, W, 0, 4), (B, 0, H, W, 0, 4), (B, C, 0, W, 0, 4), (B, C, H, 0, 0, 4), (B, C, -8, W, 4, 4),
           (B, 1 << 30, 65, 65, 0, 1)]                                                       # more than 2^31 - 1 tiles per image
    for args in bad:
        assert views(_ptr(x), _ptr(y), *args, None) == CIDNET_ERR_SHAPE, args
    assert views(None, _ptr(y), *ok, None) == CIDNET_ERR_ARG and views(_ptr(x), None, *ok, None) == CIDNET_ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())

    ya, yb = torch.rand((B * 4, C, H, W), device=dev), torch.rand((B * 4, C, W, H), device=dev)
    buf, out = _guarded((B, C, H, W), dev)
    assert merge(_ptr(ya), 4, _ptr(yb), 4, _ptr(out), B, C, H, W, None) == 0
    assert merge(_ptr(ya), 4, None, 0, _ptr(out), B, C, H, W, None) == 0
    torch.cuda.synchronize()
    out.fill_(CANARY)
    for na, b, nb, dims in [(0, yb, 4, (B, C, H, W)), (5, yb, 4, (B, C, H, W)), (-1, None, 0, (B, C, H, W)),      # na outside 1..4
                            (4, yb, 5, (B, C, H, W)), (4, yb, -1, (B, C, H, W)),                                  # nb outside 0..4
                            (4, None, 2, (B, C, H, W)), (4, yb, 0, (B, C, H, W)),                                 # yb NULL <=> nb == 0
                            (1, None, 0, (65536, C, H, W)),                                                       # B > 65535
                            (4, yb, 4, (0, C, H, W)), (4, yb, 4, (B, 0, H, W)), (4, yb, 4, (B, C, 0, W)), (4, None, 0, (B, C, H, -3)),
                            (4, None, 0, (B, 1 << 30, 65, 65))]:
        assert merge(_ptr(ya), na, _ptr(b), nb, _ptr(out), *dims, None) == CIDNET_ERR_SHAPE, (na, nb, dims)
    assert merge(None, 4, _ptr(yb), 4, _ptr(out), B, C, H, W, None) == CIDNET_ERR_ARG
    assert merge(_ptr(ya), 4, _ptr(yb), 4, None, B, C, H, W, None) == CIDNET_ERR_ARG
    torch.cuda.synchronize()
    assert bool((buf == CANARY).all())


def test_wrappers_check_their_arguments(dev):
    import hvi_cidnet_amd as P
    IO = P.image_io
    x = torch.rand((2, 3, 8, 16), device=dev)
    for first, count in ((0, 0), (2, 3), (0, 5), (-1, 2), (6, 3), (8, 1)):
        with pytest.raises(ValueError, match="0..3 or inside 4..7"):
            IO.ensemble_views(x, first, count)
    with pytest.raises(RuntimeError, match="fp32"):
        IO.ensemble_views(x.double(), 0, 4)
    with pytest.raises(RuntimeError, match=r"\(B,C,H,W\)"):
        IO.ensemble_views(x[0], 0, 4)
    ya = IO.ensemble_views(x, 0, 4)
    with pytest.raises(ValueError, match="na = 3"):
        IO.ensemble_merge(ya, None, na=3)                                                   # 8 is no multiple of 3
    with pytest.raises(ValueError, match="transposed views"):
        IO.ensemble_merge(ya, ya, na=4)                                                     # yb of the wrong shape
    # a strided input is made dense first
    wide = torch.rand((2, 3, 8, 32), device=dev)
    assert _same_bits(IO.ensemble_views(wide[..., ::2], 4, 4), _views(wide[..., ::2].contiguous(), 4, 4))


# ---- end to end: the seeded, jittered full-width model ---------------------------------------------------------------------
def _full_model(cls_name="CIDNet", seed=5):
    import hvi_cidnet_amd as P
    from oracle import cidnet_oracle as O
    m = getattr(P, cls_name)()
    p = O.make_params(seed, variant={"CIDNet": "base", "CIDNet_TNSM": "tnsm"}[cls_name])
    m.load_state_dict({k: p[k] for k in m.state_dict().keys()})
    return m.to("cuda:0")


def _images(shape, seed=21):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).cuda()


def _manual(m, imgs, ensemble, gamma=1.0, **attrs):
    """torch-built views, as batches in the same order, through the same model; the torch sum; egress"""
    import hvi_cidnet_amd as P
    na, nb = {2: (2, 0), 4: (4, 0), 8: (4, 4)}[ensemble]
    t = m.trans
    old = (m.training, t.gated, t.alpha_s, t.gated2, t.alpha)
    m.eval()
    t.gated, t.alpha_s, t.gated2, t.alpha = (attrs.get("gated", False), attrs.get("alpha_s", 1.3), attrs.get("gated2", False),
                                             attrs.get("alpha", 1.0))
    with torch.no_grad():
        x, hw = P.ingest(imgs, gamma=gamma)
        first = lambda y: y[0] if isinstance(y, tuple) else y  # noqa: E731
        ya = first(m(_views(x, 0, na)))
        yb = first(m(_views(x, 4, nb))) if nb else None
        out = _merge(ya.cpu(), yb.cpu() if nb else None, na, nb).cuda()
        q = P.egress(out, hw)
    m.train(old[0])
    t.gated, t.alpha_s, t.gated2, t.alpha = old[1:]
    return q


@pytest.mark.parametrize("cls_name,shape", [("CIDNet", (2, 13, 22, 3)), ("CIDNet_TNSM", (2, 13, 22, 3)), ("CIDNet", (1, 16, 16, 3))])
def test_enhance_u8_ensemble_equals_the_manual_chain(dev, cls_name, shape):
    _in_child(_case_enhance_u8, cls_name, shape)


def _case_enhance_u8(cls_name, shape):
    import hvi_cidnet_amd as P
    m = _full_model(cls_name)
    imgs = _images(shape)
    plain = P.enhance_u8(m, imgs)
    assert torch.equal(P.enhance_u8(m, imgs, ensemble=1), plain)                            # the default path, byte for byte
    got = {}
    for e in ((2, 4, 8) if cls_name == "CIDNet" and shape[0] == 2 else (8,)):
        got[e] = P.enhance_u8(m, imgs, ensemble=e)
        assert got[e].shape == imgs.shape and got[e].dtype == torch.uint8
        want = _manual(m, imgs, e)
        diff = (got[e].int() - want.int()).abs()
        print(f"{cls_name} {shape} ensemble={e}: bytes that differ from the manual chain: {int((diff > 0).sum())}, "
              f"from ensemble=1: {int((got[e] != plain).sum())} of {plain.numel()}")
        assert torch.equal(got[e], want), (cls_name, shape, e)
    assert not torch.equal(got[8], plain)                                                   # a stub cannot pass
    if cls_name == "CIDNet" and shape[0] == 2:                                              # the other arguments travel along
        cfg = dict(gamma=0.8, gated=True, alpha_s=1.1, gated2=True, alpha=0.9)
        attrs = {k: v for k, v in cfg.items() if k != "gamma"}
        assert torch.equal(P.enhance_u8(m, imgs, ensemble=4, **cfg), _manual(m, imgs, 4, gamma=0.8, **attrs))
        with pytest.raises(ValueError, match="tile"):
            P.enhance_u8(m, imgs, ensemble=8, tile=16)
        # inference.enhance, the fp32 side: the merged output clamped and cropped
        x = imgs.permute(0, 3, 1, 2).float().div(255)
        xp, (h, w) = P.pad_to_multiple(x, 8)
        m.eval()
        with torch.no_grad():
            m.trans.alpha_s, m.trans.alpha = 1.0, 1.0
            ya, yb = m(_views(xp, 0, 4)), m(_views(xp, 4, 4))
        want = torch.clamp(_merge(ya.cpu(), yb.cpu(), 4, 4), 0, 1)[:, :, :h, :w].cuda()
        assert torch.equal(P.enhance(m, x, ensemble=8), want)
        assert torch.equal(P.enhance(m, x, ensemble=1), P.enhance(m, x))


def test_enhance_folder_ensemble(dev, tmp_path):
    _in_child(_case_folder, str(tmp_path))


def _case_folder(tmp):
    import numpy as np
    from PIL import Image
    import hvi_cidnet_amd as P
    m = _full_model()
    imgs = _images((2, 13, 22, 3), seed=4)
    src, dst = os.path.join(tmp, "in"), os.path.join(tmp, "out")
    os.makedirs(src)
    for i, a in enumerate(imgs.cpu().numpy()):
        Image.fromarray(a).save(os.path.join(src, f"{i}.png"))
    rep = P.enhance_folder(m, src, dst, batch_size=2, ensemble=8)
    assert rep.ensemble == 8 and rep.batches == [[0, 1]]
    want = P.enhance_u8(m, imgs, ensemble=8).cpu().numpy()
    for i in range(2):
        assert np.array_equal(np.array(Image.open(os.path.join(dst, f"{i}.png"))), want[i])
    assert P.enhance_folder(m, src, os.path.join(tmp, "out1")).ensemble == 1


def test_evaluate_ensemble_scores_what_enhance_u8_writes(dev):
    _in_child(_case_evaluate)


def _case_evaluate():
    """two tiny pairs (13 x 22: SSIM needs 11 x 11), a single alpha and a sweep of two: PSNR / SSIM are those of
    psnr_ssim(enhance_u8(..., ensemble=8), gt), to the last bit"""
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import metrics as M
    m = _full_model()
    lows = _images((2, 13, 22, 3), seed=7)
    gts = _images((2, 13, 22, 3), seed=8)
    pairs = [(lows[i].cpu().numpy(), gts[i].cpu().numpy()) for i in range(2)]
    g = gts.permute(0, 3, 1, 2).contiguous()

    def scores(alpha, gated, batch_size=2, gated2=False):
        """of enhance_u8 on batches of batch_size images, as evaluate forms them"""
        out = {k: [] for k in ("psnr", "ssim", "psnr_gt_mean", "ssim_gt_mean")}
        for lo in range(0, 2, batch_size):
            q = P.enhance_u8(m, lows[lo:lo + batch_size], alpha=alpha, gated=gated, gated2=gated2, ensemble=8).permute(0, 3, 1, 2).contiguous()
            for suffix, gt_mean in (("", False), ("_gt_mean", True)):
                p, s = M.psnr_ssim(q, g[lo:lo + batch_size], gt_mean=gt_mean)
                out["psnr" + suffix] += p.tolist()
                out["ssim" + suffix] += s.tolist()
        return out

    for batch_size in (1, 2):
        res = P.evaluate(m, pairs, alpha=0.9, gated=True, batch_size=batch_size, ensemble=8)
        assert res.ensemble == 8 and res.per_image == scores(0.9, True, batch_size), (batch_size, res.per_image)
    sweep = P.evaluate(m, pairs, alpha=[0.8, 1.0], gated2=True, batch_size=2, ensemble=8)     # alpha acts under gated2 only
    assert [r.alpha for r in sweep] == [0.8, 1.0]
    for r in sweep:
        assert r.ensemble == 8 and r.per_image == scores(r.alpha, False, gated2=True), r.alpha
    assert sweep[0].per_image != sweep[1].per_image
    plain = P.evaluate(m, pairs, alpha=0.9, gated=True)
    assert plain.ensemble == 1 and plain.per_image != res.per_image
    assert P.evaluate(m, pairs, alpha=0.9, gated=True, ensemble=1).per_image == plain.per_image
    with pytest.raises(ValueError, match="ensemble"):
        P.evaluate(m, pairs, ensemble=3)


def test_evaluate_unpaired_ensemble(dev):
    _in_child(_case_unpaired)


def _case_unpaired():
    """the NIQE parameters of tests/golden suffice: one 100 x 200 image (pads to 104 x 200; two 96 x 96 blocks, the fewest NIQE
    scores -- one block alone is NaN by definition), a scene with structure and grain as tests/test_evaluate_unpaired_gpu.py
    builds them: the score is exactly NIQE of enhance_u8(..., gated2=True, ensemble=4)"""
    import numpy as np
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import metrics as M
    params = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "niqe_pris_params.npz")
    m = _full_model()
    h, w = 100, 200
    yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    base = np.stack([0.35 + 0.25 * np.sin(9 * xx + c) * np.cos(7 * yy - c) for c in range(3)], axis=-1)
    scene = np.clip(base + np.random.default_rng(3).normal(0, 0.06, (h, w, 3)), 0.02, 0.9)
    u8 = np.ascontiguousarray((scene * 255).astype(np.uint8))
    res = P.evaluate_unpaired(m, [u8], params, alpha=0.9, ensemble=4)
    q = P.enhance_u8(m, torch.from_numpy(u8).cuda(), gated2=True, alpha=0.9, ensemble=4).permute(0, 3, 1, 2).contiguous()
    want = M.niqe(q, params).tolist()
    print("niqe with ensemble=4:", res.per_image["niqe"], "of enhance_u8's bytes:", want)
    assert res.ensemble == 4 and np.isfinite(want).all() and res.per_image["niqe"] == want
    assert P.evaluate_unpaired(m, [u8], params, alpha=0.9).ensemble == 1
