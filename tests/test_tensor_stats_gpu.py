"""GPU: the per-tensor statistics kernel (csrc/tensor_stats.hip: cidnet_tensor_stats) against torch fp64 on the smallest
shapes where it can go wrong -- every segment length around the 4-element load, the wave, the block pass and the tile, every
16-byte phase of a head and a tail, NaN everywhere outside the segments -- and dp.TensorLog in the trainer (eager, hipGraph,
accumulated) and in fit(diagnose=, preview_dir=).  The planted NaN / Inf values are arithmetic in healthy kernels, not faults.

maxabs, nonfinite and first must be exactly equal; the norm within (2 len + 8) 2^-53 relative, the worst-case bound of any
summation order on either side (tensor_stats_ref.check), so nothing was measured to set it.
A negative (or NaN, or infinite) scale is REFUSED: CIDNET_ERR_ARG, nothing is launched."""
import collections
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch

from oracle import cidnet_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tensor_stats_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL = (12, 12, 24, 48)
SHAPE = (1, 3, 16, 24)
SCALE = 1.0 / 3.0                                        # not a power of two: the fp32 value, widened, is what multiplies


def _on(dev, buf):
    """the numpy view of the fixture on the device, at the same offset from an allocation's start"""
    full = buf.base
    shift = (buf.__array_interface__["data"][0] - full.__array_interface__["data"][0]) // 4
    t = torch.from_numpy(full).to(dev)
    assert t.data_ptr() % 16 == 0
    return t[shift:shift + buf.size]


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


# ---- the kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gaps", [False, True])
def test_kernel_matches_torch_fp64_at_every_phase(dev, gaps):
    from hvi_cidnet_amd import ops
    from hvi_cidnet_amd.dp import tensor_stats_plan
    for shift in range(4):
        buf, off, lens = R.fixture(gaps, shift, planted=True)
        t = _on(dev, buf)
        assert t.data_ptr() % 16 == 4 * shift
        plan = tensor_stats_plan(off, lens, t.numel(), dev)
        assert plan.kernel and plan.seg_tiles == [-(-c // 4096) for c in lens]
        got = ops.tensor_stats(t, plan, SCALE)
        assert got.dtype == torch.float64 and got.shape == (len(lens), 4) and got.device == t.device
        want = R.stats_torch(torch.from_numpy(buf), off, lens, SCALE)
        R.check(got.cpu().numpy(), want, lens)
        # what plant_all() planted, spelled out
        g = got.cpu().numpy()
        assert g[0].tolist() == [0.0, 0.0, 1.0, 0.0]
        assert g[2, 1] == float(np.float32(1e-45)) * float(np.float32(SCALE)) and g[2, 1] > 0 and g[2, 0] > 0
        assert g[3].tolist() == [0.0, 0.0, 0.0, -1.0] and g[7].tolist() == [0.0, 0.0, 0.0, -1.0]
        assert g[9].tolist() == [0.0, 0.0, 255.0, 0.0]
        assert g[10, 1] == 100.0 * float(np.float32(SCALE))
        assert g[11, 1] == float(np.float32(3e38)) * float(np.float32(SCALE)) and np.isfinite(g[11, 0]) and g[11, 0] >= g[11, 1]
        assert g[R.I4097, 2:].tolist() == [2.0, 4095.0] and g[R.I8193, 2:].tolist() == [1.0, 8192.0]
        assert g[19, 2:].tolist() == [2.0, 4095.0]


def test_kernel_planted_positions(dev):
    """NaN, +Inf and -Inf at index 0, len - 1, 4095 and 4096 of the 4097- and the 8193-element segment, one at a time"""
    from hvi_cidnet_amd import ops
    from hvi_cidnet_amd.dp import tensor_stats_plan
    base, off, lens = R.fixture(True, 1)
    t = _on(dev, base)
    plan = tensor_stats_plan(off, lens, t.numel(), dev)
    clean = ops.tensor_stats(t, plan, 1.0).cpu().numpy()
    R.check(clean, R.stats_torch(torch.from_numpy(base), off, lens, 1.0), lens)
    assert (clean[:, 2] == 0).all() and (clean[:, 3] == -1).all()
    for name, i, values in R.planted_cases():
        (pos, v), = values.items()
        at = off[i] + pos
        t[at] = float(v)
        got = ops.tensor_stats(t, plan, 1.0).cpu().numpy()
        buf = base.copy()
        buf[at] = v
        R.check(got, R.stats_torch(torch.from_numpy(buf), off, lens, 1.0), lens)
        assert got[i, 2] == 1 and got[i, 3] == pos, name
        others = [k for k in range(len(lens)) if k != i]
        assert got[others].tobytes() == clean[others].tobytes(), name
        t[at] = float(base[at])


def test_kernel_is_deterministic_and_a_row_depends_on_its_segment_alone(dev):
    from hvi_cidnet_amd import _lib, ops
    from hvi_cidnet_amd.dp import tensor_stats_plan
    buf, off, lens = R.fixture(True, 3, planted=True)
    t = _on(dev, buf)
    plan = tensor_stats_plan(off, lens, t.numel(), dev)
    a = ops.tensor_stats(t, plan, SCALE)
    b = ops.tensor_stats(t, plan, SCALE, out=torch.full((len(lens), 4), -1.0, dtype=torch.float64, device=dev))
    assert _bits(a) == _bits(b)
    for i in range(len(lens)):
        alone = ops.tensor_stats(t, tensor_stats_plan([off[i]], [lens[i]], t.numel(), dev), SCALE)
        assert _bits(alone[0]) == _bits(a[i]), i
    # the segments in another order, and one of them twice
    order = list(range(len(lens)))[::-1] + [R.I4097]
    c = ops.tensor_stats(t, tensor_stats_plan([off[i] for i in order], [lens[i] for i in order], t.numel(), dev), SCALE)
    assert _bits(c) == _bits(a[order])
    # the launcher's tile count is the plan query's: it takes exactly the plan's workspace, writes every slot of it (a
    # slot's count is never negative) and nothing behind them
    f = _lib.lib().raw("cidnet_tensor_stats")
    ws = torch.full((4 * plan.tiles + 64,), -1, dtype=torch.int64, device=dev)
    out = torch.empty((len(lens), 4), dtype=torch.float64, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(ws_bytes, scale=SCALE, n=plan.n, buf_ptr=t.data_ptr()):
        return f(ctypes.c_void_p(buf_ptr), n, plan._off, plan._len, plan.T, ctypes.c_void_p(plan.off_dev.data_ptr()),
                 ctypes.c_void_p(plan.len_dev.data_ptr()), ctypes.c_void_p(plan.table_dev.data_ptr()), ctypes.c_float(scale),
                 ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws_bytes, stream)

    assert plan.ws_bytes == 32 * plan.tiles == 32 * sum(plan.seg_tiles)
    out.fill_(-5.0)
    assert call(plan.ws_bytes - 1) == -3                                     # CIDNET_ERR_WS
    for bad in (-1.0, -0.0 - 1e-30, float("nan"), float("inf")):
        assert call(plan.ws_bytes, scale=bad) == -1                          # refused, not |s|
    assert call(plan.ws_bytes, n=off[-1] + lens[-1] - 1) == -1               # the last segment past n
    assert call(plan.ws_bytes, buf_ptr=None) == -1
    torch.cuda.synchronize()
    assert (out == -5.0).all() and (ws == -1).all()                          # nothing was launched
    assert call(plan.ws_bytes) == 0
    torch.cuda.synchronize()
    slots = ws[:4 * plan.tiles].view(-1, 4)
    assert (slots[:, 2] >= 0).all() and (ws[4 * plan.tiles:] == -1).all()
    assert _bits(out) == _bits(a)
    with pytest.raises(RuntimeError, match="CIDNET_ERR_ARG"):
        ops.tensor_stats(t, plan, -1.0)
    with pytest.raises(RuntimeError):
        ops.tensor_stats(t[:-1], plan, 1.0)


# ---- the trainer ---------------------------------------------------------------------------------------------------------
def _model(dev, chans=SMALL, seed=21):
    import hvi_cidnet_amd as P
    m = P.CIDNet(channels=list(chans))
    p = O.make_params(seed, channels=chans)
    m.load_state_dict({k: p[k] for k in m.state_dict().keys()})
    return m.to(dev)


def _batches(dev, n, shape=SHAPE, seed=31):
    return [(O.synthetic_batch(seed + i, shape).to(dev), O.synthetic_batch(seed + 100 + i, shape).to(dev)) for i in range(n)]


def _spy_on_updates(tr, plant=None):
    """record (gradient, weights, scale) as they are immediately before every update, through the one method all three modes
    apply an update with; plant(update index, gradient buffer) may write into the gradient first"""
    seen, orig = [], tr._opt_step

    def spy(loss, flat_g=None, passes=1):
        g = tr.flat_g if flat_g is None else flat_g
        if plant is not None:
            plant(len(seen), g)
        seen.append((g[:tr.n_live].clone(), tr.flat_p[:tr.n_live].clone(), 1.0 / passes))
        return orig(loss, flat_g=flat_g, passes=passes)
    tr._opt_step = spy
    return seen


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("accum", [1, 2])
def test_trainer_rows_are_the_restatement_of_the_arena(dev, use_graph, accum):
    from hvi_cidnet_amd import ops
    from hvi_cidnet_amd.dp import DataParallelTrainer, StepLog, TensorLog
    log, tlog = StepLog(8), TensorLog(8)
    tr = DataParallelTrainer(_model(dev), lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True, step_log=log, tensor_log=tlog,
                             use_graph=use_graph, accum_steps=accum)
    target = {}

    def plant(u, g):
        if u == 1:                                       # an Inf in one parameter's gradient, second update
            names = [r[0] for r in tr._live_named()]
            t = len(names) // 2
            _, o, c, _ = tr._live_named()[t]
            target.update(t=t, name=names[t], elem=c // 2)
            g[o + c // 2] = float("inf")

    seen = _spy_on_updates(tr, plant)
    bs = _batches(dev, 3 * accum - (1 if accum > 1 else 0))
    for x, gt in bs:
        tr.step(x, gt)
    if accum > 1:
        assert tr.pending_passes == 1
        tr.flush()                                       # the third update: one pass, scale 1
    torch.cuda.synchronize()
    rows, stats = log.read(), tlog.read()
    named = tr._live_named()
    off, lens = [r[1] for r in named], [r[2] for r in named]
    assert len(seen) == 3 and stats.shape == (3, 2, len(named), 4) and rows.shape == (3, 4) and len(named) > 100
    assert tlog.names == tuple(r[0] for r in named)
    assert [s[2] for s in seen] == ([1.0] * 3 if accum == 1 else [0.5, 0.5, 1.0])
    for u, (g, p, scale) in enumerate(seen):
        R.check(stats[u, 0], ops.tensor_stats_torch(g.cpu(), off, lens, scale).numpy(), lens)
        R.check(stats[u, 1], ops.tensor_stats_torch(p.cpu(), off, lens, 1.0).numpy(), lens)
        if u != 1:
            total = float(np.sqrt((stats[u, 0, :, 0] ** 2).sum()))
            assert abs(total - rows[u, 1]) <= (2 * tr.n_live + 8) * 2.0 ** -53 * rows[u, 1]
    assert rows[:, 3].tolist() == [1, -2, 2]             # the planted update was skipped
    assert tlog.first_nonfinite(stats[1]) == (target["t"], target["name"], target["elem"])
    assert stats[1, 0, :, 2].sum() == 1 and tlog.first_nonfinite(stats[0]) is None and tlog.first_nonfinite(stats[2]) is None
    assert all(tlog.first_nonfinite(stats[u], "weight") is None for u in range(3))


def _launches(fn):
    """names of the cidnet:: kernels fn() launches, in the order in which they started on the device"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    evs = [(ev.time_range.start, ev.name) for ev in prof.events() if ev.device_type == DeviceType.CUDA and "cidnet::" in ev.name]
    return [n for _, n in sorted(evs)]


def _is_stats(name):
    return "stats_tile_kernel" in name or "stats_finish_kernel" in name


@pytest.mark.parametrize("guarded", [True, False])
def test_without_a_tensor_log_the_launch_list_is_unchanged(dev, guarded):
    """the step without the log launches no statistics kernel, and the step with it launches exactly that list plus four
    launches per update, which sit immediately before the guard (unguarded: before Adam)"""
    from hvi_cidnet_amd.dp import DataParallelTrainer, StepLog, TensorLog
    x, gt = _batches(dev, 1)[0]
    res = {}
    for with_log in (False, True):
        kw = dict(max_grad_norm=1.0, skip_nonfinite=True, step_log=StepLog(8)) if guarded else {}
        tr = DataParallelTrainer(_model(dev), lr=1e-3, tensor_log=TensorLog(8) if with_log else None, **kw)
        for _ in range(2):
            tr.step(x, gt)
        res[with_log] = _launches(lambda: tr.step(x, gt))
    plain, logged = res[False], res[True]
    assert plain and not any(_is_stats(n) for n in plain)
    assert collections.Counter(n for n in logged if not _is_stats(n)) == collections.Counter(plain)
    first = next(i for i, n in enumerate(logged) if _is_stats(n))
    tail = logged[first:]
    kinds = ["tile" if "stats_tile_kernel" in n else "finish" if "stats_finish_kernel" in n else n for n in tail]
    assert kinds[:4] == ["tile", "finish", "tile", "finish"] and not any(_is_stats(n) for n in tail[4:])
    assert ("sumsq_kernel" if guarded else "adam_kernel") in tail[4]
    assert tail[4:] == plain[len(plain) - len(tail) + 4:]


# ---- fit -----------------------------------------------------------------------------------------------------------------
class _Batches:
    """two fixed batches per epoch; poison = (epoch, batch): `factor`, which the loss is multiplied with, is NaN for that one"""

    def __init__(self, dev, factor, poison):
        self.b = {e: _batches(dev, 2, (2, 3, 16, 24), seed=200 + 10 * e) for e in (1, 2)}
        self.factor, self.poison = factor, poison

    def __len__(self):
        return 2

    def epoch(self, e):
        for i, b in enumerate(self.b[e]):
            self.factor.fill_(float("nan") if (e, i) == self.poison else 1.0)
            yield b


def test_fit_diagnoses_and_writes_the_preview_on_the_device(dev, tmp_path):
    from PIL import Image
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import ops
    factor = torch.ones((), device=dev)

    def loss_fn(out, gt):
        return ops.L1LossFn.apply(out, gt) * factor

    model = _model(dev)
    batches = _Batches(dev, factor, (2, 0))
    recs = P.fit(model, batches, nEpochs=2, lr=1e-3, start_warmup=False, loss_fn=loss_fn, max_grad_norm=1.0, diagnose=True,
                 preview_dir=str(tmp_path))
    d1, d2 = recs[0]["diagnosis"], recs[1]["diagnosis"]
    assert [r["skipped"] for r in recs] == [0, 1]
    assert d1["nonfinite"] == [] and d1["weights_nonfinite"] == [] and d2["weights_nonfinite"] == []
    (hit,) = d2["nonfinite"]
    assert hit["update"] == 0 and hit["applied"] is False and hit["tensors"]
    assert hit["origin"]["name"] == hit["tensors"][0] and hit["origin"]["element"] >= 0
    for d in (d1, d2):
        norms = [e["norm"] for e in d["grad_top"]]
        assert len(norms) == 5 and norms == sorted(norms, reverse=True) and np.isfinite(norms).all() and norms[-1] > 0
    assert all(e["update"] == 1 for e in d2["grad_top"])                     # the one applied update of epoch 2
    # the preview: first sample of epoch 2's last batch, through the trained weights, in train mode
    x, gt = batches.b[2][-1]
    assert model.training
    with torch.no_grad():
        out = model(x[:1])
    q = P.egress(out)[0].cpu().numpy()
    for name, want in (("test.png", q), ("gt.png", P.egress(gt[:1])[0].cpu().numpy())):
        path = tmp_path / name
        assert np.array_equal(np.asarray(Image.open(path)), want) and want.shape == (16, 24, 3), name
        enc = io.BytesIO()
        Image.fromarray(want).save(enc, format="PNG")
        assert path.read_bytes() == enc.getvalue(), name
    assert np.array_equal(P.egress(gt[:1])[0].cpu().numpy(),
                          (gt[0].clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy())
