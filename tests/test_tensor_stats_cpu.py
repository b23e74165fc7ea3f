"""CPU: the per-tensor statistics (csrc/tensor_stats.hip) as far as they go without a device -- the host-only plan query of
the library (cidnet_tensor_stats_plan), the plain-torch restatement (ops.tensor_stats_torch) against straightforward numpy
fp64 on the fixture the GPU test uses, dp.TensorLog, the trainer's integration on the toy model of tests/test_fit_cpu.py
(use_hip_kernels=False) and fit(diagnose=, preview_dir=)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tensor_stats_ref as R  # noqa: E402

CPU = dict(use_hip_kernels=False)
TILE = 4096


# ---- the plan query ------------------------------------------------------------------------------------------------------
def _plan(off, length, n, T=None, n_out=3, table_ints=None, with_seg=True, with_table=True, pad=8):
    """cidnet_tensor_stats_plan -> (status, out, seg_tiles, table); every array is prefilled with -7 and longer than it is
    said to be, so that a write that should not happen shows"""
    from hvi_cidnet_amd import _lib
    T = len(off) if T is None else T
    tiles = sum(-(-max(c, 1) // TILE) for c in length)
    want = len(off) + 2 * tiles
    table_ints = want if table_ints is None else table_ints
    o = (ctypes.c_long * max(len(off), 1))(*off)
    c = (ctypes.c_long * max(len(length), 1))(*length)
    out = (ctypes.c_long * (3 + pad))(*([-7] * (3 + pad)))
    seg = (ctypes.c_int * (len(off) + pad))(*([-7] * (len(off) + pad)))
    nt = (max(table_ints, want) if with_table else 0) + pad
    table = (ctypes.c_int * nt)(*([-7] * nt))
    rc = _lib.lib().raw("cidnet_tensor_stats_plan")(o, c, T, n, out, n_out, seg if with_seg else None,
                                                    table if with_table else None, table_ints)
    return rc, list(out), list(seg), list(table)


def test_plan_tile_counts_table_and_workspace():
    lens = [1, 4095, 4096, 4097, 3 * 4096 + 1]
    off = list(np.cumsum([0] + lens[:-1]))
    n = sum(lens)
    rc, out, seg, table = _plan(off, lens, n)
    assert rc == 0
    want = [1, 1, 1, 2, 4]
    tiles = sum(want)
    assert seg[:5] == want and seg[5:] == [-7] * 8
    assert out[:3] == [tiles, 32 * tiles, 5 + 2 * tiles] and out[3:] == [-7] * 8
    # first tile of every segment, then every (segment, tile) exactly once, in order
    assert table[:5] == [0, 1, 2, 3, 5]
    pairs = [(table[5 + 2 * j], table[5 + 2 * j + 1]) for j in range(tiles)]
    assert pairs == [(t, k) for t in range(5) for k in range(want[t])]
    assert table[5 + 2 * tiles:] == [-7] * 8
    # sizes only: no table, no segment counts
    rc, out2, seg2, table2 = _plan(off, lens, n, with_seg=False, with_table=False)
    assert rc == 0 and out2[:3] == out[:3] and set(seg2) == {-7} and set(table2) == {-7}
    # the workspace grows with the tile count
    sizes = [_plan([0], [c], c)[1][1] for c in (1, 4096, 4097, 3 * 4096 + 1)]
    assert sizes == [32, 32, 64, 128]
    # segments need not be adjacent, ordered or aligned
    rc, out, seg, _ = _plan([9001, 3, 1], [4097, 5, 1], 20000)
    assert rc == 0 and seg[:3] == [2, 1, 1] and out[0] == 4


@pytest.mark.parametrize("case", ["len0", "len_neg", "off_neg", "past_n", "off_past_n", "T0", "n0", "short_table", "n_out",
                                  "null_out", "null_off", "null_len"])
def test_plan_argument_errors_write_nothing(case):
    from hvi_cidnet_amd import _lib
    off, lens, n, kw = [0, 10], [10, 5000], 5010, {}
    if case == "len0":
        lens = [10, 0]
    elif case == "len_neg":
        lens = [-1, 5000]
    elif case == "off_neg":
        off = [-1, 10]
    elif case == "past_n":
        n = 5009
    elif case == "off_past_n":
        off = [0, 6000]
    elif case == "T0":
        kw["T"] = 0
    elif case == "n0":
        n = 0
    elif case == "short_table":
        kw["table_ints"] = 2 + 2 * 3 - 1
    elif case == "n_out":
        kw["n_out"] = 2
    if case.startswith("null"):
        o, c, out = (ctypes.c_long * 2)(0, 10), (ctypes.c_long * 2)(10, 5000), (ctypes.c_long * 3)(-7, -7, -7)
        args = {"null_out": (o, c, 2, n, None, 3), "null_off": (None, c, 2, n, out, 3), "null_len": (o, None, 2, n, out, 3)}[case]
        assert _lib.lib().raw("cidnet_tensor_stats_plan")(*args, None, None, 0) == -1
        assert list(out) == [-7, -7, -7]
        return
    rc, out, seg, table = _plan(off, lens, n, **kw)
    assert rc == -1
    assert set(out) == {-7} and set(seg) == {-7} and set(table) == {-7}


def test_plan_rejects_what_the_index_types_cannot_hold():
    """more than 2^30 tiles (one segment of 2^42 + 1 elements: nothing that long is touched, the query is arithmetic), or
    more than 2^30 segments (checked before the arrays are read)"""
    rc, out, seg, table = _plan([0], [(1 << 42) + 1], 1 << 43, with_table=False)
    assert rc == -2 and set(out) == {-7} and set(seg) == {-7}
    rc, out, _, _ = _plan([0], [(1 << 42)], 1 << 43, with_table=False, with_seg=False)
    assert rc == 0 and out[0] == 1 << 30
    rc, out, seg, _ = _plan([0], [1], 1, T=(1 << 30) + 1, with_table=False)
    assert rc == -2 and set(out) == {-7} and set(seg) == {-7}


def test_python_plan_agrees_with_the_library():
    from hvi_cidnet_amd import ops
    from hvi_cidnet_amd.dp import tensor_stats_plan
    p = tensor_stats_plan([0, 1, 37], [1, 36, 9000], 9037, "cpu")
    assert not p.kernel and p.seg_tiles == [1, 1, 3] and p.tiles == 5
    rc, out, seg, _ = _plan([0, 1, 37], [1, 36, 9000], 9037)
    assert rc == 0 and seg[:3] == p.seg_tiles and out[0] == p.tiles
    with pytest.raises(RuntimeError):
        tensor_stats_plan([0, 5], [5, 5], 9, "cpu")
    with pytest.raises(RuntimeError):
        tensor_stats_plan([0], [1], 1, "cpu", kernel=True)
    with pytest.raises(RuntimeError, match="scale"):
        ops.tensor_stats(torch.zeros(9037), p, scale=-1.0)


# ---- the restatement against numpy ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_restatement_matches_numpy_fp64(gaps, shift):
    from hvi_cidnet_amd import ops
    from hvi_cidnet_amd.dp import tensor_stats_plan
    buf, off, lens = R.fixture(gaps, shift, planted=True)
    scale = 0.25
    want = R.stats_numpy(buf, off, lens, scale)
    t = torch.from_numpy(buf)
    got = ops.tensor_stats(t, tensor_stats_plan(off, lens, t.numel(), "cpu"), scale).numpy()
    R.check(got, want, lens)
    out = torch.full((len(off), 4), -3.0, dtype=torch.float64)
    assert ops.tensor_stats(t, tensor_stats_plan(off, lens, t.numel(), "cpu", kernel=False), scale, out=out) is out
    assert out.numpy().tobytes() == got.tobytes()


def test_restatement_on_the_planted_positions():
    from hvi_cidnet_amd import ops
    from hvi_cidnet_amd.dp import tensor_stats_plan
    base, off, lens = R.fixture(True, 1)
    plan = tensor_stats_plan(off, lens, base.size, "cpu")
    for name, i, values in R.planted_cases():
        buf = base.copy()
        for pos, v in values.items():
            buf[off[i] + pos] = v
        got = ops.tensor_stats(torch.from_numpy(buf), plan, 1.0).numpy()
        R.check(got, R.stats_numpy(buf, off, lens, 1.0), lens)
        assert got[i, 2] == 1 and got[i, 3] == next(iter(values)), name


# ---- TensorLog -----------------------------------------------------------------------------------------------------------
def test_tensor_log_wraps_and_reads_in_step_order():
    from hvi_cidnet_amd.dp import TensorLog
    log = TensorLog(3).bind("cpu", ["a", "b"])
    assert log.what == ("grad", "weight") and log.names == ("a", "b")
    for i in range(5):
        log.next_row().copy_(torch.full((2, 2, 4), float(i), dtype=torch.float64))
    rows = log.read()
    assert rows.shape == (3, 2, 2, 4) and rows[:, 0, 0, 0].tolist() == [2.0, 3.0, 4.0]
    log.reset()
    assert log.read().shape == (0, 2, 2, 4)
    row = np.zeros((2, 2, 4))
    assert log.first_nonfinite(row) is None
    row[0, 1, 2:] = 3, 17
    row[1, 0, 2:] = 1, 5
    assert log.first_nonfinite(row) == (1, "b", 17) and log.first_nonfinite(row, "weight") == (0, "a", 5)
    one = TensorLog(2, what=("weight",)).bind("cpu", ["a"])
    assert one.next_row().shape == (1, 1, 4)
    for bad in ((), ("grad", "grad"), ("moment",)):
        with pytest.raises(ValueError):
            TensorLog(2, what=bad)
    with pytest.raises(ValueError):
        TensorLog(0)


# ---- the trainer on the CPU ----------------------------------------------------------------------------------------------
class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Conv2d(3, 8, 3, padding=1)
        self.b = nn.Conv2d(8, 3, 1)
        self.dead = nn.Linear(4, 4)                      # never used: no gradient, not in the log

    def forward(self, x):
        return self.b(torch.tanh(self.a(x)))


def l1(out, gt):
    return (out - gt).abs().mean()


class ListBatches:
    def __init__(self, steps=3, seed=5, shape=(2, 3, 8, 8)):
        self.steps, self.seed, self.shape = steps, seed, shape

    def __len__(self):
        return self.steps

    def epoch(self, e):
        g = torch.Generator().manual_seed(1000 * self.seed + e)
        for _ in range(self.steps):
            yield torch.rand(self.shape, generator=g), torch.rand(self.shape, generator=g)


def _trainer(accum=1, tensor_log=True, cap=8, hook=None, **kw):
    from hvi_cidnet_amd.dp import DataParallelTrainer, StepLog, TensorLog
    torch.manual_seed(0)
    model = Net()
    log, tlog = StepLog(cap), (TensorLog(cap) if tensor_log else None)
    grads = []                                           # per pass: {name: the gradient autograd produced}
    names = {id(p): n for n, p in model.named_parameters()}

    def spy(p):
        if hook is not None:
            hook(names[id(p)], p.grad, len(grads) - 1)
        grads[-1][names[id(p)]] = p.grad.detach().clone()
    for p in model.parameters():
        p.register_post_accumulate_grad_hook(spy)        # registered before the trainer's hook, so it sees p.grad
    tr = DataParallelTrainer(model, lr=1e-2, loss_fn=l1, max_grad_norm=1.0, skip_nonfinite=True, step_log=log,
                             accum_steps=accum, **({"tensor_log": tlog} if tensor_log else {}), **kw, **CPU)
    return tr, log, tlog, grads


def _run(tr, grads, batches):
    weights = []
    for i, (x, gt) in enumerate(batches):
        if tr._ready and tr.pending_passes == 0:
            weights.append({n: tr.flat_p[o:o + c].clone() for n, o, c, _ in tr._live_named()})
        elif not tr._ready:
            weights.append({n: p.detach().reshape(-1).clone() for n, p in tr.model.named_parameters()})
        grads.append({})                                 # the first step's probing backward writes the same entry first
        tr.step(x, gt)
    return weights


def test_trainer_rows_against_the_gradients_and_the_step_log():
    tr, log, tlog, grads = _trainer()
    b = list(ListBatches(steps=3).epoch(0))
    weights = _run(tr, grads, b)
    rows, stats = log.read(), tlog.read()
    names = tlog.names
    assert names == tuple(r[0] for r in tr._live_named()) and set(names) == {"a.weight", "a.bias", "b.weight", "b.bias"}
    assert stats.shape == (3, 2, 4, 4) and rows.shape == (3, 4)
    n = tr.n_live
    for u in range(3):
        g = stats[u, 0]
        total = float(np.sqrt((g[:, 0] ** 2).sum()))
        assert abs(total - rows[u, 1]) <= (2 * n + 8) * 2.0 ** -53 * rows[u, 1], (u, total, rows[u, 1])
        for t, name in enumerate(names):
            assert g[t, 1] == float(grads[u][name].abs().max()) * 1.0
            assert g[t, 2] == 0 and g[t, 3] == -1
            w = weights[u][name].double()
            assert stats[u, 1, t, 1] == float(w.abs().max()) and stats[u, 1, t, 2] == 0
            assert abs(stats[u, 1, t, 0] - float(w.pow(2).sum().sqrt())) <= (2 * w.numel() + 8) * 2.0 ** -53 * stats[u, 1, t, 0]


def test_trainer_accumulated_update_logs_one_row_with_the_guards_scale():
    tr, log, tlog, grads = _trainer(accum=2)
    b = list(ListBatches(steps=4).epoch(0))
    _run(tr, grads, b)
    rows, stats = log.read(), tlog.read()
    assert rows.shape == (2, 4) and stats.shape == (2, 2, 4, 4) and len(grads) == 4
    for u in range(2):
        for t, name in enumerate(tlog.names):
            summed = grads[2 * u][name] + grads[2 * u + 1][name]                  # fp32, pass order
            assert stats[u, 0, t, 1] == float(summed.abs().max()) * 0.5           # 1 / (world * 2)
        total = float(np.sqrt((stats[u, 0, :, 0] ** 2).sum()))
        assert abs(total - rows[u, 1]) <= (2 * tr.n_live + 8) * 2.0 ** -53 * rows[u, 1]
    # a group the epoch leaves open: flush() logs its row with 1 / (world * 1)
    grads.append({})
    tr.step(*b[0])
    assert tlog.issued == 2
    tr.flush()
    assert tlog.issued == 3 == log.issued
    last = tlog.read()[2]
    for t, name in enumerate(tlog.names):
        assert last[0, t, 1] == float(grads[4][name].abs().max())


def test_trainer_localises_a_planted_nan_and_leaves_the_other_rows_alone():
    target, elem = "a.weight", 101

    def plant(name, grad, _pass):
        if name == target and plant.on:
            grad.view(-1)[elem] = float("nan")
    plant.on = False
    b = list(ListBatches(steps=2).epoch(0))
    clean_tr, clean_log, clean_tlog, g0 = _trainer()
    _run(clean_tr, g0, b)
    tr, log, tlog, g1 = _trainer(hook=plant)
    _run(tr, g1, b[:1])
    before = tr.flat_p.clone()
    plant.on = True
    g1.append({})
    tr.step(*b[1])
    plant.on = False
    rows, stats, clean = log.read(), tlog.read(), clean_tlog.read()
    assert rows[1, 3] == -2 and torch.equal(before, tr.flat_p)               # skipped
    t = tlog.names.index(target)
    assert stats[1, 0, t, 2] == 1 and stats[1, 0, t, 3] == elem
    assert tlog.first_nonfinite(stats[1]) == (t, target, elem) and tlog.first_nonfinite(stats[0]) is None
    assert tlog.first_nonfinite(stats[1], "weight") is None
    # the finite elements of the poisoned tensor still count; every other tensor's row is the clean run's, bit for bit
    assert np.isfinite(stats[1, 0, t, :2]).all() and stats[1, 0, t, 0] > 0
    others = [i for i in range(len(tlog.names)) if i != t]
    assert stats[1, 0, others].tobytes() == clean[1, 0, others].tobytes()
    assert stats[1, 1].tobytes() == clean[1, 1].tobytes() and stats[0].tobytes() == clean[0].tobytes()


def test_without_a_tensor_log_nothing_changes():
    """the trainer without the argument against the trainer with the log: same state_dict keys, same weights, moments and step
    log bit for bit (the log only reads), and no plan or ring exists without it"""
    b = list(ListBatches(steps=3).epoch(0))
    plain, log0, _, g0 = _trainer(tensor_log=False)
    _run(plain, g0, b)
    with_log, log1, _, g1 = _trainer()
    _run(with_log, g1, b)
    assert plain.tensor_log is None and plain._stats_plan is None
    s0, s1 = plain.state_dict(), with_log.state_dict()
    assert sorted(s0) == sorted(s1) == sorted(["exp_avg", "exp_avg_sq", "steps_applied", "steps_skipped", "lr", "betas", "eps",
                                               "weight_decay"])
    assert torch.equal(plain.flat_p, with_log.flat_p) and torch.equal(plain.opt.m, with_log.opt.m)
    assert torch.equal(plain.opt.v, with_log.opt.v) and log0.read().tobytes() == log1.read().tobytes()


# ---- fit(diagnose=, preview_dir=) ----------------------------------------------------------------------------------------
class PoisonAt:
    """l1 whose value is NaN at the given (0-based) calls: the whole gradient of that update is NaN"""

    def __init__(self, calls):
        self.calls, self.n = set(calls), -1

    def __call__(self, out, gt):
        self.n += 1
        return l1(out, gt) * (float("nan") if self.n in self.calls else 1.0)


def test_fit_diagnose_and_preview(tmp_path):
    from PIL import Image
    from hvi_cidnet_amd import fit
    torch.manual_seed(0)
    model = Net()
    batches = ListBatches(steps=3, shape=(2, 3, 8, 12))
    # call 0 is the probing backward, calls 1..3 epoch 1, 4..6 epoch 2: poison the second update of epoch 2
    recs = fit(model, batches, nEpochs=2, lr=1e-2, start_warmup=False, loss_fn=PoisonAt([5]), max_grad_norm=1.0,
               trainer_args=CPU, diagnose=True, diagnose_top=3, preview_dir=str(tmp_path / "pv"))
    assert [sorted(r["diagnosis"]) for r in recs] == [["grad_top", "nonfinite", "weights_nonfinite"]] * 2
    d1, d2 = recs[0]["diagnosis"], recs[1]["diagnosis"]
    assert d1["nonfinite"] == [] and d1["weights_nonfinite"] == [] and d2["weights_nonfinite"] == []
    assert recs[1]["skipped"] == 1 and len(d2["nonfinite"]) == 1
    hit = d2["nonfinite"][0]
    # every gradient is NaN from its first element on; the origin is the first tensor in arena order: the last layer's
    assert hit["update"] == 1 and hit["applied"] is False and len(hit["tensors"]) == 4
    assert hit["origin"]["tensor"] == 0 and hit["origin"]["name"] == hit["tensors"][0] and hit["origin"]["element"] == 0
    assert hit["origin"]["name"].startswith("b.")
    for d in (d1, d2):
        top = d["grad_top"]
        assert len(top) == 3 and [e["norm"] for e in top] == sorted((e["norm"] for e in top), reverse=True)
        assert all(np.isfinite(e["norm"]) and 0 <= e["update"] < 3 and e["name"] in hit["tensors"] for e in top)
    assert all(e["update"] != 1 for e in d2["grad_top"])                     # applied updates only
    # the preview: the epoch's last batch, first sample
    x, gt = list(batches.epoch(2))[-1]
    got = np.asarray(Image.open(tmp_path / "pv" / "gt.png"))
    assert got.shape == (8, 12, 3)
    assert np.array_equal(got, (gt[0].clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).numpy())
    test = np.asarray(Image.open(tmp_path / "pv" / "test.png"))
    with torch.no_grad():
        want = (model(x[:1])[0].clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).numpy()
    assert test.shape == (8, 12, 3) and np.array_equal(test, want)
    assert sorted(os.listdir(tmp_path / "pv")) == ["gt.png", "test.png"]


def test_fit_defaults_keep_the_record_keys_and_values(tmp_path):
    from hvi_cidnet_amd import fit
    kw = dict(nEpochs=2, lr=1e-2, start_warmup=False, loss_fn=l1, max_grad_norm=1.0, trainer_args=CPU)
    torch.manual_seed(0)
    plain = fit(Net(), ListBatches(), **kw)
    assert [sorted(r) for r in plain] == [["clipped", "epoch", "grad_norm_max", "loss", "lr", "skipped", "steps"]] * 2
    torch.manual_seed(0)
    diag = fit(Net(), ListBatches(), diagnose=True, preview_dir=str(tmp_path), **kw)
    assert [{k: v for k, v in r.items() if k != "diagnosis"} for r in diag] == plain


def test_run_epoch_hands_the_last_batch_back_only_when_asked():
    from hvi_cidnet_amd import run_epoch
    tr, log, _, grads = _trainer(tensor_log=False)

    class Spy(ListBatches):
        def epoch(self, e):
            for b in super().epoch(e):
                grads.append({})
                yield b
    rows = run_epoch(tr, Spy(steps=2), 1, log)
    assert rows.shape == (2, 4)
    last = ["stale"]
    rows = run_epoch(tr, Spy(steps=2), 2, log, last_batch=last)
    want = list(ListBatches(steps=2).epoch(2))[-1]
    assert rows.shape == (2, 4) and len(last) == 1 and all(torch.equal(a, b) for a, b in zip(last[0], want))
