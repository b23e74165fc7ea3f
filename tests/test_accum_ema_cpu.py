"""CPU: gradient accumulation and the EMA of the weights in dp.DataParallelTrainer / fit.fit, on the plain-torch restatement
(use_hip_kernels=False) and a small network with a multi-use parameter and a dead layer.  Everything here is pinned bit for
bit: an accumulated update against three forward_backward passes added by hand, the average against its numpy fp32
restatement, ema_weights() against a model loaded from ema_state_dict(), resume against the uninterrupted run; two gloo ranks
against one process to the tolerance of tests/test_dp_gloo.py."""
import copy
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

CPU = dict(use_hip_kernels=False)


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Conv2d(3, 8, 3, padding=1)
        self.norm_w = nn.Parameter(torch.ones(8))       # used twice per step (multi-use parameter)
        self.b = nn.Conv2d(8, 3, 1)
        self.dead = nn.Linear(4, 4)                      # never used: no gradient, no optimizer state (like I_LCA5)

    def forward(self, x):
        h = torch.tanh(self.a(x)) * self.norm_w[None, :, None, None]
        return self.b(h * self.norm_w[None, :, None, None])


def _net(seed=0):
    torch.manual_seed(seed)
    return Net()


def l1(out, gt):
    return (out - gt).abs().mean()


def _batches(n, seed=5, shape=(2, 3, 8, 8)):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(shape, generator=g), torch.rand(shape, generator=g)) for _ in range(n)]


class ListBatches:
    """epoch(e) is a function of (seed, e), as data.TrainBatches' plan is"""

    def __init__(self, steps=3, seed=5):
        self.steps, self.seed = steps, seed

    def __len__(self):
        return self.steps

    def epoch(self, e):
        return iter(_batches(self.steps, seed=1000 * self.seed + e))


def _trainer(model, **kw):
    from hvi_cidnet_amd.dp import DataParallelTrainer
    return DataParallelTrainer(model, lr=1e-2, n_buckets=3, loss_fn=l1, **CPU, **kw)


def _ema_numpy(e, p, decay):
    """e + w (p - e) in fp32, three roundings, w = fp32(1 - decay) formed in double"""
    w = np.float32(1.0 - decay)
    return (e + (w * (p - e).astype(np.float32)).astype(np.float32)).astype(np.float32)


def test_accumulated_update_equals_three_passes_added_by_hand():
    from hvi_cidnet_amd.dp import StepLog
    K = 3
    bs = _batches(2 * K)
    guard = dict(max_grad_norm=0.05, skip_nonfinite=True)
    log, log2 = StepLog(4), StepLog(4)
    tr = _trainer(_net(), accum_steps=K, step_log=log, **guard)
    hand = _trainer(_net(), step_log=log2, **guard)
    for u in range(2):
        group = bs[u * K:(u + 1) * K]
        for j, (x, gt) in enumerate(group):
            assert tr.pending_passes == j
            before = [p.detach().clone() for p in tr.model.parameters()]
            loss = tr.step(x, gt)
            assert not loss.requires_grad
            if j < K - 1:                                         # no update before the K-th pass
                assert all(torch.equal(a, b) for a, b in zip(before, tr.model.parameters()))
        assert tr.pending_passes == 0
        total, loss_sum = None, None
        for x, gt in group:
            ls = hand.forward_backward(x, gt).to(torch.float32)
            g = hand.flat_g.clone()
            total = g if total is None else total + g            # fp32, pass order
            loss_sum = ls if loss_sum is None else loss_sum + ls
        n = hand.n_live
        row = log2.next_row()
        hand.opt.step(total, n, grad_scale=1.0 / K, loss=loss_sum * np.float32(1.0 / K), log_row=row)
        assert torch.equal(tr.flat_p, hand.flat_p)
        assert torch.equal(tr.opt.m, hand.opt.m) and torch.equal(tr.opt.v, hand.opt.v)
    rows, rows2 = log.read(), log2.read()
    assert rows.shape == (2, 4) and rows.tobytes() == rows2.tobytes()           # one row per update
    assert rows[:, 3].tolist() == [1, 2] and (rows[:, 2] < 1.0).all()
    assert tr.opt.steps_applied() == 2


def test_defaults_change_nothing():
    bs = _batches(5)
    a = _trainer(_net(3))
    b = _trainer(_net(3), accum_steps=1, ema_decay=None)
    for x, gt in bs:
        la, lb = a.step(x, gt), b.step(x, gt)
        assert torch.equal(la, lb)
    assert torch.equal(a.flat_p, b.flat_p) and torch.equal(a.opt.m, b.opt.m) and torch.equal(a.opt.v, b.opt.v)
    keys = {"exp_avg", "exp_avg_sq", "steps_applied", "steps_skipped", "lr", "betas", "eps", "weight_decay"}
    assert set(a.state_dict()) == set(b.state_dict()) == keys
    assert b.pending_passes == 0 and not hasattr(b.opt, "ema") and not hasattr(b.opt, "acc")
    b.flush()                                                    # no open group: nothing happens
    assert torch.equal(a.flat_p, b.flat_p)
    with pytest.raises(RuntimeError, match="ema_decay"):
        b.ema_state_dict()
    for bad in (dict(accum_steps=0), dict(ema_decay=1.0), dict(ema_decay=-0.1)):
        with pytest.raises(ValueError):
            _trainer(_net(), **bad)


def test_ema_follows_applied_steps_only():
    from hvi_cidnet_amd.dp import StepLog
    decay = 0.9
    scale = {"v": 1.0}
    model = _net(1)
    from hvi_cidnet_amd.dp import DataParallelTrainer
    tr = DataParallelTrainer(model, lr=1e-2, n_buckets=3, loss_fn=lambda o, g: l1(o, g) * scale["v"], max_grad_norm=0.05,
                             skip_nonfinite=True, step_log=StepLog(8), ema_decay=decay, **CPU)
    init = {k: v.clone() for k, v in model.state_dict().items()}
    want = None
    for i, (x, gt) in enumerate(_batches(6)):
        scale["v"] = float("nan") if i == 3 else 1.0
        before = tr.ema.clone() if i else None
        tr.step(x, gt)
        n = tr.n_live
        if want is None:                                          # the average starts as a copy of the initial weights
            flat0 = torch.cat([init[name].reshape(-1) for name, *_ in tr._live_named()])
            want = flat0.numpy().copy()
            assert torch.equal(tr.ema[n:], tr.flat_p[n:]) and tr.ema.numel() == tr.flat_p.numel() > n
        if i == 3:
            assert torch.equal(tr.ema, before)                    # bit-unchanged across the skipped step
        else:
            want = _ema_numpy(want, tr.flat_p[:n].numpy(), decay)
        assert tr.ema[:n].numpy().tobytes() == want.tobytes(), i
    assert (tr.opt.steps_applied(), tr.opt.steps_skipped()) == (5, 1)
    assert torch.equal(tr.ema[n:], tr.flat_p[n:])                 # the dead tail stays the copy
    assert not torch.equal(tr.ema[:n], tr.flat_p[:n])
    # the unguarded path: every step is applied
    tr2 = _trainer(_net(1), ema_decay=decay)
    want = None
    for x, gt in _batches(3):
        tr2.step(x, gt)
        n = tr2.n_live
        if want is None:
            tr0 = _trainer(_net(1))
            tr0.forward_backward(x, gt)
            want = tr0.flat_p[:n].numpy().copy()
        want = _ema_numpy(want, tr2.flat_p[:n].numpy(), decay)
        assert tr2.ema[:n].numpy().tobytes() == want.tobytes()


def test_ema_weights_context_and_state_dict():
    bs = _batches(5)
    model = _net(2)
    tr = _trainer(model, accum_steps=2, ema_decay=0.5)
    with pytest.raises(RuntimeError):
        tr.ema_state_dict()                                       # before the first step
    for x, gt in bs[:4]:
        tr.step(x, gt)
    sd = tr.ema_state_dict()
    assert list(sd) == list(model.state_dict()) and all(v.device.type == "cpu" for v in sd.values())
    fresh = _net(9)
    fresh.load_state_dict(sd, strict=True)
    assert torch.equal(sd["dead.weight"], model.state_dict()["dead.weight"])
    assert not torch.equal(sd["a.weight"], model.state_dict()["a.weight"])
    p0, e0 = tr.flat_p.clone(), tr.ema.clone()
    x = bs[4][0]
    with torch.no_grad():
        plain = model(x)
        with tr.ema_weights():
            inside = model(x)
            assert torch.equal(inside, fresh(x)) and not torch.equal(inside, plain)
            with pytest.raises(RuntimeError, match="ema_weights"):
                tr.step(*bs[4])
            with pytest.raises(RuntimeError):
                tr.state_dict()
        assert torch.equal(model(x), plain)
    assert torch.equal(tr.flat_p, p0) and torch.equal(tr.ema, e0)

    class Boom(Exception):
        pass

    with pytest.raises(Boom):
        with tr.ema_weights():
            raise Boom
    assert torch.equal(tr.flat_p, p0) and torch.equal(tr.ema, e0)
    # an open group: no context, no state
    tr.step(*bs[4])
    assert tr.pending_passes == 1
    with pytest.raises(RuntimeError, match="open"):
        with tr.ema_weights():
            pass
    with pytest.raises(RuntimeError, match="open"):
        tr.state_dict()
    assert torch.equal(tr.flat_p, p0) and torch.equal(tr.ema, e0)
    tr.flush()                                                    # one pass, 1 / (world * 1): a plain step from that batch
    assert tr.pending_passes == 0 and not torch.equal(tr.flat_p, p0)
    twin = _trainer(_net(2), accum_steps=2, ema_decay=0.5)
    for x, gt in bs[:4]:
        twin.step(x, gt)
    twin.forward_backward(*bs[4])
    twin.opt.step(twin.flat_g, twin.n_live, grad_scale=1.0)
    assert torch.equal(tr.flat_p, twin.flat_p) and torch.equal(tr.ema, twin.ema)
    # state: strict about the average in both directions
    st = tr.state_dict()
    assert set(st["ema"]) == set(st["exp_avg"]) and st["ema_decay"] == 0.5 and "dead.weight" not in st["ema"]
    with pytest.raises(KeyError):
        _trainer(_net(2)).load_state_dict(st)
    with pytest.raises(KeyError):
        tr.load_state_dict({k: v for k, v in st.items() if k != "ema"})
    other = _trainer(_net(2), accum_steps=2, ema_decay=0.5)
    other.model.load_state_dict(model.state_dict())
    other.load_state_dict(st)
    for x, gt in bs[:2]:
        tr.step(x, gt)
        other.step(x, gt)
    assert torch.equal(tr.flat_p, other.flat_p) and torch.equal(tr.ema, other.ema)


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def test_fit_accumulates_averages_and_resumes_exactly(tmp_path, monkeypatch):
    """three batches per epoch with K = 2: two updates per epoch, the second by flush() from one pass"""
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import metrics

    def evaluate(model, pairs, **kw):                              # a CPU stand-in with evaluate's result fields
        with torch.no_grad():
            mse = [float(((model(x) - gt) ** 2).mean()) for x, gt in pairs]
        return types.SimpleNamespace(psnr=float(np.mean([-10 * np.log10(m) for m in mse])), ssim=float(np.mean(mse)))

    monkeypatch.setattr(metrics, "evaluate", evaluate)
    val = _batches(2, seed=77, shape=(1, 3, 8, 8))
    at = 2
    kw = dict(nEpochs=4, lr=1e-2, warmup_epochs=1, snapshots=2, loss_fn=l1, max_grad_norm=0.05, trainer_args=CPU,
              accum_steps=2, ema_decay=0.999, val_weights="both", val_pairs=val)
    for bad in (dict(val_weights="ema", ema_decay=None), dict(val_weights="both", ema_decay=None), dict(val_weights="x")):
        with pytest.raises(ValueError):
            P.fit(_net(2), ListBatches(), **{**kw, **bad})
    full = P.fit(_net(2), ListBatches(), out_dir=str(tmp_path / "a"), **kw)
    assert all(r["steps"] == 2 and r["skipped"] == 0 for r in full)
    assert all(("psnr_ema" in r) == ("psnr" in r) == (r["epoch"] % 2 == 0) for r in full)
    assert all(r["psnr"] != r["psnr_ema"] and r["ssim"] != r["ssim_ema"] for r in full if "psnr" in r)
    first = []

    class Stop(Exception):
        pass

    def stop_there(rec):
        first.append(rec)
        if rec["epoch"] == at:
            raise Stop

    with pytest.raises(Stop):
        P.fit(_net(2), ListBatches(), out_dir=str(tmp_path / "b"), on_epoch=stop_there, **kw)
    rest = P.fit(_net(7), ListBatches(), out_dir=str(tmp_path / "b"), resume=str(tmp_path / "b" / f"epoch_{at}.train.pt"), **kw)
    assert first + rest == full
    for name in ("epoch_4.pth", "epoch_4.ema.pth"):
        wa, wb = _load(tmp_path / "a" / name), _load(tmp_path / "b" / name)
        assert wa.keys() == wb.keys() and all(torch.equal(wa[k], wb[k]) for k in wa), name
    sa, sb = _load(tmp_path / "a" / "epoch_4.train.pt")["trainer"], _load(tmp_path / "b" / "epoch_4.train.pt")["trainer"]
    for k in ("exp_avg", "exp_avg_sq", "ema"):
        assert sa[k].keys() == sb[k].keys() and all(torch.equal(sa[k][n], sb[k][n]) for n in sa[k]), k
    assert sa["steps_applied"] == sb["steps_applied"] == 8 and sa["ema_decay"] == sb["ema_decay"] == 0.999
    fresh = _net(11)
    fresh.load_state_dict(_load(tmp_path / "a" / "epoch_4.ema.pth"), strict=True)
    model_w = _load(tmp_path / "a" / "epoch_4.pth")
    assert not torch.equal(fresh.a.weight, model_w["a.weight"]) and torch.equal(fresh.dead.weight, model_w["dead.weight"])
    # the validation of the average is the validation of the file's weights
    assert full[-1]["psnr_ema"] == evaluate(fresh, val).psnr
    # a run without the average refuses this file, and the other way round
    with pytest.raises(KeyError):
        P.fit(_net(7), ListBatches(), resume=str(tmp_path / "b" / f"epoch_{at}.train.pt"),
              **{**kw, "ema_decay": None, "val_weights": "model"})


# ---- two gloo ranks ---------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


UPDATES, K2 = 2, 2


def _micro(world):
    """(updates, ranks, passes) micro-batches of 2 images"""
    g = torch.Generator().manual_seed(7)
    xs = torch.rand(UPDATES, world, K2, 2, 3, 8, 8, generator=g)
    return xs, torch.rand(UPDATES, world, K2, 2, 3, 8, 8, generator=g)


def _worker(rank, world, port, q):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = [0]
    real = dist.all_reduce

    def counting(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)

    dist.all_reduce = counting
    from hvi_cidnet_amd.dp import DataParallelTrainer
    torch.manual_seed(100 + rank)                       # different init per rank: the broadcast must fix it, the EMA too
    tr = DataParallelTrainer(Net(), lr=1e-2, n_buckets=3, loss_fn=l1, use_hip_kernels=False, accum_steps=K2, ema_decay=0.9)
    xs, gts = _micro(world)
    per_update = []
    for u in range(UPDATES):
        for j in range(K2):
            if j == K2 - 1:
                c0 = calls[0]                           # the setup's layout check is behind us: count from the last pass on
            elif u:
                c1 = calls[0]
            tr.step(xs[u, rank, j], gts[u, rank, j])
            if j < K2 - 1 and u:
                assert calls[0] == c1                   # no collective before the K-th pass
        per_update.append(calls[0] - c0)
    # an open group of one pass, flushed: one collective
    tr.step(xs[0, rank, 0], gts[0, rank, 0])
    c0 = calls[0]
    tr.flush()
    flush_calls = calls[0] - c0
    q.put((rank, tr.flat_p.numpy().copy(), tr.ema.numpy().copy(), len(tr.buckets), per_update, flush_calls,
           {n: (off, c) for n, off, c, _ in tr._live_named()}))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_accumulate_with_one_all_reduce_per_bucket():
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r, *rest = q.get(timeout=240)
        res[r] = rest
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    p0, e0, nb, per_update, flush_calls, layout = res[0]
    assert nb >= 2
    for r in range(world):
        assert res[r][3] == [nb] * UPDATES, res[r][3]   # one all-reduce per bucket per update, not per pass
        assert res[r][4] == 1
    assert p0.tobytes() == res[1][0].tobytes() and e0.tobytes() == res[1][1].tobytes()
    assert not np.array_equal(p0, e0)
    # one process, K = 4, over the same micro-batches; then the flushed group: both ranks' first micro-batch, K = 2
    torch.manual_seed(100)
    net = Net()
    xs, gts = _micro(world)
    one = _trainer(net, accum_steps=world * K2, ema_decay=0.9)
    for u in range(UPDATES):
        for r in range(world):
            for j in range(K2):
                one.step(xs[u, r, j], gts[u, r, j])
    for r in range(world):
        one.step(xs[0, r, 0], gts[0, r, 0])
    assert one.pending_passes == 2
    one.flush()
    assert {n: (off, c) for n, off, c, _ in one._live_named()} == layout
    for got, want, what in ((p0, one.flat_p, "p"), (e0, one.ema, "ema")):
        got = torch.from_numpy(got)
        assert torch.allclose(got, want, atol=2e-6, rtol=1e-5), (what, (got - want).abs().max())
