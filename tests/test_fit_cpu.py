"""CPU: the training run driver (hvi-cidnet_amd/fit.py) and the guarded optimizer's plain-torch restatement
(dp.FlatAdam(kernel=False, max_grad_norm / skip_nonfinite / device_state)) on a toy model: schedule wiring and snapshot
files, the guard against clip_grad_norm_ + torch.optim.Adam, exact resume, and the strictness of the trainer's state."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn


def _toy(seed=0):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Conv2d(3, 6, 3, padding=1), nn.Tanh(), nn.Conv2d(6, 3, 1))


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Conv2d(3, 8, 3, padding=1)
        self.b = nn.Conv2d(8, 3, 1)
        self.dead = nn.Linear(4, 4)                      # never used: no gradient, no optimizer state (like I_LCA5)

    def forward(self, x):
        return self.b(torch.tanh(self.a(x)))


def l1(out, gt):
    return (out - gt).abs().mean()


class ListBatches:
    """epoch(e) is a function of (seed, e), as data.TrainBatches' plan is"""

    def __init__(self, steps=3, seed=5, shape=(2, 3, 8, 8)):
        self.steps, self.seed, self.shape = steps, seed, shape

    def __len__(self):
        return self.steps

    def epoch(self, e):
        g = torch.Generator().manual_seed(1000 * self.seed + e)
        for _ in range(self.steps):
            yield torch.rand(self.shape, generator=g), torch.rand(self.shape, generator=g)


CPU = dict(use_hip_kernels=False)


@pytest.mark.parametrize("start_warmup,start_epoch", [(True, 0), (False, 0), (True, 2), (False, 1)])
def test_fit_schedule_and_snapshots(tmp_path, start_warmup, start_epoch):
    from hvi_cidnet_amd import WarmupCosineLR, fit
    n, warm, snap = 7, 2, 3
    model = _toy()
    seen = []
    recs = fit(model, ListBatches(), nEpochs=n, lr=1e-3, warmup_epochs=warm, start_warmup=start_warmup,
               start_epoch=start_epoch, snapshots=snap, loss_fn=l1, out_dir=str(tmp_path), on_epoch=seen.append,
               trainer_args=CPU)
    sched = WarmupCosineLR(1e-3, n, warm, start_epoch, start_warmup)
    assert [r["epoch"] for r in recs] == list(range(start_epoch + 1, start_epoch + n + 1))
    assert [r["lr"] for r in recs] == [sched.lr_after(k) for k in range(n)]
    assert seen == recs
    assert all(r["steps"] == 3 and r["skipped"] == 0 and r["clipped"] == 0 and np.isfinite(r["loss"]) for r in recs)
    want = sorted(f"epoch_{e}{ext}" for e in range(start_epoch + 1, start_epoch + n + 1) if e % snap == 0
                  for ext in (".pth", ".train.pt"))
    assert sorted(os.listdir(tmp_path)) == want and want
    last = max(e for e in range(start_epoch + 1, start_epoch + n + 1) if e % snap == 0)
    fresh = _toy(seed=9)
    fresh.load_state_dict(torch.load(tmp_path / f"epoch_{last}.pth"), strict=True)
    if last == start_epoch + n:
        for a, b in zip(fresh.parameters(), model.parameters()):
            assert torch.equal(a, b)


def _flat_twin(model):
    """(model copy, its parameters) for clip_grad_norm_ + torch.optim.Adam beside the trainer"""
    twin = copy.deepcopy(model)
    return twin, list(twin.parameters())


def test_guard_restatement_matches_clip_grad_norm_and_adam():
    from hvi_cidnet_amd.dp import DataParallelTrainer, StepLog
    model = _toy(1)
    twin, tparams = _flat_twin(model)
    opt = torch.optim.Adam(tparams, lr=1e-2)
    scale = {"v": 1.0}
    log = StepLog(8)
    tr = DataParallelTrainer(model, lr=1e-2, loss_fn=lambda o, g: l1(o, g) * scale["v"], max_grad_norm=0.01,
                             skip_nonfinite=True, step_log=log, **CPU)
    b = list(ListBatches(steps=3).epoch(0))

    def twin_step(x, gt):
        opt.zero_grad()
        l1(twin(x), gt).backward()
        norm = torch.nn.utils.clip_grad_norm_(tparams, 0.01)
        opt.step()
        return float(norm)

    def close():
        for p, t in zip(model.parameters(), tparams):
            assert torch.allclose(p, t, atol=1e-7, rtol=1e-6)

    tr.step(*b[0])
    norm0 = twin_step(*b[0])
    close()
    assert tr.opt.steps_applied() == 1 and tr.opt.steps_skipped() == 0
    rows = log.read()
    assert rows.shape == (1, 4) and rows[0, 3] == 1 and rows[0, 2] < 1.0
    assert abs(rows[0, 1] - norm0) <= 1e-5 * norm0
    # a poisoned batch: parameters, both moments and the applied count stay where they were
    before = [t.clone() for t in (tr.flat_p, tr.opt.m, tr.opt.v)]
    scale["v"] = float("nan")
    tr.step(*b[1])
    scale["v"] = 1.0
    for was, now in zip(before, (tr.flat_p, tr.opt.m, tr.opt.v)):
        assert torch.equal(was, now)
    assert tr.opt.steps_applied() == 1 and tr.opt.steps_skipped() == 1
    assert log.read()[1, 3] == -2
    # the next clean step is the twin's next step
    tr.step(*b[2])
    twin_step(*b[2])
    close()
    assert tr.opt.steps_applied() == 2 and log.read()[2, 3] == 2


def test_unguarded_flat_adam_is_unchanged():
    """all three switches off: the host-count object of before (no device state at all)"""
    from hvi_cidnet_amd.dp import FlatAdam
    p = torch.arange(6, dtype=torch.float32)
    a = FlatAdam(p.clone(), lr=1e-2, kernel=False)
    assert not a.guarded and not hasattr(a, "state")
    g = torch.linspace(-1, 1, 6)
    a.step(g, 6)
    t = p.clone().requires_grad_(True)
    t.grad = g.clone()
    torch.optim.Adam([t], lr=1e-2).step()
    assert a.t == 1 and a.steps_applied() == 1 and torch.allclose(a.p, t.detach(), atol=1e-7, rtol=1e-6)


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=False)


# the learning rate differs between the snapshot epoch and the one after it in every case: resume inside the warm-up
# (default warm-up of 3), inside the cosine part behind it, and inside the cosine part without warm-up
@pytest.mark.parametrize("sched,at", [(dict(), 2), (dict(), 6), (dict(start_warmup=False), 2),
                                      (dict(warmup_epochs=1), 2)])
def test_fit_exact_resume(tmp_path, sched, at):
    from hvi_cidnet_amd import WarmupCosineLR, fit
    kw = dict(nEpochs=8, lr=1e-2, snapshots=2, loss_fn=l1, max_grad_norm=0.05, trainer_args=CPU, **sched)
    full = fit(_toy(2), ListBatches(), out_dir=str(tmp_path / "a"), **kw)
    w = WarmupCosineLR(1e-2, 8, sched.get("warmup_epochs", 3), 0, sched.get("start_warmup", True))
    assert [r["lr"] for r in full] == [w.lr_after(k) for k in range(8)]
    if "warmup_epochs" not in sched:
        assert w.lr_after(at - 1) != w.lr_after(at)
    first = []

    class Stop(Exception):
        pass

    def stop_there(rec):
        first.append(rec)
        if rec["epoch"] == at:
            raise Stop

    with pytest.raises(Stop):
        fit(_toy(2), ListBatches(), out_dir=str(tmp_path / "b"), on_epoch=stop_there, **kw)
    rest = fit(_toy(7), ListBatches(), out_dir=str(tmp_path / "b"), resume=str(tmp_path / "b" / f"epoch_{at}.train.pt"), **kw)
    assert [r["epoch"] for r in rest] == list(range(at + 1, 9))
    assert first + rest == full
    wa, wb = _load(tmp_path / "a" / "epoch_8.pth"), _load(tmp_path / "b" / "epoch_8.pth")
    assert wa.keys() == wb.keys() and all(torch.equal(wa[k], wb[k]) for k in wa)
    sa, sb = _load(tmp_path / "a" / "epoch_8.train.pt"), _load(tmp_path / "b" / "epoch_8.train.pt")
    for k in ("exp_avg", "exp_avg_sq"):
        assert sa["trainer"][k].keys() == sb["trainer"][k].keys()
        assert all(torch.equal(sa["trainer"][k][n], sb["trainer"][k][n]) for n in sa["trainer"][k])
    assert sa["trainer"]["steps_applied"] == sb["trainer"]["steps_applied"] == 24
    assert sa["trainer"]["lr"] == sb["trainer"]["lr"] == full[-1]["lr"]
    assert sa["epochs_done"] == sb["epochs_done"] == 8
    # another schedule than the file's is refused
    with pytest.raises(ValueError, match="resume"):
        fit(_toy(7), ListBatches(), resume=str(tmp_path / "b" / f"epoch_{at}.train.pt"), **{**kw, "nEpochs": 9})


def test_load_state_dict_hyper_parameters_and_set_lr_order():
    """lr, betas, eps and weight decay come from the loaded state, whatever the new trainer was built with; a set_lr after
    the load wins, before the first step (state still parked) and after it"""
    from hvi_cidnet_amd.dp import DataParallelTrainer
    b = list(ListBatches(steps=4).epoch(0))
    hyper = dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.01)

    def reference(lr3):
        torch.manual_seed(0)
        t = DataParallelTrainer(Net(), loss_fn=l1, skip_nonfinite=True, **hyper, **CPU)
        for x, gt in b[:2]:
            t.step(x, gt)
        sd, w = copy.deepcopy(t.state_dict()), {k: v.clone() for k, v in t.model.state_dict().items()}
        if lr3 is not None:
            t.set_lr(lr3)
        t.step(*b[2])
        return t, sd, w

    for lr3 in (None, 7e-4):
        ref, sd, w = reference(lr3)
        assert (sd["lr"], sd["betas"], sd["eps"], sd["weight_decay"]) == (3e-3, (0.8, 0.95), 1e-6, 0.01)
        for early in (True, False):
            torch.manual_seed(1)
            m2 = Net()
            t2 = DataParallelTrainer(m2, lr=0.5, loss_fn=l1, skip_nonfinite=True, **CPU)     # other hyper-parameters
            if not early:
                t2.step(*b[3])
            t2.load_state_dict(copy.deepcopy(sd))
            m2.load_state_dict(w)
            if lr3 is not None:
                t2.set_lr(lr3)
            t2.step(*b[2])
            o = t2.opt
            assert (o.lr, o.betas, o.eps, o.wd) == (3e-3 if lr3 is None else lr3, (0.8, 0.95), 1e-6, 0.01)
            assert t2.state_dict()["lr"] == o.lr
            assert torch.equal(t2.flat_p[:t2.n_live], _reorder(ref, t2)), (lr3, early)


@pytest.mark.parametrize("guarded", [False, True])
def test_trainer_state_dict_round_trip_is_strict(guarded):
    from hvi_cidnet_amd.dp import DataParallelTrainer
    kw = dict(lr=1e-2, loss_fn=l1, skip_nonfinite=guarded, **CPU)
    b = list(ListBatches(steps=3).epoch(0))
    torch.manual_seed(0)
    tr = DataParallelTrainer(Net(), **kw)
    for x, gt in b[:2]:
        tr.step(x, gt)
    sd = tr.state_dict()
    assert sd["steps_applied"] == 2 and sd["steps_skipped"] == 0 and sd["lr"] == 1e-2
    assert not any(n.startswith("dead") for n in sd["exp_avg"]) and "a.weight" in sd["exp_avg"]
    assert all(not t.is_cuda and t.shape == dict(tr.model.named_parameters())[n].shape for n, t in sd["exp_avg_sq"].items())
    tr.step(*b[2])
    # loaded before the first step and after it: both continue as the original
    for early in (True, False):
        torch.manual_seed(0)
        m2 = Net()
        t2 = DataParallelTrainer(m2, **kw)
        if not early:
            t2.step(*b[0])
        ref_w = copy.deepcopy(sd)
        t2.load_state_dict(ref_w)
        m2.load_state_dict(_weights_after_two(kw, b))
        t2.step(*b[2])
        assert t2.opt.steps_applied() == 3
        assert torch.equal(t2.flat_p[:t2.n_live], _reorder(tr, t2))
    # strictness
    for mutate, exc in ((lambda s: s["exp_avg"].pop("a.weight"), KeyError),
                        (lambda s: s["exp_avg"].__setitem__("nope", torch.zeros(1)), KeyError),
                        (lambda s: s["exp_avg"].__setitem__("dead.weight", torch.zeros(4, 4)), KeyError),
                        (lambda s: s["exp_avg_sq"].__setitem__("a.bias", torch.zeros(9)), ValueError)):
        bad = copy.deepcopy(sd)
        mutate(bad)
        with pytest.raises(exc):
            tr.load_state_dict(bad)


def _weights_after_two(kw, b):
    from hvi_cidnet_amd.dp import DataParallelTrainer
    torch.manual_seed(0)
    m = Net()
    t = DataParallelTrainer(m, **kw)
    for x, gt in b[:2]:
        t.step(x, gt)
    return {k: v.clone() for k, v in m.state_dict().items()}


def _reorder(src, dst):
    """src's live parameters in dst's arena order"""
    by_name = {n: src.flat_p[off:off + c] for n, off, c, _ in src._live_named()}
    return torch.cat([by_name[n] for n, *_ in dst._live_named()])


def test_step_log_wraps_and_reads_in_step_order():
    from hvi_cidnet_amd.dp import StepLog
    log = StepLog(3).bind("cpu")
    for i in range(5):
        log.next_row().copy_(torch.full((4,), float(i), dtype=torch.float64))
    assert log.read()[:, 0].tolist() == [2.0, 3.0, 4.0]
    log.reset()
    assert log.read().shape == (0, 4)
