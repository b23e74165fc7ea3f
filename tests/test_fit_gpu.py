"""GPU: the training run driver (hvi-cidnet_amd/fit.py) over data.TrainBatches and the full-width CIDNet: the copies an
epoch makes, exact resume in the fp32 and the bf16 mode at three points of the schedule, and the records of a run against a
hand-written loop and a direct metrics.evaluate call."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import cidnet_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import data_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
FULL = (36, 36, 72, 144)
CROP = (64, 96)


def _model(dev, seed=21):
    import hvi_cidnet_amd as P
    m = P.CIDNet(channels=list(FULL))
    p = O.make_params(seed, channels=FULL)
    m.load_state_dict({k: p[k] for k in m.state_dict().keys()})
    return m.to(dev)


def _batches(dev, seed=23, n=6, batch=2):
    import hvi_cidnet_amd as P
    sizes = [(80, 120), (64, 96), (100, 130)] * (n // 3)
    pairs = P.ResidentPairs(R.random_images(seed, sizes), R.random_images(seed + 1000, sizes), dev)
    return P.TrainBatches(pairs, batch, CROP, seed=3, gamma=(60, 120))


def _val_pairs(seed=77, n=2):
    lows = R.random_images(seed, [CROP] * n)
    highs = R.random_images(seed + 1, [CROP] * n)
    return [(torch.from_numpy(a).permute(2, 0, 1).float().div(255) * 0.4, b) for a, b in zip(lows, highs)]


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def _copies(fn):
    """names of the memory-copy activities the profiler attributes to fn()"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = []
    for ev in prof.events():
        names += [k.name for k in (getattr(ev, "kernels", []) or []) if "memcpy" in k.name.lower()]
    return names


def test_epoch_copies_the_plan_up_and_the_log_down(dev):
    """an epoch of the driver (one without a snapshot: validation has copies of its own): one host-to-device copy, the plan,
    and one device-to-host copy, the step log"""
    from hvi_cidnet_amd import StepLog, run_epoch
    from hvi_cidnet_amd.dp import DataParallelTrainer
    tb = _batches(dev)
    log = StepLog(len(tb))
    tr = DataParallelTrainer(_model(dev), lr=1e-4, max_grad_norm=1.0, skip_nonfinite=True, step_log=log)
    run_epoch(tr, tb, 1, log)
    out = []
    names = [n.lower() for n in _copies(lambda: out.append(run_epoch(tr, tb, 2, log)))]
    assert sorted("htod" if "htod" in n else "dtoh" if "dtoh" in n else n for n in names) == ["dtoh", "htod"], names
    assert out[0].shape == (len(tb), 4) and out[0][:, 3].tolist() == [len(tb) + 1 + i for i in range(len(tb))]


# resume inside the default warm-up of 3, inside the cosine part behind it, and without warm-up: the learning rate of the
# snapshot epoch differs from the next one's in each
@pytest.mark.parametrize("precision,start_warmup,at", [("f32", True, 2), ("f32", True, 6), ("bf16", False, 2)])
def test_fit_exact_resume_on_the_device(dev, tmp_path, precision, start_warmup, at):
    """8 epochs against `at` epochs + a fresh model and trainer + resume for the rest: weights, both moments and the records
    are bit-identical"""
    import hvi_cidnet_amd as P
    kw = dict(nEpochs=8, lr=2e-4, start_warmup=start_warmup, snapshots=2, max_grad_norm=1.0)
    w = P.WarmupCosineLR(2e-4, 8, 3, 0, start_warmup)
    assert w.lr_after(at - 1) != w.lr_after(at)
    P.set_precision(precision)
    try:
        full = P.fit(_model(dev), _batches(dev), out_dir=str(tmp_path / "a"), **kw)
        first = []

        class Stop(Exception):
            pass

        def stop_there(rec):
            first.append(rec)
            if rec["epoch"] == at:
                raise Stop

        with pytest.raises(Stop):
            P.fit(_model(dev), _batches(dev), out_dir=str(tmp_path / "b"), on_epoch=stop_there, **kw)
        rest = P.fit(_model(dev, seed=5), _batches(dev), out_dir=str(tmp_path / "b"),
                     resume=str(tmp_path / "b" / f"epoch_{at}.train.pt"), **kw)
    finally:
        P.set_precision("f32")
    assert [r["lr"] for r in full] == [w.lr_after(k) for k in range(8)]
    assert [r["epoch"] for r in rest] == list(range(at + 1, 9)) and first + rest == full, (first + rest, full)
    assert all(r["skipped"] == 0 and np.isfinite(r["loss"]) for r in full)
    wa, wb = _load(tmp_path / "a" / "epoch_8.pth"), _load(tmp_path / "b" / "epoch_8.pth")
    assert wa.keys() == wb.keys() and all(torch.equal(wa[k].view(torch.int32), wb[k].view(torch.int32)) for k in wa)
    sa, sb = _load(tmp_path / "a" / "epoch_8.train.pt")["trainer"], _load(tmp_path / "b" / "epoch_8.train.pt")["trainer"]
    assert len(sa["exp_avg"]) > 150 and not any(n.startswith("I_LCA5") for n in sa["exp_avg"])
    for k in ("exp_avg", "exp_avg_sq"):
        assert sa[k].keys() == sb[k].keys()
        assert all(torch.equal(sa[k][n].view(torch.int32), sb[k][n].view(torch.int32)) for n in sa[k]), k
    assert sa["steps_applied"] == sb["steps_applied"] == 24
    # the weights moved at all
    w2 = _load(tmp_path / "a" / "epoch_2.pth")
    assert any(not torch.equal(w2[k], wa[k]) for k in wa)


def test_fit_records_against_a_hand_written_loop_and_evaluate(dev, tmp_path):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd.dp import DataParallelTrainer
    val = _val_pairs()
    kw = dict(nEpochs=3, lr=2e-4, warmup_epochs=1)
    recs = P.fit(_model(dev), _batches(dev), snapshots=1, max_grad_norm=1.0, val_pairs=val, out_dir=str(tmp_path), **kw)
    assert [r["epoch"] for r in recs] == [1, 2, 3]
    # validation: a direct call on the saved weights
    for r in recs:
        m = _model(dev, seed=9)
        m.load_state_dict(_load(tmp_path / f"epoch_{r['epoch']}.pth"), strict=True)
        res = P.evaluate(m, val)
        assert (r["psnr"], r["ssim"]) == (res.psnr, res.ssim), (r, res.psnr, res.ssim)
    # the loss: the reference's way, .item() after every step, over the same plan
    tb = _batches(dev)
    sched = P.WarmupCosineLR(kw["lr"], kw["nEpochs"], kw["warmup_epochs"])
    tr = DataParallelTrainer(_model(dev), lr=sched.lr_after(0), max_grad_norm=1.0, skip_nonfinite=True)
    for k, r in enumerate(recs):
        assert sched.apply(tr, k) == r["lr"]
        losses = [float(tr.step(x, gt).item()) for x, gt in tb.epoch(r["epoch"])]
        total = 0.0
        for v in losses:
            total += v
        assert r["loss"] == total / len(losses), (r["loss"], total / len(losses))
        assert r["steps"] == len(losses) and r["skipped"] == 0 and r["grad_norm_max"] > 0
