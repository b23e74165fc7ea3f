"""The training run: the epoch loop of the reference's train.py:195-274 over the pieces this package already has --
data.TrainBatches (the batches), dp.DataParallelTrainer (the step, here with its guard), schedule.WarmupCosineLR (the
learning rate of every epoch), metrics.evaluate (validation) and the reference's checkpoint format.

    from hvi_cidnet_amd import CIDNet, CIDNetLoss, ResidentPairs, TrainBatches, fit, folder_pairs
    model = CIDNet().to(device)
    pairs = ResidentPairs.from_folders(low_dir, high_dir, device)
    batches = TrainBatches(pairs, batch_size=8, crop=256, seed=0, gamma=(60, 120))
    records = fit(model, batches, nEpochs=1000, lr=1e-4, loss_fn=CIDNetLoss(model), max_grad_norm=1.0,
                  val_pairs=folder_pairs(val_low, val_high), out_dir="weights/train", on_epoch=print)

Inside an epoch the host never waits for the device except through the trainer's own back-pressure: the loss, the gradient
norm, the clip coefficient and the apply / skip decision of every step are written by the guard into a device-resident step
log (dp.StepLog) that is read once, after the epoch's last step.

What differs from the reference's loop:
  * the reference calls clip_grad_norm_ BEFORE zero_grad() / backward() (train.py:68-73), so it clips the previous step's
    gradients and changes nothing; here the clip sits between the backward and the update, and a step whose gradient holds
    a NaN or an Inf is skipped on the device (skip_nonfinite) instead of poisoning the weights and both Adam moments;
  * `resume=` continues a run exactly (Adam moments, step counts, schedule position); the reference's own resume
    (`start_epoch` > 0: weights only, fresh Adam, restarted warm-up, shortened cosine period) is kept as it is;
  * the reference's two tools against gradient explosion are opt-in and device-side: diagnose=True logs per-tensor gradient
    and weight statistics of every update (dp.TensorLog; what --grad_detect's set_detect_anomaly answers, without a host
    wait or a second backward) and preview_dir= writes the per-epoch test.png / gt.png of train.py:84-89, clamped where
    the reference's ToPILImage wraps (the validation's enhanced images can be written as well: val_args=dict(save_dir=...),
    metrics.evaluate);
  * left out: the metrics .md table (on_epoch hands the numbers to the caller), the
    option parser, the cyclic scheduler variant.  LPIPS is opt-in: val_args=dict(lpips=params or the two paths) adds
    `lpips` (and `lpips_ema`) to the record (metrics.evaluate(lpips=)); so is the CIEDE2000 colour difference:
    val_args=dict(ciede2000=True) adds `ciede2000` (and `ciede2000_ema`).
The sets kept as one sub-folder per scene (SICE / SID / LOL-blur, data/SICE_blur_SID.py) train through the same loop:
data.ResidentPairs.from_scene_folders and TrainBatches(sampling="scene") draw a scene, then one of its images; and a batch
source that yields (x, gt, raw) -- TrainBatches(raw=True), the low image before `** gamma` -- has its third element handed to
the step as raw_input, which is what train_tnsm.py:55,68 gives the TNSM loss.  fit() itself takes no argument for either.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.distributed as dist

from .dp import DataParallelTrainer, StepLog, TensorLog
from .schedule import WarmupCosineLR

_SCHEDULE_KEYS = ("nEpochs", "lr", "warmup_epochs", "start_warmup", "start_epoch")


def run_epoch(trainer, batches, epoch, step_log, last_batch=None):
    """The steps of one epoch and ONE read of the step log -> its rows, (updates, 4) fp64 (dp.StepLog's columns).  With
    accum_steps = K > 1 a batch is one pass and a row one update; a group the epoch's last batch leaves open is applied
    from the passes it has (trainer.flush), so 61 batches with K = 4 are 16 updates, the last from one pass.
    last_batch: a list that is cleared and then holds the epoch's last batch (fit's preview reads it)."""
    step_log.reset()
    batch = None
    for batch in batches.epoch(epoch):                           # (x, gt) or (x, gt, raw): the third is the step's raw_input
        trainer.step(*batch)
    if last_batch is not None:
        last_batch[:] = [] if batch is None else [batch]
    if trainer.pending_passes > 0:
        trainer.flush()
    return step_log.read()


def epoch_stats(rows):
    """The record entries that come out of an epoch's step log; the loss is the fp64 mean, summed in step order, of the
    applied steps' losses (NaN when none was applied)"""
    applied = rows[:, StepLog.COUNT] > 0
    total = 0.0
    for v in rows[applied, StepLog.LOSS]:
        total += float(v)
    n = int(applied.sum())
    norms = rows[:, StepLog.NORM]
    finite = norms[np.isfinite(norms)]
    return {"steps": int(rows.shape[0]), "skipped": int(rows.shape[0]) - n, "loss": total / n if n else float("nan"),
            "grad_norm_max": float(finite.max()) if finite.size else float("nan"),
            "clipped": int((rows[applied, StepLog.COEF] < 1.0).sum())}


def diagnose_epoch(rows, stats, names, what=("grad", "weight"), top=5):
    """The record's `diagnosis` from an epoch's step log rows and tensor log rows (dp.TensorLog.read(): (updates, len(what),
    T, 4)); names: the tensors in arena order.
      nonfinite: one entry per update whose gradient held a non-finite element -- update (index in the epoch), applied,
        tensors (the affected names in arena order) and origin (name, tensor, element of the first of them: the
        parameter nearest the loss in gradient-ready order);
      grad_top: the `top` tensors by their largest gradient norm over the applied updates -- name, norm, update;
      weights_nonfinite: names of the tensors whose weights held a non-finite element at any update."""
    n = min(rows.shape[0], stats.shape[0])
    out = {"nonfinite": [], "grad_top": [], "weights_nonfinite": []}
    applied = rows[:n, StepLog.COUNT] > 0
    if "grad" in what:
        g = stats[:n, what.index("grad")]
        for u in range(n):
            bad = np.flatnonzero(g[u, :, TensorLog.NONFINITE] > 0)
            if bad.size:
                t = int(bad[0])
                out["nonfinite"].append({"update": u, "applied": bool(applied[u]), "tensors": [names[i] for i in bad],
                                         "origin": {"name": names[t], "tensor": t, "element": int(g[u, t, TensorLog.FIRST])}})
        if applied.any():
            norms = np.where(applied[:, None], g[:, :, TensorLog.NORM], -1.0)
            at = norms.argmax(axis=0)
            best = norms[at, np.arange(norms.shape[1])]
            order = sorted(range(len(names)), key=lambda i: (-best[i], i))[:max(int(top), 0)]
            out["grad_top"] = [{"name": names[i], "norm": float(best[i]), "update": int(at[i])} for i in order]
    if "weight" in what:
        w = stats[:n, what.index("weight")]
        out["weights_nonfinite"] = [names[i] for i in np.flatnonzero((w[:, :, TensorLog.NONFINITE] > 0).any(axis=0))]
    return out


def preview_bytes(img):
    """(3, h, w) fp32 -> (h, w, 3) uint8 as a numpy array, trunc(clamp(v, 0, 1) * 255): image_io.egress on the device, its
    plain-torch restatement for a CPU tensor"""
    if img.is_cuda:
        from . import image_io
        return image_io.egress(img.unsqueeze(0).contiguous())[0].cpu().numpy()
    return (img.detach().float().clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()


def write_preview(model, batch, preview_dir):
    """The reference's per-epoch preview (train.py:84-89): test.png = the model's output for the first sample of `batch`
    (a no_grad forward in the mode the model is in; a tuple result's first element), gt.png = that sample's ground truth,
    each epoch over the last.  The reference hands the unclamped tensor to ToPILImage, whose .byte() wraps values outside
    [0, 1]; this clamps."""
    from PIL import Image
    x, gt = batch[0], batch[1]
    with torch.no_grad():
        out = model(x[:1])
    if isinstance(out, (tuple, list)):
        out = out[0]
    os.makedirs(preview_dir, exist_ok=True)
    Image.fromarray(preview_bytes(out[0])).save(os.path.join(preview_dir, "test.png"))
    Image.fromarray(preview_bytes(gt[0])).save(os.path.join(preview_dir, "gt.png"))


def _model_device(model):
    for p in model.parameters():
        return p.device
    raise RuntimeError("fit: the model has no parameters")


def fit(model, batches, *, nEpochs, lr, warmup_epochs=3, start_warmup=True, start_epoch=0, snapshots=10, loss_fn=None,
        max_grad_norm=None, skip_nonfinite=True, val_pairs=None, val_args=None, out_dir=None, resume=None,
        process_group=None, on_epoch=None, trainer_args=None, accum_steps=1, ema_decay=None, val_weights="model",
        diagnose=False, diagnose_top=5, preview_dir=None):
    """Train `model` for the epochs start_epoch + 1 ... start_epoch + nEpochs and return one record per epoch.

    batches: anything with __len__ (steps per epoch) and epoch(e) yielding (x, gt) or (x, gt, raw): data.TrainBatches.
    The learning rate of the k-th epoch of this run (k = 0, 1, ...) is WarmupCosineLR(lr, nEpochs, warmup_epochs,
    start_epoch, start_warmup).lr_after(k): the reference constructs its scheduler, trains an epoch, then steps it, so with
    warm-up the first epoch runs at lr 0 (schedule.py lists the quirks); past the reference's single cosine period the
    schedule is undefined and raises, as the reference fails there.
    Every `snapshots` epochs rank 0 writes, into out_dir, epoch_{epoch}.pth (the model's state_dict(), what the reference
    loads with strict=True) and epoch_{epoch}.train.pt (the trainer's state_dict(), the epoch, the position in the schedule
    and the arguments that fix it); then, when val_pairs is given, metrics.evaluate(model, val_pairs, **val_args) runs and
    the record gains psnr / ssim, lpips when val_args carries lpips= and ciede2000 when it carries ciede2000=True (val_args may carry save_dir: the scored images are then also written there, each
    validation over the last one's files).
    Record: epoch, lr, steps, skipped, loss (mean over the applied steps, see epoch_stats; averaged over the ranks with one
    all-reduce per epoch), grad_norm_max, clipped (applied steps with coef < 1).  on_epoch(record) runs on every rank.
    start_epoch > 0 is the reference's resume: the caller loads weights, Adam starts fresh, the warm-up restarts.
    resume = path of an epoch_*.train.pt: the exact one.  The trainer's state and the epoch counter come from the file, the
    model's weights from the epoch_*.pth beside it, the schedule continues where it was (its arguments must be the file's);
    since data.epoch_plan is a function of (seed, epoch) and every reduction of a step has a fixed order, the run continues
    bit-identically.  trainer_args: further DataParallelTrainer arguments.
    accum_steps = K: every batch is one pass of an update summed over K of them (DataParallelTrainer); `steps`, `skipped` and
    the loss of the record then count updates, ceil(len(batches) / K) per epoch, the last one from the batches that are left.
    ema_decay: the trainer keeps an exponential moving average of the weights; a snapshot also writes epoch_{epoch}.ema.pth
    (trainer.ema_state_dict(), the same checkpoint format) and `resume=` restores the average with the rest.
    val_weights: "model" validates the trained weights (psnr / ssim), "ema" the averaged ones (psnr_ema / ssim_ema,
    evaluated inside trainer.ema_weights()), "both" both; "ema" and "both" need ema_decay.
    diagnose: the trainer also writes a dp.TensorLog sized like the step log (per-tensor statistics of every update's
    gradient and weights, four more launches per update and nothing else), read once per epoch beside the step log; the
    record gains `diagnosis` (diagnose_epoch: nonfinite, grad_top with diagnose_top entries, weights_nonfinite).  Nothing of
    it is stored in a snapshot.
    preview_dir: after every epoch rank 0 writes test.png and gt.png there (write_preview) from the first sample of the
    epoch's last batch, after the epoch's last update.
    With the defaults neither adds a launch or a record key."""
    if val_weights not in ("model", "ema", "both"):
        raise ValueError(f"fit: val_weights must be 'model', 'ema' or 'both' (got {val_weights!r})")
    if val_weights != "model" and ema_decay is None:
        raise ValueError(f"fit: val_weights={val_weights!r} needs ema_decay")
    accum_steps = int(accum_steps)
    if accum_steps < 1:
        raise ValueError("fit: accum_steps must be at least 1")
    sched_args = dict(nEpochs=int(nEpochs), lr=float(lr), warmup_epochs=int(warmup_epochs), start_warmup=bool(start_warmup),
                      start_epoch=int(start_epoch))
    sched = WarmupCosineLR(sched_args["lr"], sched_args["nEpochs"], sched_args["warmup_epochs"], sched_args["start_epoch"],
                           sched_args["start_warmup"])
    snapshots = int(snapshots)
    if snapshots <= 0:
        raise ValueError("fit: snapshots must be positive")
    if len(batches) <= 0:
        raise ValueError("fit: an epoch without steps")
    log = StepLog(-(-len(batches) // accum_steps))                # one row per update
    extra = dict(trainer_args or {})
    tlog = None
    if diagnose:
        tlog = extra["tensor_log"] = TensorLog(log.capacity)
    trainer = DataParallelTrainer(model, lr=sched.lr_after(0), loss_fn=loss_fn, process_group=process_group,
                                  max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, step_log=log,
                                  accum_steps=accum_steps, ema_decay=ema_decay, **extra)
    first, done = sched_args["start_epoch"] + 1, 0
    if resume is not None:
        saved = torch.load(resume, map_location="cpu", weights_only=False)
        for k in _SCHEDULE_KEYS:
            if saved["schedule"][k] != sched_args[k]:
                raise ValueError(f"fit: resume file was written with {k} = {saved['schedule'][k]!r}, this call has {sched_args[k]!r}")
        weights = os.path.join(os.path.dirname(os.path.abspath(resume)), saved["weights"])
        model.load_state_dict(torch.load(weights, map_location="cpu"), strict=True)
        trainer.load_state_dict(saved["trainer"])
        first, done = int(saved["epoch"]) + 1, int(saved["epochs_done"])
    rank, world = trainer.rank, trainer.world
    if out_dir is not None and rank == 0:
        os.makedirs(out_dir, exist_ok=True)
    records = []
    for epoch in range(first, sched_args["start_epoch"] + sched_args["nEpochs"] + 1):
        lr_now = sched.apply(trainer, done)
        model.train()
        last = [] if preview_dir is not None else None
        if tlog is not None:
            tlog.reset()
        rows = run_epoch(trainer, batches, epoch, log, last_batch=last)
        done += 1
        rec = {"epoch": epoch, "lr": lr_now, **epoch_stats(rows)}
        if tlog is not None:
            rec["diagnosis"] = diagnose_epoch(rows, tlog.read(), tlog.names, tlog.what, diagnose_top)
        if last and rank == 0:
            write_preview(model, last[0], preview_dir)
        if world > 1:
            t = torch.tensor([rec["loss"]], dtype=torch.float64, device=_model_device(model))
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=process_group)
            rec["loss"] = float(t.item()) / world
        if epoch % snapshots == 0:
            if out_dir is not None and rank == 0:
                _snapshot(model, trainer, out_dir, epoch, done, sched_args)
            if val_pairs is not None and val_weights in ("model", "both"):
                res = _validate(model, val_pairs, val_args, process_group)
                rec["psnr"], rec["ssim"] = res.psnr, res.ssim
                if (val_args or {}).get("lpips") is not None:
                    rec["lpips"] = res.lpips
                if (val_args or {}).get("ciede2000"):
                    rec["ciede2000"] = res.ciede2000
            if val_pairs is not None and val_weights in ("ema", "both"):
                with trainer.ema_weights():
                    res = _validate(model, val_pairs, val_args, process_group)
                rec["psnr_ema"], rec["ssim_ema"] = res.psnr, res.ssim
                if (val_args or {}).get("lpips") is not None:
                    rec["lpips_ema"] = res.lpips
                if (val_args or {}).get("ciede2000"):
                    rec["ciede2000_ema"] = res.ciede2000
        records.append(rec)
        if on_epoch is not None:
            on_epoch(rec)
    return records


def _validate(model, val_pairs, val_args, process_group):
    from . import metrics
    kw = dict(val_args or {})
    if process_group is not None:
        kw.setdefault("process_group", process_group)
    res = metrics.evaluate(model, val_pairs, **kw)
    return res[0] if isinstance(res, list) else res


def _snapshot(model, trainer, out_dir, epoch, done, sched_args):
    name = f"epoch_{epoch}.pth"
    torch.save({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, os.path.join(out_dir, name))
    torch.save({"trainer": trainer.state_dict(), "epoch": int(epoch), "epochs_done": int(done), "schedule": dict(sched_args),
                "weights": name}, os.path.join(out_dir, f"epoch_{epoch}.train.pt"))
    if trainer.ema_decay is not None:
        torch.save(trainer.ema_state_dict(), os.path.join(out_dir, f"epoch_{epoch}.ema.pth"))
