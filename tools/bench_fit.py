"""Cost of the guarded step and of the run driver (hvi_cidnet_amd.fit) at B = 8, 400 x 600, full-width model.  One JSON line
per measurement:

  step           ms per step, guard off against guard on (clip + skip + step log), alternated three times, --steps steps per
                 timing, host clock around work that ends in a device synchronise
  epoch          one epoch of run_epoch (the step log read once at the end) against the same epoch with loss.item() after
                 every step (the reference's way, train.py:75), alternated three times, over a synthetic resident set
  accum_ema      --accum K and / or --ema DECAY: ms per pass of the guarded step with accum_steps=K / ema_decay=DECAY against
                 the guarded step without them, alternated three times (nothing else is measured in such a run)
  diagnose       --diagnose: ms per step of the guarded step with the per-tensor log (dp.TensorLog, gradient and weights: four
                 more launches per update) against the guarded step without it, alternated three times (nothing else is
                 measured in such a run); with --trace-run a few steps of both for a rocprofv3 run
  kernels        --share PATH: time per launch of the guard's kernels from the kernel_stats.csv of a run under
                 rocprofv3 --kernel-trace --stats (a run of its own: --trace-run launches only a few guarded steps)

Every line is printed and appended to --out (default profiles/fit_<precision>.jsonl; --share: profiles/fit_kernels.jsonl).

    python tools/bench_fit.py [--precision f32|bf16] [--steps 20] [--pairs 64] [--out FILE]
    python tools/bench_fit.py [--precision f32|bf16] [--steps 20] --accum 4 --ema 0.999
    python tools/bench_fit.py [--precision f32|bf16] [--steps 20] --diagnose
    rocprofv3 --kernel-trace --stats -f csv -d OUT -o run -- python tools/bench_fit.py --trace-run
    python tools/bench_fit.py --share OUT/.../run_kernel_stats.csv
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, B = 400, 600, 8
GUARD_KERNELS = ("sumsq_kernel", "guard_finish_kernel", "adam_dev_kernel", "adam_kernel", "stats_tile_kernel", "stats_finish_kernel")


_OUT = None


def emit(row):
    line = json.dumps(row)
    print(line)
    if _OUT is not None:
        os.makedirs(os.path.dirname(os.path.abspath(_OUT)), exist_ok=True)
        with open(_OUT, "a") as f:
            f.write(line + "\n")


def _share(path):
    with open(path) as f:
        for r in csv.DictReader(f):
            for k in GUARD_KERNELS:
                if "cidnet::" in r["Name"] and k in r["Name"]:
                    emit({"what": "kernels", "kernel": k, "calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3,
                          "min_us": float(r.get("MinNs", "nan")) / 1e3, "max_us": float(r.get("MaxNs", "nan")) / 1e3})


def _resident(dev, n):
    import torch
    from hvi_cidnet_amd import ResidentPairs
    g = torch.Generator().manual_seed(0)
    distinct = [torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g) for _ in range(16)]
    return ResidentPairs([distinct[i % 16] for i in range(n)], [distinct[(i + 5) % 16] for i in range(n)], dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f32", choices=["f32", "bf16"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=64, help="size of the synthetic resident set (an epoch has pairs / 8 steps)")
    ap.add_argument("--trace-run", action="store_true", help="a few guarded steps only (for a rocprofv3 run)")
    ap.add_argument("--share", default=None, help="kernel_stats.csv of a rocprofv3 run of this tool with --trace-run")
    ap.add_argument("--accum", type=int, default=1, help="K: time the guarded step with accum_steps=K against the plain one")
    ap.add_argument("--ema", type=float, default=None, help="DECAY: time the guarded step with ema_decay=DECAY against the plain one")
    ap.add_argument("--diagnose", action="store_true", help="time the guarded step with a TensorLog against the plain one")
    ap.add_argument("--out", default=None, help="file the JSON lines are appended to")
    a = ap.parse_args()
    global _OUT
    _OUT = a.out or os.path.join(ROOT, "profiles", "fit_kernels.jsonl" if a.share is not None else f"fit_{a.precision}.jsonl")
    if a.share is not None:
        _share(a.share)
        return
    import torch
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd.dp import DataParallelTrainer
    if not torch.cuda.is_available():
        raise SystemExit("bench_fit needs a GPU")
    dev = torch.device("cuda:0")
    P.set_precision(a.precision)
    torch.manual_seed(0)
    x0, gt0 = torch.rand((B, 3, H, W), device=dev), torch.rand((B, 3, H, W), device=dev)

    def trainer(guard, capacity=64):
        torch.manual_seed(0)
        kw = dict(max_grad_norm=1.0, skip_nonfinite=True, step_log=P.StepLog(capacity)) if guard else {}
        return DataParallelTrainer(P.CIDNet().to(dev), lr=1e-4, **kw)

    if a.accum > 1 or a.ema is not None:
        # the guarded step without and with accumulation / the average, alternated; ms per PASS (one B = 8 batch), so the two
        # compare directly: with --accum K a timing runs steps - steps % K passes, i.e. whole updates
        torch.manual_seed(0)
        plain = trainer(True)
        torch.manual_seed(0)
        feat = DataParallelTrainer(P.CIDNet().to(dev), lr=1e-4, max_grad_norm=1.0, skip_nonfinite=True,
                                   step_log=P.StepLog(64), accum_steps=a.accum, ema_decay=a.ema)
        passes = max(a.accum, a.steps - a.steps % a.accum)
        pair = {"plain": plain, "feature": feat}
        for tr in pair.values():
            for _ in range(2 * a.accum if a.accum > 1 else 5):
                tr.step(x0, gt0)
        torch.cuda.synchronize()
        for rep in range(3):
            for name, tr in pair.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(passes):
                    tr.step(x0, gt0)
                torch.cuda.synchronize()
                t = time.perf_counter() - t0
                emit({"what": "accum_ema", "precision": a.precision, "mode": name, "accum": a.accum if name == "feature" else 1,
                      "ema": a.ema if name == "feature" else None, "rep": rep, "passes": passes,
                      "ms_per_pass": t / passes * 1e3})
        return
    if a.diagnose:
        torch.manual_seed(0)
        feat = DataParallelTrainer(P.CIDNet().to(dev), lr=1e-4, max_grad_norm=1.0, skip_nonfinite=True,
                                   step_log=P.StepLog(64), tensor_log=P.TensorLog(64))
        pair = {"plain": trainer(True), "diagnose": feat}
        for tr in pair.values():
            for _ in range(5):
                tr.step(x0, gt0)
        torch.cuda.synchronize()
        for rep in range(1 if a.trace_run else 3):
            for name, tr in pair.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    tr.step(x0, gt0)
                torch.cuda.synchronize()
                t = time.perf_counter() - t0
                if not a.trace_run:
                    emit({"what": "diagnose", "precision": a.precision, "mode": name, "rep": rep, "steps": a.steps,
                          "ms_per_step": t / a.steps * 1e3})
        return
    trainers = {"guard_off": trainer(False), "guard_on": trainer(True)}
    for tr in trainers.values():
        for _ in range(5):
            tr.step(x0, gt0)
    torch.cuda.synchronize()
    if a.trace_run:
        for _ in range(10):
            for tr in trainers.values():
                tr.step(x0, gt0)
        torch.cuda.synchronize()
        return
    for rep in range(3):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr.step(x0, gt0)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            emit({"what": "step", "precision": a.precision, "mode": name, "rep": rep, "steps": a.steps,
                  "ms_per_step": t / a.steps * 1e3})
    del trainers["guard_off"]

    # one epoch: the step log read once against loss.item() after every step
    tb = P.TrainBatches(_resident(dev, a.pairs), B, (H, W), seed=0, drop_last=True)
    tr = trainers["guard_on"]
    log = tr.step_log
    if log.capacity < len(tb):
        raise SystemExit(f"--pairs {a.pairs}: more than {log.capacity} steps per epoch")

    def with_log(e):
        return P.epoch_stats(P.run_epoch(tr, tb, e, log))["loss"]

    def with_item(e):
        log.reset()
        losses = [float(tr.step(x, gt).item()) for x, gt in tb.epoch(e)]
        return sum(losses) / len(losses)

    with_log(100)
    with_item(101)
    for rep in range(3):
        for name, fn in (("step_log", with_log), ("item_every_step", with_item)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = fn(rep)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            emit({"what": "epoch", "precision": a.precision, "mode": name, "rep": rep, "steps": len(tb),
                  "ms_per_step": t / len(tb) * 1e3, "loss": loss})


if __name__ == "__main__":
    main()
