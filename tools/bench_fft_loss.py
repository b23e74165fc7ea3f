"""Cost of the frequency-domain training loss (csrc/fft_loss.hip) at 8 x 3 x 256 x 256 and 8 x 3 x 400 x 600:
  * "term": FFTLoss forward + backward (both gradients) -- device time between events around --launches back-to-back calls,
    and the host's time to enqueue one (where the two are close the device waits for the host and the figure is an enqueue
    cost); also the forward alone, and the ABI's forward (with and without the signs) and backward entries on their own;
  * "torch.fft": for information only, the same loss composed from torch.fft.rfft2 + autograd on the device (hipFFT plans and
    ATen kernels): a yardstick for this tool, never a path of the package;
  * "step": the trainer's step (full-width CIDNet, batch 8 at 256 x 256, eager) with the base objective and with fft_weight
    > 0, alternated round by round in one visit, the best round of each;
  * "stage": each of the five launches alone -- row forward, column forward (|.| and signs), finish, column adjoint, row
    adjoint -- with its rate in TFLOP/s (2 flop per multiply-add of the product it forms).  The entry points launch them
    back to back, so a kernel's own time comes from a kernel trace, in a run of its own per case:
        rocprofv3 --kernel-trace --stats -d DIR -o fft0 --output-format csv -- python tools/bench_fft_loss.py --loop 0
        python tools/bench_fft_loss.py --stats DIR/.../fft0_kernel_stats.csv --case 0
One JSON line per measurement.

    python tools/bench_fft_loss.py [--launches 10] [--reps 3] [--steps 4] [--no-step] [--no-torch]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((8, 256, 256), (8, 400, 600))


# the five launches of a term by the kernel names a trace shows (dft_gemm_kernel<how B is read, epilogue>)
KERNELS = (("row forward", "dft_gemm_kernel<0, 0>"), ("column forward", "dft_gemm_kernel<2, 1>"), ("finish", "fft_loss_finish_kernel"),
           ("column adjoint", "dft_gemm_kernel<3, 0>"), ("row adjoint", "dft_gemm_kernel<1, 2>"))


def gemm_flop(Pn, h, w):
    """2 flop per multiply-add of the four products for Pn planes of h x w"""
    Wh = w // 2 + 1
    row, col = 2.0 * Pn * h * w * 2 * Wh, 2.0 * Pn * h * 2 * h * 2 * Wh
    return {"row forward": row, "column forward": col, "column adjoint": col, "row adjoint": row}


def from_stats(path, case):
    """one "stage" line per launch from the kernel statistics of a traced --loop run"""
    import csv
    B, h, w = CASES[case]
    flop = gemm_flop(B * 3, h, w)
    rows = list(csv.DictReader(open(path)))
    total = 0.0
    for stage, key in KERNELS:
        hit = [r for r in rows if key in r["Name"]]
        if len(hit) != 1:
            raise SystemExit(f"{path}: {len(hit)} kernels match {key!r}")
        us = float(hit[0]["AverageNs"]) / 1e3
        total += us
        rec = {"what": "stage", "stage": stage, "shape": [B * 3, h, w], "calls": int(hit[0]["Calls"]), "us_per_call": us}
        if stage in flop:
            rec.update(gflop=flop[stage] / 1e9, tflops=flop[stage] / us / 1e6)
        print(json.dumps(rec), flush=True)
    print(json.dumps({"what": "stage", "stage": "sum of the five", "shape": [B * 3, h, w], "us_per_call": total}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true", help="leave out the trainer's step")
    ap.add_argument("--no-torch", action="store_true", help="leave out the torch.fft composition")
    ap.add_argument("--loop", type=int, default=None, metavar="CASE", help="only run the term --launches times at CASES[CASE] (to be traced)")
    ap.add_argument("--stats", default=None, metavar="CSV", help="print the stage lines from the kernel statistics of a traced --loop run")
    ap.add_argument("--case", type=int, default=0, help="the case --stats belongs to")
    a = ap.parse_args()
    if a.stats:
        return from_stats(a.stats, a.case)
    import torch
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import ops
    from hvi_cidnet_amd._lib import lib
    from hvi_cidnet_amd.dp import DataParallelTrainer
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    L = lib()

    def timed(fn, launches):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        best, host = float("inf"), float("inf")
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            for _ in range(launches):
                fn()
            host = min(host, (time.perf_counter() - t0) * 1e6 / launches)
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1e3 / launches)
        return best, host

    def images(B, h, w):
        xx = torch.linspace(0, 1, w, device=dev).view(1, 1, 1, w)
        gt = (0.6 * xx + 0.4 * torch.rand(B, 3, h, w, device=dev, generator=g)).clamp(0, 1)
        x = (gt * 0.8 + 0.05 * torch.randn(B, 3, h, w, device=dev, generator=g)).clamp(0, 1)
        return x, gt

    def entry(name, shape, fn, flop):
        us, _ = timed(fn, a.launches)
        print(json.dumps({"what": "entry", "entry": name, "shape": list(shape), "us_per_call": us, "gflop": flop / 1e9,
                          "tflops": flop / us / 1e6}), flush=True)

    if a.loop is not None:
        B, h, w = CASES[a.loop]
        x, gt = images(B, h, w)
        for _ in range(a.launches + 2):
            xr, gr = x.detach().requires_grad_(True), gt.detach().requires_grad_(True)
            P.FFTLoss()(xr, gr).backward()
        torch.cuda.synchronize()
        return
    for B, h, w in CASES:
        x, gt = images(B, h, w)
        loss_fn = P.FFTLoss()

        def term():
            xr, gr = x.detach().requires_grad_(True), gt.detach().requires_grad_(True)
            loss_fn(xr, gr).backward()

        def fwd():
            with torch.no_grad():
                loss_fn(x, gt)
        us, host = timed(term, a.launches)
        usf, hostf = timed(fwd, a.launches)
        print(json.dumps({"what": "term", "shape": [B, h, w], "launches": a.launches, "us_fwd_bwd": us, "host_us_fwd_bwd": host,
                          "us_fwd": usf, "host_us_fwd": hostf, "us_per_image": us / B}), flush=True)
        # the ABI's entries on their own, on the tensors of a real pass
        Pn, Wh = B * 3, w // 2 + 1
        th, tw = ops.dft_table(h, h, dev), ops.dft_table(w, Wh, dev)
        n = int(L.raw("cidnet_fft_loss_ws_floats")(Pn, h, w))
        ws = torch.empty(n, device=dev)
        S = torch.empty((Pn, h, Wh, 2), device=dev)
        loss = torch.empty((), device=dev)
        one = torch.ones(1, device=dev)
        ga, gb = torch.empty_like(x), torch.empty_like(x)
        f1, st, p = ctypes.c_float(1.0), ops._stream, ops._p
        flop = sum(gemm_flop(Pn, h, w)[k] for k in ("row forward", "column forward"))
        entry("loss forward, no signs", (Pn, h, w), lambda: L.call(
            "cidnet_fft_loss_fwd", p(x), p(gt), p(th), p(tw), f1, 0, p(loss), None, p(ws), n, Pn, h, w, st()), flop)
        entry("loss forward with signs", (Pn, h, w), lambda: L.call(
            "cidnet_fft_loss_fwd", p(x), p(gt), p(th), p(tw), f1, 0, p(loss), p(S), p(ws), n, Pn, h, w, st()), flop)
        entry("loss backward, ga and gb", (Pn, h, w), lambda: L.call(
            "cidnet_fft_loss_bwd", p(S), p(th), p(tw), p(one), f1, 0, p(ga), p(gb), p(ws), n, Pn, h, w, st()), flop)
        if not a.no_torch:
            def torch_term():
                xr, gr = x.detach().requires_grad_(True), gt.detach().requires_grad_(True)
                fa, fb = torch.fft.rfft2(xr), torch.fft.rfft2(gr)
                torch.nn.functional.l1_loss(torch.view_as_real(fa), torch.view_as_real(fb)).backward()
            try:
                ust, hostt = timed(torch_term, a.launches)
                print(json.dumps({"what": "torch.fft", "shape": [B, h, w], "us_fwd_bwd": ust, "host_us_fwd_bwd": hostt,
                                  "ours_over_torch": us / ust}), flush=True)
            except RuntimeError as e:                      # a build without hipFFT: say so, it is information only
                print(json.dumps({"what": "torch.fft", "shape": [B, h, w], "error": str(e)[:200]}), flush=True)

    if a.no_step:
        return
    B, h, w = CASES[0]
    x, gt = images(B, h, w)
    trainers = []
    for name, kw in (("base", {}), ("fft", {"fft_weight": 0.1})):
        torch.manual_seed(0)
        model = P.CIDNet().to(dev)
        tr = DataParallelTrainer(model, lr=1e-4, loss_fn=P.CIDNetLoss(model, **kw).to(dev))
        for _ in range(2):
            tr.step(x, gt)
        torch.cuda.synchronize()
        trainers.append((name, tr))
    best = {name: float("inf") for name, _ in trainers}
    for _ in range(a.reps):
        for name, tr in trainers:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr.step(x, gt)
            torch.cuda.synchronize()
            best[name] = min(best[name], (time.perf_counter() - t0) * 1e3 / a.steps)
    for name, _ in trainers:
        print(json.dumps({"what": "step", "objective": name, "shape": [B, h, w], "steps": a.steps, "reps": a.reps,
                          "ms_per_step": best[name], "img_per_s": B / best[name] * 1e3,
                          "ms_over_base": best[name] - best["base"]}), flush=True)


if __name__ == "__main__":
    main()
