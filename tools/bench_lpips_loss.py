"""Cost of the LPIPS training loss (csrc/lpips.hip forward, csrc/lpips_loss.hip backward) with LpipsParams.random() (the
arithmetic does not depend on the values), at 8 x 3 x 256 x 256 and 8 x 3 x 400 x 600:
  * "term": LPIPSLoss forward + backward -- device time between events around --launches back-to-back calls, and the host's
    time to enqueue one (where the two are close the device waits for the host and the figure is an enqueue cost);
  * "stage": the same work split into its launches, each timed alone on the tensors of a real pass: the two ingests, the
    extractor (convolutions with their rate in TFLOP/s, pools), the distance, then the backward chain in the order it runs;
  * "step": the trainer's step (full-width CIDNet, batch 8 at 256 x 256, eager) with the base objective, with lpips_weight > 0
    and with P_weight = 1e-2, alternated round by round in one visit, the best round of each.
One JSON line per measurement.

    python tools/bench_lpips_loss.py [--launches 10] [--reps 3] [--steps 4] [--no-step] [--no-vgg]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((8, 256, 256), (8, 400, 600))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true", help="leave out the trainer's step")
    ap.add_argument("--no-vgg", action="store_true", help="leave out the P_weight = 1e-2 step")
    a = ap.parse_args()
    import torch
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import ops
    from hvi_cidnet_amd import metrics as M
    from hvi_cidnet_amd.dp import DataParallelTrainer
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    L = M.lib()
    prm = P.LpipsParams.random()

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

    def stage(name, shape, fn, flop=None, **more):
        us, _ = timed(fn, a.launches)
        rec = {"what": "stage", "stage": name, "shape": list(shape), "us_per_call": us, **more}
        if flop is not None:
            rec.update(gflop=flop / 1e9, tflops=flop / us / 1e6)
        print(json.dumps(rec), flush=True)
        return us

    def new(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)

    for B, h, w in CASES:
        x, gt = images(B, h, w)
        loss_fn = P.LPIPSLoss(prm)

        def term():
            xr = x.detach().requires_grad_(True)
            loss_fn(xr, gt).backward()

        def fwd():
            with torch.no_grad():
                loss_fn(x, gt)
        us, host = timed(term, a.launches)
        usf, hostf = timed(fwd, a.launches)
        print(json.dumps({"what": "term", "shape": [B, h, w], "launches": a.launches, "us_fwd_bwd": us, "host_us_fwd_bwd": host,
                          "us_fwd": usf, "host_us_fwd": hostf, "us_per_image": us / B}), flush=True)
        # the launches one by one, on the tensors of a real pass
        weights, biases, heads = prm.on(dev)
        wts = prm.dgrad_on(dev)
        N, S = 2 * B, ops._stream
        z = new(N, 3, h, w)
        total = stage("ingest (x and gt)", (B, h, w), lambda: (L.call("cidnet_lpips_ingest_f32", ops._p(x), ops._p(z), B, h, w, S()),
                                                             L.call("cidnet_lpips_ingest_f32", ops._p(gt), ops._p(z[B:]), B, h, w, S())))
        taps, t, H, W = [], z, h, w
        for l, (_, m, c, k, stride, pad, pooled) in enumerate(M.LPIPS_LAYERS):
            if pooled:
                Hp, Wp = (H - 3) // 2 + 1, (W - 3) // 2 + 1
                y = new(N, c, Hp, Wp)
                total += stage(f"pool before conv {l}", (N, c, H, W),
                               lambda: L.call("cidnet_lpips_maxpool3s2", ops._p(t), ops._p(y), N * c, H, W, S()))
                t, H, W = y, Hp, Wp
            Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
            y = new(N, m, Ho, Wo)
            total += stage(f"conv {l}", (N, m, Ho, Wo), lambda: L.call("cidnet_lpips_conv_relu", ops._p(t), ops._p(weights[l]),
                                                                       ops._p(biases[l]), ops._p(y), N, m, c, H, W, k, stride, pad, S()),
                           flop=2.0 * N * m * c * k * k * Ho * Wo)
            taps.append(y)
            t, H, W = y, Ho, Wo
        n = L.raw("cidnet_lpips_loss_ws_floats")(B, h, w)
        ws, loss = new(n), new()

        def distance():
            for l, f in enumerate(taps):
                L.call("cidnet_metric_lpips_layer", ops._p(f), ops._p(f[B:]), ops._p(heads[l]), ops._p(ws), n, l, B, f.shape[1],
                       f.shape[2], f.shape[3], h, w, S())
            L.call("cidnet_lpips_loss_finish", ops._p(ws), n, ops._f(1.0), ops._p(loss), B, h, w, S())
        total += stage("distance (5 layer launches + finish)", (B, h, w), distance)

        def dist_grad(l, mask):
            f = taps[l]
            d = new(B, *f.shape[1:])
            us = stage(f"distance backward {l}", (B, *f.shape[1:]), lambda: L.call(
                "cidnet_lpips_layer_bwd", ops._p(f), ops._p(f[B:]), ops._p(heads[l]), ops._p(d), ops._f(1.0), mask, B, f.shape[1],
                f.shape[2] * f.shape[3], S()))
            return d, us
        d, us = dist_grad(4, 1)
        total += us
        for l in range(4, 0, -1):
            _, m, c, k, stride, pad, pooled = M.LPIPS_LAYERS[l]
            fh, fw = taps[l].shape[-2:]
            below = taps[l - 1]
            add, us = dist_grad(l - 1, 0)
            total += us
            dx = new(B, c, fh, fw)
            flop = 2.0 * B * m * c * k * k * fh * fw
            if pooled:
                total += stage(f"conv {l} data gradient", (B, c, fh, fw), lambda: L.call(
                    "cidnet_lpips_conv_dgrad", ops._p(d), ops._p(wts[l]), None, None, ops._p(dx), B, m, c, fh, fw, k, stride, pad, S()),
                    flop=flop)
                Hs, Ws = below.shape[-2:]
                dn = new(B, c, Hs, Ws)
                total += stage(f"pool backward + mask + add -> tap {l - 1}", (B, c, Hs, Ws), lambda: L.call(
                    "cidnet_lpips_maxpool3s2_bwd", ops._p(below), ops._p(dx), ops._p(add), ops._p(dn), B * c, Hs, Ws, S()))
                d = dn
            else:
                total += stage(f"conv {l} data gradient + mask + add", (B, c, fh, fw), lambda: L.call(
                    "cidnet_lpips_conv_dgrad", ops._p(d), ops._p(wts[l]), ops._p(below), ops._p(add), ops._p(dx), B, m, c, fh, fw, k,
                    stride, pad, S()), flop=flop)
                d = dx
        _, m, c, k, stride, pad, _ = M.LPIPS_LAYERS[0]
        dz, gx = new(B, 3, h, w), new(B, 3, h, w)
        fh, fw = taps[0].shape[-2:]
        total += stage("conv 0 data gradient (gather)", (B, 3, h, w), lambda: L.call(
            "cidnet_lpips_conv_dgrad", ops._p(d), ops._p(wts[0]), None, None, ops._p(dz), B, m, c, h, w, k, stride, pad, S()),
            flop=2.0 * B * m * c * k * k * fh * fw)
        total += stage("ingest backward", (B, 3, h, w), lambda: L.call("cidnet_lpips_ingest_f32_bwd", ops._p(dz), ops._p(gx), B, h, w, S()))
        print(json.dumps({"what": "stage", "stage": "sum of the stages", "shape": [B, h, w], "us_per_call": total}), flush=True)

    if a.no_step:
        return
    B, h, w = CASES[0]
    x, gt = images(B, h, w)
    variants = [("base", {}), ("lpips", {"lpips_weight": 1.0, "lpips_params": prm})]
    if not a.no_vgg:
        variants.append(("vgg", {"P_weight": 1e-2}))
    trainers = []
    for name, kw in variants:
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
