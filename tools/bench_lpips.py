"""Cost of on-device LPIPS (csrc/lpips.hip) with LpipsParams.random() (the arithmetic does not depend on the values):
  * "lpips": metrics.lpips per pair at 400 x 600, batch 1 and 8, and at 1728 x 2304, batch 1, without and with the GT-mean
    rescale -- device time between events around --launches back-to-back calls, and the host's time to enqueue one call
    (where the two are close the device waits for the host and the figure is an enqueue cost);
  * "stage": the same work at 400 x 600 split into its launches -- ingest, the five convolutions (with the rate of each in
    TFLOP/s), the two pools, the distance -- each timed alone on a batch of 2 B images (restored + ground truth);
  * "evaluate": wall time of metrics.evaluate over 16 pairs of 400 x 600 at batch size 1 and 8, with and without lpips=
    (--no-lpips times only the latter, and runs on a tree that has no LPIPS).
One JSON line per measurement.

    python tools/bench_lpips.py [--launches 20] [--reps 3] [--no-lpips] [--skip-large]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((1, 400, 600), (8, 400, 600), (1, 1728, 2304))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--no-lpips", action="store_true", help="time evaluate() without lpips= only")
    ap.add_argument("--skip-large", action="store_true", help="leave out 1728 x 2304")
    a = ap.parse_args()
    import torch
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import ops
    from hvi_cidnet_amd import metrics as M
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)

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
        xx = torch.linspace(0, 255, w, device=dev).view(1, 1, 1, w)
        gt = (0.6 * xx + 0.4 * 255 * torch.rand(B, 3, h, w, device=dev, generator=g)).clamp(0, 255).to(torch.uint8)
        q = (gt.float() * 0.8 + 12 * torch.randn(B, 3, h, w, device=dev, generator=g)).clamp(0, 255).to(torch.uint8)
        return q, gt

    if not a.no_lpips:
        prm = P.LpipsParams.random()
        for B, h, w in CASES:
            if a.skip_large and h > 1000:
                continue
            q, gt = images(B, h, w)
            for gm in (False, True):
                us, host = timed(lambda: M.lpips(q, gt, prm, gt_mean=gm), a.launches)
                print(json.dumps({"what": "lpips", "shape": [B, h, w], "gt_mean": gm, "launches": a.launches, "us_per_call": us,
                                  "host_us_per_call": host, "us_per_pair": us / B}), flush=True)
        for B in (1, 8):
            h, w = 400, 600
            q, gt = images(B, h, w)
            N = 2 * B
            both = torch.cat([q, gt])
            L = M.lib()
            weights, biases, heads = prm.on(dev)
            x = torch.empty((N, 3, h, w), dtype=torch.float32, device=dev)
            us, _ = timed(lambda: L.call("cidnet_metric_lpips_ingest", ops._p(both), None, ops._p(x), N, h, w, ops._stream()), a.launches)
            print(json.dumps({"what": "stage", "stage": "ingest", "images": N, "shape": [h, w], "us_per_call": us}), flush=True)
            H, W = h, w
            for l, (_, m, c, k, stride, pad, pooled) in enumerate(M.LPIPS_LAYERS):
                if pooled:
                    Hp, Wp = (H - 3) // 2 + 1, (W - 3) // 2 + 1
                    y = torch.empty((N, c, Hp, Wp), dtype=torch.float32, device=dev)
                    us, _ = timed(lambda: L.call("cidnet_lpips_maxpool3s2", ops._p(x), ops._p(y), N * c, H, W, ops._stream()), a.launches)
                    print(json.dumps({"what": "stage", "stage": f"pool before conv {l}", "images": N, "in": [c, H, W],
                                      "us_per_call": us}), flush=True)
                    x, H, W = y, Hp, Wp
                Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
                y = torch.empty((N, m, Ho, Wo), dtype=torch.float32, device=dev)
                us, _ = timed(lambda: L.call("cidnet_lpips_conv_relu", ops._p(x), ops._p(weights[l]), ops._p(biases[l]), ops._p(y), N,
                                             m, c, H, W, k, stride, pad, ops._stream()), a.launches)
                flop = 2.0 * N * m * c * k * k * Ho * Wo
                print(json.dumps({"what": "stage", "stage": f"conv {l}", "images": N, "M": m, "K": c * k * k, "pixels": Ho * Wo,
                                  "us_per_call": us, "gflop": flop / 1e9, "tflops": flop / us / 1e6}), flush=True)
                x, H, W = y, Ho, Wo
            f = M._lpips_extract([(q, None), (gt, None)], prm)
            us, host = timed(lambda: M._lpips_distance([t[:B] for t in f], [t[B:] for t in f], prm, h, w), a.launches)
            print(json.dumps({"what": "stage", "stage": "distance (5 layer launches + finish)", "pairs": B, "us_per_call": us,
                              "host_us_per_call": host}), flush=True)

    # evaluate(): the full-width model with its initial weights, 16 pairs of 400 x 600
    torch.manual_seed(0)
    model = P.CIDNet().to(dev)
    pairs = []
    for i in range(a.pairs):
        q, gt = images(1, 400, 600)
        pairs.append((q[0].float().div(255).cpu(), gt[0].cpu()))
    variants = [("without", {})] if a.no_lpips else [("without", {}), ("with", {"lpips": P.LpipsParams.random()})]
    for bs in (1, 8):
        for name, kw in variants:
            P.evaluate(model, pairs[:bs], batch_size=bs, **kw)
            torch.cuda.synchronize()
            best = float("inf")
            for _ in range(a.reps):
                t0 = time.perf_counter()
                P.evaluate(model, pairs, batch_size=bs, **kw)
                best = min(best, time.perf_counter() - t0)
            print(json.dumps({"what": "evaluate", "lpips": name, "pairs": a.pairs, "shape": [400, 600], "batch_size": bs,
                              "wall_ms": best * 1e3, "wall_ms_per_pair": best * 1e3 / a.pairs}), flush=True)


if __name__ == "__main__":
    main()
