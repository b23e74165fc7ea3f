"""Cost of on-device CIEDE2000 (csrc/ciede2000.hip) at 400 x 600 and 1024 x 1024, batch 1 and 8, on uniformly random image
pairs (every pixel pays the full formula whatever its colour; the GT-mean variant adds three fp64 pow per pixel).  Timed with
device events over --launches back-to-back calls, best of --reps:
  "plain_kernels" / "gt_mean_kernels": cidnet_metric_ciede2000_u8 called directly on pre-allocated outputs and workspace, the
      mean alone (the pixel launch and the finish launch: the code under test); gt_mean with a scale formed beforehand;
  "map_kernels": the same with the per-pixel map written as well (8 bytes per pixel);
  "both": the plain call, the scale (cidnet_metric_gt_mean_scale) and the GT-mean call through the Python wrappers, allocations
      included -- evaluate(ciede2000=True)'s share of a batch, were the scale not shared with the batch's other metrics;
  "psnr_ssim": the yardstick, metrics.psnr_ssim on the same images (not the code under test).
Each line also carries host_us_per_call, the host's time to enqueue one call: where it is close to us_per_call the device waits
for the host and the figure is an enqueue cost, not kernel time.  One JSON line per measurement.

    python tools/bench_ciede2000.py [--launches 100] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1, 400, 600), (8, 400, 600), (1, 1024, 1024), (8, 1024, 1024))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    from hvi_cidnet_amd import _lib, ops
    from hvi_cidnet_amd import metrics as M
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    L = _lib.lib()

    def timed(fn):
        """best of --reps, per call, in microseconds -> (device time between events around --launches back-to-back calls,
        host time to enqueue them)"""
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        best, host = float("inf"), float("inf")
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            for _ in range(a.launches):
                fn()
            host = min(host, (time.perf_counter() - t0) * 1e6 / a.launches)
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1e3 / a.launches)
        return best, host

    for B, h, w in SHAPES:
        q = (torch.rand(B, 3, h, w, device=dev, generator=g) * 255).to(torch.uint8)
        gt = (torch.rand(B, 3, h, w, device=dev, generator=g) * 255).to(torch.uint8)
        table = M._ciede_tables_on(dev)
        nws = L.raw("cidnet_metric_ciede2000_ws_bytes")(B, h, w)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        mean = torch.empty(B, dtype=torch.float64, device=dev)
        dmap = torch.empty((B, h, w), dtype=torch.float64, device=dev)
        scale = M.gt_mean_scale(q, gt)

        def kernels(s, m):
            return lambda: L.call("cidnet_metric_ciede2000_u8", ops._p(q), ops._p(gt), ops._p(s), ops._p(table), ops._p(m), ops._p(mean),
                                  ops._p(ws), nws, B, h, w, ops._stream())
        cases = (("plain_kernels", kernels(None, None)), ("gt_mean_kernels", kernels(scale, None)), ("map_kernels", kernels(None, dmap)),
                 ("both", lambda: M._ciede_both(q, gt, M._gt_mean_scale(q, gt))), ("psnr_ssim", lambda: M.psnr_ssim(q, gt)))
        for what, fn in cases:
            us, host = timed(fn)
            print(json.dumps({"what": what, "shape": [B, h, w], "launches": a.launches, "us_per_call": us, "host_us_per_call": host,
                              "us_per_image": us / B, "ns_per_pixel": us * 1e3 / (B * h * w)}), flush=True)
        assert torch.equal(mean, M.ciede2000(q, gt))                     # the last direct call was a plain one


if __name__ == "__main__":
    main()
