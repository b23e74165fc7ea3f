"""Cost of on-device evaluation (metrics.evaluate) at the LOL size, 400 x 600: img/s with batch_size 1 and 8 and with a
4-value alpha sweep, the forward alone for comparison, and the metric kernels alone (to_uint8 + PSNR / SSIM without and
with the GT-mean rescale).  One JSON line per measurement.

    python tools/bench_eval.py [--images 32] [--reps 3] [--gt_scale 0.64]
      (--gt_scale S != 1: the ground truths are round(400 S) x round(600 S) and the evaluations run with resize=True)
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/bench_eval.py --images 16 --reps 1
      (then: python tools/bench_eval.py --share OUT/.../run_kernel_stats.csv -> the metric kernels' share of GPU time)
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

METRIC_KERNELS = ("to_uint8_kernel", "gray_sum_kernel", "gt_mean_scale_kernel", "metric_tile_kernel", "metric_finish_kernel",
                  "resize_rows_kernel", "resize_cols_kernel")


def _share(path):
    tot = met = 0.0
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            ns = float(r["TotalDurationNs"])
            tot += ns
            if any(k in r["Name"] for k in METRIC_KERNELS):
                met += ns
                rows[r["Name"][:90]] = {"calls": int(r["Calls"]), "total_us": ns / 1e3, "avg_us": float(r["AverageNs"]) / 1e3}
    print(json.dumps({"kernel_time_total_ms": tot / 1e6, "metric_kernels_ms": met / 1e6, "metric_share": met / tot if tot else 0.0,
                      "metric_kernels": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gt_scale", type=float, default=1.0, help="size of the ground truths relative to the inputs")
    ap.add_argument("--share", default=None, help="kernel_stats.csv of a rocprofv3 run of this tool")
    a = ap.parse_args()
    if a.share:
        _share(a.share)
        return
    import torch
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import metrics as M
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = P.CIDNet().to(dev)
    H, W = 400, 600
    GH, GW = (H, W) if a.gt_scale == 1.0 else (max(11, round(H * a.gt_scale)), max(11, round(W * a.gt_scale)))
    resize = (GH, GW) != (H, W)
    g = torch.Generator(device=dev).manual_seed(1)
    pairs = []
    for _ in range(a.images):
        low = torch.rand(3, H, W, device=dev, generator=g) * 0.3
        gt = (torch.rand(3, GH, GW, device=dev, generator=g) * 255).to(torch.uint8)
        pairs.append((low, gt))

    def timed(fn):
        fn()                                                     # warm-up (allocator, prepared state)
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        return best

    for bs in (1, 8):
        t = timed(lambda: P.evaluate(model, pairs, gated=True, batch_size=bs, resize=resize))
        print(json.dumps({"what": "evaluate", "size": [H, W], "gt_size": [GH, GW], "batch_size": bs, "images": a.images, "s": t,
                          "img_per_s": a.images / t}))
    alphas = [0.80, 0.82, 0.84, 1.0]
    t = timed(lambda: P.evaluate(model, pairs, gated2=True, alpha=alphas, batch_size=8, resize=resize))
    print(json.dumps({"what": "evaluate_alpha_sweep", "alphas": alphas, "batch_size": 8, "images": a.images, "s": t,
                      "img_per_s": a.images / t, "img_alpha_per_s": a.images * len(alphas) / t}))

    x = torch.stack([p[0] for p in pairs[:8]])
    gt = torch.stack([p[1] for p in pairs[:8]])
    model.eval()
    with torch.no_grad():
        def fwd():
            for _ in range(4):
                model(x)
        t_fwd = timed(fwd) / 32
        out = model(x)

        def met():
            for _ in range(4):
                q = M.resize_u8(M.to_uint8(out, (H, W)), (GH, GW))
                M.psnr_ssim(q, gt, gt_mean=False)
                M.psnr_ssim(q, gt, gt_mean=True)
        t_met = timed(met) / 32
    model.train()
    print(json.dumps({"what": "per_image_at_bs8", "forward_ms": t_fwd * 1e3, "metrics_ms": t_met * 1e3,
                      "metrics_over_forward": t_met / t_fwd}))


if __name__ == "__main__":
    main()
