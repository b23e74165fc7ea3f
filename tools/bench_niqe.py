"""Cost of on-device NIQE (metrics.niqe, metrics.evaluate_unpaired) at 400 x 600 and 1024 x 1024, batch 1 and 8: NIQE-only
img/s (features on the device + the 36 x 36 tail on the host), evaluate_unpaired img/s with the full-width model, the
forward and the NIQE feature kernels per image, and -- as the stand-in for the reference's CPU script, which needs cv2 --
the time of the numpy restatement tests/niqe_ref.py on the same sizes.  One JSON line per measurement.

    python tools/bench_niqe.py --params tests/golden/niqe_pris_params.npz [--images 16] [--reps 3] [--cpu]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/bench_niqe.py --params ... --profile
      (then: python tools/bench_niqe.py --share OUT/.../run_kernel_stats.csv -> the NIQE kernels' share of GPU time)
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NIQE_KERNELS = ("niqe_luma_kernel", "niqe_half_rows_kernel", "niqe_half_cols_kernel", "niqe_block_kernel", "niqe_fit_kernel")
SIZES = ((400, 600), (1024, 1024))


def _share(path):
    tot = met = 0.0
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            ns = float(r["TotalDurationNs"])
            tot += ns
            if any(k in r["Name"] for k in NIQE_KERNELS + ("to_uint8_kernel",)):
                met += ns
                rows[r["Name"][:90]] = {"calls": int(r["Calls"]), "total_us": ns / 1e3, "avg_us": float(r["AverageNs"]) / 1e3}
    print(json.dumps({"kernel_time_total_ms": tot / 1e6, "niqe_kernels_ms": met / 1e6, "niqe_share": met / tot if tot else 0.0,
                      "niqe_over_rest": met / (tot - met) if tot > met else 0.0, "niqe_kernels": rows}))


def _cpu(a):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import niqe_ref as R
    with np.load(a.params) as z:
        mu, cov, win = z["mu_pris_param"], z["cov_pris_param"], z["gaussian_window"]
    rng = np.random.default_rng(0)
    for h, w in SIZES:
        img = np.clip(rng.normal(120, 40, (3, h, w)), 0, 255).astype(np.uint8)
        R.niqe(img, mu, cov, win)
        t0 = time.perf_counter()
        R.niqe(img, mu, cov, win)
        t = time.perf_counter() - t0
        print(json.dumps({"what": "niqe_ref_numpy_cpu", "size": [h, w], "threads": os.environ.get("OMP_NUM_THREADS"), "s_per_image": t}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", required=True, help="the reference's niqe_pris_params.npz")
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu", action="store_true", help="also time tests/niqe_ref.py on the host")
    ap.add_argument("--profile", action="store_true", help="one evaluate_unpaired pass at 400 x 600, batch 8 (for rocprofv3)")
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
    prm = M.load_niqe_params(a.params)
    model = P.CIDNet().to(dev)
    g = torch.Generator(device=dev).manual_seed(1)

    def timed(fn):
        fn()                                                     # warm-up (allocator, tables, prepared state)
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        return best

    if a.profile:
        images = [torch.rand(3, 400, 600, device=dev, generator=g) * 0.3 for _ in range(a.images)]
        P.evaluate_unpaired(model, images, prm, batch_size=8)
        torch.cuda.synchronize()
        return
    for H, W in SIZES:
        images = [torch.rand(3, H, W, device=dev, generator=g) * 0.3 for _ in range(a.images)]
        q = (torch.rand(a.images, 3, H, W, device=dev, generator=g) * 255).to(torch.uint8)
        for bs in (1, 8):
            def only():
                for i in range(0, a.images, bs):
                    M.niqe(q[i:i + bs], prm)
            t = timed(only)
            print(json.dumps({"what": "niqe", "size": [H, W], "batch_size": bs, "images": a.images, "s": t, "img_per_s": a.images / t}))

            def feats():
                for i in range(0, a.images, bs):
                    M.niqe_features(q[i:i + bs], prm)
            t = timed(feats)
            print(json.dumps({"what": "niqe_features_device_only", "size": [H, W], "batch_size": bs, "images": a.images, "s": t,
                              "img_per_s": a.images / t, "ms_per_image": 1e3 * t / a.images}))
            t = timed(lambda: P.evaluate_unpaired(model, images, prm, batch_size=bs))
            print(json.dumps({"what": "evaluate_unpaired", "size": [H, W], "batch_size": bs, "images": a.images, "s": t,
                              "img_per_s": a.images / t}))
        x = torch.stack(images[:8])
        model.eval()
        with torch.no_grad():
            t_fwd = timed(lambda: model(x)) / 8
        model.train()
        print(json.dumps({"what": "forward_per_image_at_bs8", "size": [H, W], "ms": t_fwd * 1e3}))
    if a.cpu:
        _cpu(a)


if __name__ == "__main__":
    main()
