"""Cost of on-device BRISQUE (metrics.brisque) beside NIQE (metrics.niqe, the yardstick) on the same images in the same run, at
400 x 600 and 1728 x 2304, batch 1 and 8: microseconds per image of the whole score, of the features alone and -- from HIP
events around each staged call -- of the stages.  BrisqueParams.random() stands in for the user's model (774 support vectors,
the size of the published one, unless --sv says otherwise).  One JSON line per measurement.

    python tools/bench_brisque.py --params tests/golden/niqe_pris_params.npz [--images 8] [--reps 5] [--sv 774]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/bench_brisque.py --params ... --profile
      (then: python tools/bench_brisque.py --share OUT/.../run_kernel_stats.csv -> the BRISQUE kernels' share of GPU time)
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BRISQUE_KERNELS = ("brisque_gray_kernel", "brisque_gauss_kernel", "brisque_resample_kernel", "brisque_tile_kernel", "brisque_fit_kernel",
                   "brisque_svr_kernel")
SIZES = ((400, 600), (1728, 2304))


def _share(path):
    tot = met = 0.0
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            ns = float(r["TotalDurationNs"])
            tot += ns
            if any(k in r["Name"] for k in BRISQUE_KERNELS):
                met += ns
                rows[r["Name"][:90]] = {"calls": int(r["Calls"]), "total_us": ns / 1e3, "avg_us": float(r["AverageNs"]) / 1e3}
    print(json.dumps({"kernel_time_total_ms": tot / 1e6, "brisque_kernels_ms": met / 1e6, "brisque_share": met / tot if tot else 0.0,
                      "brisque_kernels": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", required=True, help="the reference's niqe_pris_params.npz (for the NIQE yardstick)")
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sv", type=int, default=774, help="support vectors of the stand-in model")
    ap.add_argument("--profile", action="store_true", help="one pass of brisque() at both sizes, batch 1 (for rocprofv3)")
    ap.add_argument("--share", default=None, help="kernel_stats.csv of a rocprofv3 run of this tool")
    a = ap.parse_args()
    if a.share:
        _share(a.share)
        return
    import torch
    from hvi_cidnet_amd import metrics as M
    dev = torch.device("cuda:0")
    prm = M.load_niqe_params(a.params)
    bp = M.BrisqueParams.random(0, n_sv=a.sv)
    g = torch.Generator(device=dev).manual_seed(1)

    def timed(fn):
        fn()                                                     # warm-up (allocator, uploaded parameters)
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        return best

    def event_us(fn):
        fn()
        best = float("inf")
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1e3)
        return best

    for H, W in SIZES:
        q = torch.randint(0, 256, (a.images, 3, H, W), device=dev, generator=g, dtype=torch.uint8)
        if a.profile:
            M.brisque(q[:1], bp)
            torch.cuda.synchronize()
            continue
        for bs in (1, 8):
            if bs > a.images:
                continue
            for what, fn in (("niqe", lambda x: M.niqe(x, prm)), ("niqe_features_device_only", lambda x: M.niqe_features(x, prm)),
                             ("brisque", lambda x: M.brisque(x, bp)), ("brisque_features", M.brisque_features)):
                def run():
                    for i in range(0, a.images, bs):
                        fn(q[i:i + bs])
                t = timed(run)
                print(json.dumps({"what": what, "size": [H, W], "batch_size": bs, "images": a.images, "us_per_image": 1e6 * t / a.images}))
        x = q[:1]
        y = M.brisque_gray(x)
        y2 = M.brisque_half(y)
        _, mom = M.brisque_mscn(y)
        f = M.brisque_features(x)
        stages = {"gray": lambda: M.brisque_gray(x), "half": lambda: M.brisque_half(y), "tile_scale1_with_map": lambda: M.brisque_mscn(x),
                  "tile_scale2_with_map": lambda: M.brisque_mscn(y2), "fit_one_scale": lambda: M.brisque_fit(mom),
                  "svr": lambda: M.brisque_score(f, bp), "features": lambda: M.brisque_features(x),
                  "niqe_features": lambda: M.niqe_features(x, prm)}
        print(json.dumps({"what": "stages_event_us_batch1", "size": [H, W], "sv": a.sv, **{k: event_us(v) for k, v in stages.items()}}))


if __name__ == "__main__":
    main()
