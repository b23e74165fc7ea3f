"""Cost of on-device LOE (csrc/loe.hip) at 8 x 400 x 600 and 1 x 1024 x 1024, for sample=50 and sample=None (every pixel), on a
natural-image-like pair (most samples near the histogram's diagonal: the contended case) and on a uniformly random one.  Two
timings per case, each with device events over --launches back-to-back calls: "loe_kernels", cidnet_metric_loe_u8 called
directly on pre-allocated outputs and workspace (the memset of the bins, the histogram launch, the finish launch: the code
under test), and "loe", the Python wrapper metrics.loe (the same plus three allocations and the argument checks).  Each line
also carries host_us_per_call, the host's time to enqueue one call: where it is close to us_per_call the device waits for the
host and the figure is an enqueue cost, not kernel time.  Yardsticks that are not the code under test: metrics.to_uint8 on the
same shapes, and metrics.niqe per image.  One JSON line per measurement.

    python tools/bench_loe.py [--params tests/golden/niqe_pris_params.npz] [--launches 200] [--reps 3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((8, 400, 600), (1, 1024, 1024))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", default=None, help="the reference's niqe_pris_params.npz (without it the NIQE yardstick is skipped)")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    from hvi_cidnet_amd import _lib, ops
    from hvi_cidnet_amd import metrics as M
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)

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
        yy = torch.linspace(0, 1, h, device=dev).view(1, 1, h, 1)
        xx = torch.linspace(0, 1, w, device=dev).view(1, 1, 1, w)
        scene = (0.25 + 0.2 * torch.sin(9 * xx) * torch.cos(7 * yy)).expand(B, 3, h, w) + 0.03 * torch.randn(B, 3, h, w, device=dev, generator=g)
        pairs = {"natural": (M.to_uint8(scene.contiguous()), M.to_uint8((scene.clamp(0, 1) ** 0.45).contiguous())),
                 "uniform": ((torch.rand(B, 3, h, w, device=dev, generator=g) * 255).to(torch.uint8),
                             (torch.rand(B, 3, h, w, device=dev, generator=g) * 255).to(torch.uint8))}
        for name, (lo, hi) in pairs.items():
            for sample in (50, None):
                step, rows, cols = M.loe_grid(h, w, sample)
                plan = (ctypes.c_int * 6)()
                _lib.lib().raw("cidnet_metric_loe_plan")(h, w, step, plan, 6)
                L = _lib.lib()
                nws = L.raw("cidnet_metric_loe_ws_bytes")(B)
                ws = torch.empty(nws, dtype=torch.uint8, device=dev)
                num = torch.empty(B, dtype=torch.int64, device=dev)
                val = torch.empty(B, dtype=torch.float64, device=dev)
                args = (ops._p(lo), ops._p(hi), B, h, w, step, ops._p(num), ops._p(val), ops._p(ws), nws, ops._stream())
                read = 6 * rows * cols * B
                for what, fn in (("loe_kernels", lambda: L.call("cidnet_metric_loe_u8", *args)), ("loe", lambda: M.loe(lo, hi, sample))):
                    us, host = timed(fn)
                    print(json.dumps({"what": what, "data": name, "shape": [B, h, w], "sample": sample, "step": step, "m": rows * cols,
                                      "blocks_per_image": plan[2], "samples_per_block": plan[3], "counter_bits": plan[4],
                                      "launches": a.launches, "us_per_call": us, "host_us_per_call": host, "us_per_image": us / B,
                                      "sample_bytes": read, "histogram_bytes": B * 65536 * 4}), flush=True)
                assert torch.equal(val, M.loe(lo, hi, sample))
        x = scene.contiguous()
        us, host = timed(lambda: M.to_uint8(x))
        print(json.dumps({"what": "to_uint8", "shape": [B, h, w], "launches": a.launches, "us_per_call": us, "host_us_per_call": host,
                          "us_per_image": us / B, "bytes": 15 * B * h * w}), flush=True)
        if a.params:
            prm = M.load_niqe_params(a.params)
            q = pairs["natural"][1]
            us, host = timed(lambda: M.niqe(q, prm))
            print(json.dumps({"what": "niqe", "shape": [B, h, w], "launches": a.launches, "us_per_call": us, "host_us_per_call": host,
                              "us_per_image": us / B}), flush=True)


if __name__ == "__main__":
    main()
