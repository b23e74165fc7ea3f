"""Cost of metrics.resize_u8 (csrc/resize.hip) at the sizes an evaluation meets: 400 x 600 -> 384 x 384 and 1024 x 1024 ->
400 x 600, per pass and for the whole call, beside PIL's CPU time for the same Image.resize.  One JSON line per measurement.

    python tools/bench_resize.py [--batch 1 8] [--iters 200]

A pass is timed alone by resizing one axis only (the other pass is then skipped, not run as an identity): the horizontal
pass is (h_in, w_in) -> (h_in, w_out), the vertical one (h_in, w_out) -> (h_out, w_out).  bytes = what a pass must move, its
input once and its output once; the rate is over device-event time, the share against the 6.29 TB/s a float4 copy reaches."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BYTES_PER_S = 6.29e12
SHAPES = (((400, 600), (384, 384)), ((1024, 1024), (400, 600)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from hvi_cidnet_amd import metrics as M
    assert torch.cuda.is_available(), "bench_resize.py needs a GPU"
    dev = torch.device("cuda:0")

    def timed(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / a.iters

    rng = np.random.default_rng(0)
    for (H, W), (h, w) in SHAPES:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        pil = Image.fromarray(img)
        t_pil = float("inf")
        for _ in range(5):
            t0 = time.perf_counter()
            ref = pil.resize((w, h))
            t_pil = min(t_pil, time.perf_counter() - t0)
        for B in a.batch:
            q = torch.from_numpy(img.transpose(2, 0, 1)).to(dev).unsqueeze(0).repeat(B, 1, 1, 1).contiguous()
            out = M.resize_u8(q, (h, w))
            assert np.array_equal(out[B - 1].cpu().numpy().transpose(1, 2, 0), np.array(ref)), "differs from PIL"
            mid = M.resize_u8(q, (H, w))
            passes = (("horizontal", q, (H, w), B * 3 * (H * W + H * w)), ("vertical", mid, (h, w), B * 3 * (H * w + h * w)),
                      ("both", q, (h, w), B * 3 * (H * W + 2 * H * w + h * w)))
            for what, src, size, nbytes in passes:
                t = timed(lambda: M.resize_u8(src, size))
                print(json.dumps({"what": what, "from": [H, W], "to": [h, w], "batch": B, "us": t * 1e6, "bytes": nbytes,
                                  "bytes_per_s": nbytes / t, "share_of_hbm_copy": nbytes / t / HBM_COPY_BYTES_PER_S,
                                  "pil_cpu_us_per_image": t_pil * 1e6 if what == "both" else None,
                                  "pil_over_device_per_image": t_pil / (t / B) if what == "both" else None}), flush=True)


if __name__ == "__main__":
    main()
