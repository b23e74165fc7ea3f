"""Cost of the self-ensemble kernels (csrc/ensemble.hip) beside the 8 forwards they surround, at 3 x 400 x 600 with B = 8 and at
3 x 1024 x 1024 with B = 4.  One JSON line per measurement.

    python tools/bench_ensemble.py [--iters 100] [--forward_iters 3] [--no_forward]

views A = ensemble_views(x, 0, 4), views B = ensemble_views(x, 4, 4) (through LDS), merge = ensemble_merge(ya, yb) with four
views in each group.  bytes = the algorithmic count, one read and one write per view element: 2 * 4 * B C H W * 4 for either
views call (the kernel itself reads x once for the four views: `bytes_moved` counts that, 5 B C H W * 4) and (8 + 1) B C H W *
4 for the merge.  The rates are over device-event time; the share is against the 6.29 TB/s a float4 copy reaches.  The
operands of the smaller shape fit the last-level cache between two calls, so its rates are not memory rates: each timed call
therefore works on its own copy of the operands, `--copies` of them used in turn (default: enough for 1 GiB)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_BYTES_PER_S = 6.29e12
SHAPES = ((8, 3, 400, 600), (4, 3, 1024, 1024))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--forward_iters", type=int, default=3)
    ap.add_argument("--copies", type=int, default=0, help="operand sets used in turn (0: enough for 1 GiB of them)")
    ap.add_argument("--no_forward", action="store_true", help="time the kernels only")
    a = ap.parse_args(argv)
    import torch
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import image_io as IO
    assert torch.cuda.is_available(), "bench_ensemble.py needs a GPU"
    dev = torch.device("cuda:0")

    def timed(fn, iters):
        for i in range(min(10, iters)):
            fn(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / iters

    model = None
    if not a.no_forward:
        torch.manual_seed(0)
        model = P.CIDNet().to(dev).eval()
    for B, C, H, W in SHAPES:
        n = B * C * H * W * 4                                    # bytes of one view of the batch
        copies = a.copies or max(2, -(-(1 << 30) // (9 * n)))
        xs = [torch.rand((B, C, H, W), device=dev) for _ in range(copies)]
        yas = [IO.ensemble_views(x, 0, 4) for x in xs]
        ybs = [IO.ensemble_views(x, 4, 4) for x in xs]
        xi = (xs[0] * 1024).round()                              # integer-valued: the sum of its 8 views is exact
        assert torch.equal(IO.ensemble_merge(IO.ensemble_views(xi, 0, 4), IO.ensemble_views(xi, 4, 4)), xi)
        del xi
        runs = (("views_a", lambda i: IO.ensemble_views(xs[i % copies], 0, 4), 8 * n, 5 * n),
                ("views_b", lambda i: IO.ensemble_views(xs[i % copies], 4, 4), 8 * n, 5 * n),
                ("merge", lambda i: IO.ensemble_merge(yas[i % copies], ybs[i % copies]), 9 * n, 9 * n),
                ("merge_a_only", lambda i: IO.ensemble_merge(yas[i % copies]), 5 * n, 5 * n))
        for what, fn, nbytes, moved in runs:
            t = timed(fn, a.iters)
            print(json.dumps({"what": what, "shape": [B, C, H, W], "copies": copies, "us": t * 1e6, "bytes": nbytes,
                              "bytes_per_s": nbytes / t, "share_of_hbm_copy": nbytes / t / HBM_COPY_BYTES_PER_S,
                              "bytes_moved": moved, "moved_per_s": moved / t,
                              "moved_share_of_hbm_copy": moved / t / HBM_COPY_BYTES_PER_S}), flush=True)
        if model is None:
            continue
        del yas, ybs
        with torch.no_grad():
            x = xs[0]
            t_fwd = timed(lambda i: (model(IO.ensemble_views(x, 0, 4)), model(IO.ensemble_views(x, 4, 4))), a.forward_iters)
            t_all = timed(lambda i: IO._ensemble(model, x, 4, 4), a.forward_iters)
            t_one = timed(lambda i: model(x), a.forward_iters)
        print(json.dumps({"what": "forwards", "shape": [B, C, H, W], "us_8_views_with_their_kernels": t_fwd * 1e6,
                          "us_views_forwards_merge": t_all * 1e6, "us_one_forward_of_the_batch": t_one * 1e6}), flush=True)


if __name__ == "__main__":
    main()
