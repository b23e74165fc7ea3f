"""Cost of the on-device JPEG file round trip (metrics.jpeg_roundtrip_u8, evaluate_unpaired(file_roundtrip=True)) at 400 x 600
and 1024 x 1024, batch 1 and 8: device time per image between two events, the bytes the two launches must move over that time,
Pillow's encode + decode of the same images on a pool of host threads (what scoring the decoded file costs without the
kernels), evaluate_unpaired with and without the round trip on .jpg names with the full-width model, and the forward per image
for the kernels' share of it.  One JSON line per measurement.

    python tools/bench_jpeg.py --params tests/golden/niqe_pris_params.npz [--images 16] [--reps 5] [--threads 16]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/bench_jpeg.py --profile
      (then: python tools/bench_jpeg.py --share OUT/.../run_kernel_stats.csv -> each launch's time per image and bytes / s)
"""
import argparse
import concurrent.futures as cf
import csv
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((400, 600), (1024, 1024))
PROFILE_CALLS = 20


def _bytes(h, w):
    """(launch A, launch B) bytes per image that must cross HBM: RGB in and the decoded planes out; the planes in and RGB out"""
    H, W = -(-h // 16) * 16, -(-w // 16) * 16
    return 3 * h * w + H * W * 3 // 2, h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2) + 3 * h * w


def _share(path):
    h, w = SIZES[0]
    n = PROFILE_CALLS * 8
    for r in csv.DictReader(open(path)):
        for k, b in zip(("jpeg_codec_kernel", "jpeg_finish_kernel"), _bytes(h, w)):
            if k in r["Name"]:
                us = float(r["TotalDurationNs"]) / 1e3 / n
                print(json.dumps({"kernel": k, "size": [h, w], "batch_size": 8, "calls": int(r["Calls"]), "us_per_image": us,
                                  "bytes_per_image": b, "GB_per_s": b / us / 1e3}))


def _pil_roundtrip(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", quality=75)
    buf.seek(0)
    with Image.open(buf) as im:
        return im.convert("RGB").tobytes()


class _Named(list):
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", default=None, help="the reference's niqe_pris_params.npz (needed for evaluate_unpaired)")
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--profile", action="store_true", help=f"{PROFILE_CALLS} round trips of 8 images of 400 x 600 (for rocprofv3)")
    ap.add_argument("--share", default=None, help="kernel_stats.csv of a rocprofv3 run of this tool")
    a = ap.parse_args()
    if a.share:
        _share(a.share)
        return
    import torch
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib, metrics as M
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)

    def photo(n, h, w):
        """smooth structure plus grain: a byte image that compresses like one, uint8 (n,3,h,w) on the device"""
        yy = torch.linspace(0, 1, h, device=dev).view(1, 1, h, 1)
        xx = torch.linspace(0, 1, w, device=dev).view(1, 1, 1, w)
        c = torch.arange(3, device=dev).view(1, 3, 1, 1)
        base = 0.45 + 0.3 * torch.sin(9 * xx + c) * torch.cos(7 * yy - c)
        return ((base + 0.04 * torch.randn(n, 3, h, w, device=dev, generator=g)).clamp(0, 1) * 255).to(torch.uint8)

    if a.profile:
        q = photo(8, *SIZES[0])
        for _ in range(PROFILE_CALLS):
            M.jpeg_roundtrip_u8(q)
        torch.cuda.synchronize()
        return

    def device_ms(fn, calls):
        fn()
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / calls)
        return best

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        return best

    prm = M.load_niqe_params(a.params) if a.params else None
    model = P.CIDNet().to(dev)
    L = _lib.lib()
    qtab = torch.from_numpy(M.jpeg_quant_plan(75).device_table()).to(dev)
    for H, W in SIZES:
        q = photo(a.images, H, W)
        for bs in (1, 8):
            ms = device_ms(lambda: M.jpeg_roundtrip_u8(q[:bs]), 200) / bs
            ba, bb = _bytes(H, W)
            print(json.dumps({"what": "jpeg_roundtrip_u8_device", "size": [H, W], "batch_size": bs, "ms_per_image": ms,
                              "bytes_per_image": ba + bb, "GB_per_s": (ba + bb) / ms / 1e6}))
            # the C entry point on buffers allocated once: what the wrapper's allocations and argument handling add
            src, dst = q[:bs].contiguous(), torch.empty_like(q[:bs])
            nws = L.raw("cidnet_metric_jpeg_ws_bytes")(bs, H, W)
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            f, st = L.raw("cidnet_metric_jpeg_roundtrip_u8"), torch.cuda.current_stream().cuda_stream
            args = (src.data_ptr(), dst.data_ptr(), ws.data_ptr(), nws, qtab.data_ptr(), bs, H, W, st)
            ms = device_ms(lambda: f(*args), 200) / bs
            assert torch.equal(dst, M.jpeg_roundtrip_u8(src))
            print(json.dumps({"what": "cidnet_metric_jpeg_roundtrip_u8_device", "size": [H, W], "batch_size": bs,
                              "ms_per_image": ms, "GB_per_s": (ba + bb) / ms / 1e6}))
        host = [np_img for np_img in q.permute(0, 2, 3, 1).contiguous().cpu().numpy()]
        with cf.ThreadPoolExecutor(a.threads) as ex:
            t = wall(lambda: list(ex.map(_pil_roundtrip, host)))
        print(json.dumps({"what": "pillow_encode_decode_host", "size": [H, W], "threads": a.threads, "images": a.images,
                          "ms_per_image": 1e3 * t / a.images}))
        t1 = wall(lambda: _pil_roundtrip(host[0]))
        print(json.dumps({"what": "pillow_encode_decode_host", "size": [H, W], "threads": 1, "images": 1, "ms_per_image": 1e3 * t1}))
        x = (q[:8].float() / 255) * 0.3
        model.eval()
        with torch.no_grad():
            t_fwd = wall(lambda: model(x)) / 8
        model.train()
        print(json.dumps({"what": "forward_per_image_at_bs8", "size": [H, W], "ms": t_fwd * 1e3}))
        if prm is None:
            continue
        images = _Named((q[i].float() / 255) * 0.3 for i in range(a.images))
        images.names = [f"{i:03d}.jpg" for i in range(a.images)]
        for bs in (1, 8):
            for flag in (False, True):
                t = wall(lambda: P.evaluate_unpaired(model, images, prm, batch_size=bs, file_roundtrip=flag))
                print(json.dumps({"what": "evaluate_unpaired", "size": [H, W], "batch_size": bs, "file_roundtrip": flag,
                                  "images": a.images, "s": t, "img_per_s": a.images / t}))


if __name__ == "__main__":
    main()
