"""Cost of the on-device PNG encoder (image_io.png_zlib_u8, enhance_folder(png="device")) at 8 x 400 x 600 and 1 x 1024 x 1024,
on a smooth scene with grain and on a constant image: device time of the launches between two events with the bytes they must
move, Pillow's default PNG save of the same images on a pool of host threads and on one thread, and the folder run -- 64
synthetic 400 x 600 files through enhance_folder(batch_size=8, threads=16, depth=2) as .png encoded by Pillow, .png encoded on
the device, and .bmp, alternated.  One JSON line per measurement.

    python tools/bench_png.py [--files 64] [--reps 5] [--threads 16] [--rounds 3]
"""
import argparse
import concurrent.futures as cf
import io
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((8, 400, 600), (1, 1024, 1024))


def _pil_png(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "PNG")
    return buf.tell()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--skip_folder", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib, image_io as IO
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)

    def photo(n, h, w):
        """smooth structure plus grain: a byte image that compresses like a photograph, uint8 (n,h,w,3) on the device"""
        yy = torch.linspace(0, 1, h, device=dev).view(1, h, 1, 1)
        xx = torch.linspace(0, 1, w, device=dev).view(1, 1, w, 1)
        c = torch.arange(3, device=dev).view(1, 1, 1, 3)
        base = 0.45 + 0.3 * torch.sin(9 * xx + c) * torch.cos(7 * yy - c)
        return ((base + 0.015 * torch.randn(n, h, w, 3, device=dev, generator=g)).clamp(0, 1) * 255).to(torch.uint8)

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
        best = float("inf")
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            best = min(best, time.perf_counter() - t0)
        return best

    L = _lib.lib()
    for B, H, W in SHAPES:
        for content in ("grain", "constant"):
            q = photo(B, H, W) if content == "grain" else torch.full((B, H, W, 3), 77, dtype=torch.uint8, device=dev)
            plan = IO.png_plan(H, W)
            streams, sizes = IO.png_zlib_u8(q)
            n = sizes.cpu().tolist()
            host = q.cpu().numpy()
            pil = [_pil_png(x) for x in host]
            # raw pixels read twice (scores, then the filtered bytes), filtered bytes written, read again, the stream written,
            # the slot zeroed
            moved = B * (2 * 3 * H * W + 2 * H * (1 + 3 * W) + plan.capacity) + sum(n)
            ms = device_ms(lambda: IO.png_zlib_u8(q), a.calls)
            print(json.dumps({"what": "png_zlib_u8_device", "shape": [B, H, W], "content": content, "ms_per_call": ms,
                              "ms_per_image": ms / B, "bytes_moved": moved, "GB_per_s": moved / ms / 1e6,
                              "segments": plan.segments, "capacity": plan.capacity, "stream_bytes": n[0], "pillow_bytes": pil[0],
                              "size_ratio_to_pillow": sum(n) / sum(pil)}))
            out = torch.empty((B, plan.capacity), dtype=torch.uint8, device=dev)
            sz = torch.empty(B, dtype=torch.int64, device=dev)
            ws = torch.empty(B * plan.ws_bytes, dtype=torch.uint8, device=dev)
            f, st = L.raw("cidnet_png_encode_u8"), torch.cuda.current_stream().cuda_stream
            args = (q.data_ptr(), 3 * H * W, out.data_ptr(), plan.capacity, sz.data_ptr(), ws.data_ptr(), ws.numel(), B, H, W, 5,
                    32768, st)
            ms = device_ms(lambda: f(*args), a.calls)
            assert torch.equal(out, streams) and torch.equal(sz, sizes)
            print(json.dumps({"what": "cidnet_png_encode_u8_device", "shape": [B, H, W], "content": content, "ms_per_call": ms,
                              "ms_per_image": ms / B, "GB_per_s": moved / ms / 1e6}))
            imgs = [host[i % B] for i in range(max(B, a.threads))]
            with cf.ThreadPoolExecutor(a.threads) as ex:
                t = wall(lambda: list(ex.map(_pil_png, imgs)))
            print(json.dumps({"what": "pillow_png_save_host", "shape": [B, H, W], "content": content, "threads": a.threads,
                              "images": len(imgs), "ms_per_image": 1e3 * t / len(imgs)}))
            t1 = wall(lambda: _pil_png(host[0]))
            print(json.dumps({"what": "pillow_png_save_host", "shape": [B, H, W], "content": content, "threads": 1, "images": 1,
                              "ms_per_image": 1e3 * t1}))
    if a.skip_folder:
        return
    model = P.CIDNet().to(dev).eval()
    root = tempfile.mkdtemp(prefix="cidnet_png_bench_")
    try:
        low = (photo(a.files, 400, 600).float() * 0.3).to(torch.uint8).cpu().numpy()
        for ext in ("png", "bmp"):
            os.makedirs(os.path.join(root, "in_" + ext))
            for i, x in enumerate(low):
                Image.fromarray(x).save(os.path.join(root, "in_" + ext, f"{i:03d}.{ext}"))
        runs = (("png", "pillow"), ("png", "device"), ("bmp", "pillow"))
        for ext, png in runs:                                    # warm-up: buffers, plans, the page cache
            P.enhance_folder(model, os.path.join(root, "in_" + ext), os.path.join(root, "out"), batch_size=8, threads=a.threads,
                             depth=2, png=png)
        for rnd in range(a.rounds):
            for ext, png in runs:
                rep = P.enhance_folder(model, os.path.join(root, "in_" + ext), os.path.join(root, "out"), batch_size=8,
                                       threads=a.threads, depth=2, png=png)
                s = rep.seconds
                print(json.dumps({"what": "enhance_folder", "round": rnd, "ext": ext, "png": png, "files": a.files,
                                  "size": [400, 600], "batch_size": 8, "threads": a.threads, "depth": 2, "wall_s": s["wall"],
                                  "img_per_s": a.files / s["wall"], "wait_for_slot_share": s["wait_for_slot"] / s["wall"]}))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
