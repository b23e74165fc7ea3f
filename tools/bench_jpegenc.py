"""Cost of the on-device JPEG encoder (image_io.jpeg_scan_u8, enhance_folder(jpeg="device")) at 8 x 400 x 600 and 1 and 8 x
1024 x 1024, on a smooth scene with grain and on a constant image: device time of the six launches between two events, Pillow's
save(.., 'JPEG') of the same images alone (no open) on a pool of host threads and on one thread -- Pillow is the yardstick,
not the code under test -- and the folder run: 64 synthetic 400 x 600 files and 16 of 1728 x 2304, through
enhance_folder(batch_size=8, threads=16, depth=2) as .jpg encoded by Pillow, .jpg encoded on the device, and .bmp, alternated,
with wait-for-slot shares, bytes downloaded per image and second-copy counts.  One JSON line per measurement.

    python tools/bench_jpegenc.py [--reps 5] [--calls 200] [--threads 16] [--rounds 3] [--skip_folder] [--only_kernels]
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

SHAPES = ((8, 400, 600), (1, 1024, 1024), (8, 1024, 1024))
FOLDERS = ((64, 400, 600), (16, 1728, 2304))


def _pil_jpeg(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG")
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--jpeg_prefix", type=float, default=0.25)
    ap.add_argument("--skip_folder", action="store_true")
    ap.add_argument("--only_kernels", action="store_true", help="a few encoder calls and nothing else (for a kernel trace)")
    a = ap.parse_args()
    import torch
    from PIL import Image
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import _lib, metrics as M, image_io as IO
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
            plan = IO.jpeg_encode_plan(H, W)
            out = torch.empty((B, plan.capacity), dtype=torch.uint8, device=dev)
            sz = torch.empty(B, dtype=torch.int64, device=dev)
            ws = torch.empty(B * plan.ws_bytes, dtype=torch.uint8, device=dev)
            f, st = L.raw("cidnet_jpeg_encode_u8"), torch.cuda.current_stream().cuda_stream
            args = (q.data_ptr(), 3 * H * W, out.data_ptr(), plan.capacity, sz.data_ptr(), ws.data_ptr(), ws.numel(),
                    M._jpeg_table_on(dev, 75).data_ptr(), B, H, W, st)
            if a.only_kernels:
                for _ in range(10):
                    assert f(*args) == 0
                torch.cuda.synchronize()
                continue
            ms = device_ms(lambda: f(*args), a.calls)
            n = sz.cpu().tolist()
            host = q.cpu().numpy()
            pil = [_pil_jpeg(x) for x in host]
            got = out.cpu().numpy()
            same = all(IO.jpeg_file(H, W, 75, got[b, :n[b]].tobytes()) == pil[b] for b in range(B))
            print(json.dumps({"what": "cidnet_jpeg_encode_u8_device", "shape": [B, H, W], "content": content, "ms_per_call": ms,
                              "ms_per_image": ms / B, "raw_bytes": 3 * H * W, "scan_bytes": n[0], "capacity": plan.capacity,
                              "ws_bytes_per_image": plan.ws_bytes, "groups": plan.groups, "equals_pillow": same}), flush=True)
            imgs = [host[i % B] for i in range(max(B, a.threads))]
            with cf.ThreadPoolExecutor(a.threads) as ex:
                t = wall(lambda: list(ex.map(_pil_jpeg, imgs)))
            print(json.dumps({"what": "pillow_jpeg_save_host", "shape": [B, H, W], "content": content, "threads": a.threads,
                              "images": len(imgs), "ms_per_image": 1e3 * t / len(imgs)}), flush=True)
            t1 = wall(lambda: _pil_jpeg(host[0]))
            print(json.dumps({"what": "pillow_jpeg_save_host", "shape": [B, H, W], "content": content, "threads": 1, "images": 1,
                              "ms_per_image": 1e3 * t1}), flush=True)
    if a.skip_folder or a.only_kernels:
        return
    model = P.CIDNet().to(dev).eval()
    for files, H, W in FOLDERS:
        root = tempfile.mkdtemp(prefix="cidnet_jpegenc_bench_")
        try:
            for ext in ("jpg", "bmp"):
                os.makedirs(os.path.join(root, "in_" + ext))
            for i in range(files):
                x = (photo(1, H, W).float() * 0.3).to(torch.uint8)[0].cpu().numpy()
                Image.fromarray(x).save(os.path.join(root, "in_jpg", f"{i:03d}.jpg"), quality=95)
                Image.fromarray(x).save(os.path.join(root, "in_bmp", f"{i:03d}.bmp"))
            runs = (("jpg", "pillow"), ("jpg", "device"), ("bmp", "pillow"))
            kw = dict(batch_size=8, threads=a.threads, depth=2, jpeg_prefix=a.jpeg_prefix)
            for ext, jpeg in runs:                               # warm-up: buffers, plans, the page cache
                P.enhance_folder(model, os.path.join(root, "in_" + ext), os.path.join(root, "out_" + jpeg), jpeg=jpeg, **kw)
            names = sorted(os.listdir(os.path.join(root, "out_device")))
            same = all(open(os.path.join(root, "out_device", n), "rb").read() == open(os.path.join(root, "out_pillow", n), "rb").read()
                       for n in names if n.endswith(".jpg"))
            for rnd in range(a.rounds):
                for ext, jpeg in runs:
                    rep = P.enhance_folder(model, os.path.join(root, "in_" + ext), os.path.join(root, "out_" + jpeg), jpeg=jpeg, **kw)
                    s = rep.seconds
                    print(json.dumps({"what": "enhance_folder", "round": rnd, "ext": ext, "jpeg": jpeg, "files": files,
                                      "size": [H, W], "batch_size": 8, "threads": a.threads, "depth": 2, "wall_s": s["wall"],
                                      "img_per_s": files / s["wall"], "wait_for_slot_share": s["wait_for_slot"] / s["wall"],
                                      "downloaded_bytes_per_image": rep.downloaded / files, "raw_bytes_per_image": 3 * H * W,
                                      "second_copies": rep.jpeg_second_copies, "jpeg_prefix": a.jpeg_prefix,
                                      "device_files_equal_pillows": same}), flush=True)
        finally:
            shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
