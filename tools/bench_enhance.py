"""Cost of writing enhanced images to disk (hvi_cidnet_amd.image_io).  One JSON line per measurement:

  ingest / egress   the two kernels at 8 x 400 x 600 and 1 x 1024 x 1024: time per launch (device events around >= 200 launches,
                    host enqueue included when it is the slower side), the bytes a launch moves, from shapes -- 3 h w + 12 Hp Wp
                    per image -- and the achieved bytes per second; ingest with the / 255 quotients and with a gamma table
  to_uint8          the project's existing fp32 -> uint8 pass (metrics.to_uint8) on the same shape, as a yardstick that is not the
                    code under test: 3 h w + 12 h w bytes per image
  torch_ingest /    the same results composed from torch ops: .permute().float() / 255, F.pad, ** gamma;
  torch_egress      clamp().mul(255).byte().permute() of the crop: time per call and kernel launches per call
  pipeline          a folder of 64 synthetic 400 x 600 PNGs written by this tool: enhance_folder(batch_size=8, threads=16,
                    depth=2) against the serial chain a caller had to write before it (decode -> upload fp32 -> enhance ->
                    to_uint8 -> .cpu() -> save, one thread), alternated, three times each: images per second, their ratio, and
                    the share of the pipelined run that the main thread spent waiting for a batch in flight

  large             (--images mixed | big, optionally --tile N) a folder written by this tool -- mixed: eight images of eight
                    sizes between 2.2 and 3.1 megapixels; big: one 4096 x 6144 image -- through enhance_folder(tile=N) (N absent:
                    the whole image per launch), once to warm up and three times timed: wall seconds and megapixels per second.
                    With --tile also the two tile kernels alone on the largest image's plan: time per launch, bytes from shapes
                    -- 15 per tile pixel in, 12 per tile pixel + 3 per image pixel out -- and achieved bytes per second.
                    --tile alone implies --images mixed.  Nothing else runs in this mode.

    python tools/bench_enhance.py [--launches 200] [--files 64] [--dir DIR] [--skip-pipeline]
    python tools/bench_enhance.py --images mixed [--tile 1024] [--tile_overlap 32] [--tile_batch 8]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK = 8.0e12                 # bytes / s, MI355X specification
CASES = [(8, 400, 600), (1, 1024, 1024)]


def image_bytes(h, w, Hp, Wp):
    return 3 * h * w + 12 * Hp * Wp


def _events(fn, n):
    """ms per call of fn over n calls, by device events (host enqueue included when it is the slower side)"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def _line(what, shape, n, ms, nbytes, **extra):
    print(json.dumps({"what": what, "shape": list(shape), "calls": n, "us_per_call": ms * 1e3, "bytes": nbytes,
                      "bytes_per_s": nbytes / (ms * 1e-3), "share_of_hbm_peak": nbytes / (ms * 1e-3) / HBM_PEAK, **extra}),
          flush=True)


def kernels(n):
    import torch
    import torch.nn.functional as F
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import metrics as M
    from bench_data import _kernel_launches
    dev = torch.device("cuda:0")
    div = torch.full((), 255.0, dtype=torch.float32, device=dev)
    for B, h, w in CASES:
        Hp, Wp = P.image_io.padded_size(h, w)
        img = torch.randint(0, 256, (B, h, w, 3), dtype=torch.uint8, device=dev)
        x = torch.rand((B, 3, Hp, Wp), device=dev) * 1.2 - 0.1
        nb = B * image_bytes(h, w, Hp, Wp)
        for gamma in (1.0, 1.4):
            P.ingest(img, gamma=gamma)                            # warm-up: code object, table upload, allocator
            _line("ingest", (B, h, w), n, _events(lambda: P.ingest(img, gamma=gamma), n), nb, gamma=gamma, padded=[Hp, Wp])
        P.egress(x, (h, w))
        _line("egress", (B, h, w), n, _events(lambda: P.egress(x, (h, w)), n), nb, padded=[Hp, Wp])
        M.to_uint8(x, (h, w))
        _line("to_uint8", (B, h, w), n, _events(lambda: M.to_uint8(x, (h, w)), n), B * 15 * h * w, padded=[Hp, Wp])

        def torch_ingest(gamma):
            t = img.permute(0, 3, 1, 2).float() / div
            t = F.pad(t, (0, Wp - w, 0, Hp - h), "reflect") if (Hp, Wp) != (h, w) else t
            return t ** gamma if gamma != 1.0 else t.contiguous()

        def torch_egress():
            return x[:, :, :h, :w].clamp(0, 1).mul(255).byte().permute(0, 2, 3, 1).contiguous()
        for gamma in (1.0, 1.4):
            torch_ingest(gamma)
            _line("torch_ingest", (B, h, w), n, _events(lambda: torch_ingest(gamma), n), nb, gamma=gamma,
                  kernel_launches=_kernel_launches(lambda: torch_ingest(gamma)),
                  ours_launches=_kernel_launches(lambda: P.ingest(img, gamma=gamma)))
        torch_egress()
        _line("torch_egress", (B, h, w), n, _events(torch_egress, n), nb, kernel_launches=_kernel_launches(torch_egress),
              ours_launches=_kernel_launches(lambda: P.egress(x, (h, w))))


def _write_folder(folder, files, h=400, w=600):
    import numpy as np
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(0)
    for i in range(files):
        # smooth dark content (a PNG of noise does not compress and is not what a photograph decodes or encodes like)
        base = rng.integers(0, 96, size=(h // 8, w // 8, 3), dtype=np.uint8)
        Image.fromarray(base).resize((w, h), Image.BICUBIC).save(os.path.join(folder, f"{i:04d}.png"))


def _serial(model, files, out_dir, dev):
    """what a caller wrote before enhance_folder: one image at a time, one thread, 12 bytes per pixel up, planar bytes down"""
    import torch
    from PIL import Image
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import metrics as M
    os.makedirs(out_dir, exist_ok=True)
    for path, name in zip(files.paths, files.names):
        a = M._read_rgb(path)
        x = torch.from_numpy(a).permute(2, 0, 1).float().div(255).to(dev)
        y = P.enhance(model, x)
        q = M.to_uint8(y).permute(1, 2, 0).cpu()
        Image.fromarray(q.numpy()).save(os.path.join(out_dir, name))


def pipeline(folder, files):
    import torch
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import metrics as M
    dev = torch.device("cuda:0")
    src = os.path.join(folder, "in")
    _write_folder(src, files)
    torch.manual_seed(0)
    model = P.CIDNet().to(dev).eval()
    model.trans.alpha_s, model.trans.alpha = 1.0, 1.0            # what enhance() sets: both runs compute the same images
    listing = M.folder_images(src)
    kw = dict(alpha_s=1.0, alpha=1.0, batch_size=8, threads=16, depth=2)
    P.enhance_folder(model, listing, os.path.join(folder, "warm_p"), **kw)          # warm-up of both: code objects, allocator
    _serial(model, listing, os.path.join(folder, "warm_s"), dev)
    same = all(open(os.path.join(folder, "warm_p", n), "rb").read() == open(os.path.join(folder, "warm_s", n), "rb").read()
               for n in listing.names)
    rates = {"pipelined": [], "serial": []}
    for rep in range(3):
        torch.cuda.synchronize()
        r = P.enhance_folder(model, listing, os.path.join(folder, f"p{rep}"), **kw)
        rates["pipelined"].append(files / r.seconds["wall"])
        print(json.dumps({"what": "pipeline", "run": "enhance_folder", "rep": rep, "files": files, "batch_size": 8, "threads": 16,
                          "depth": 2, "s": r.seconds["wall"], "images_per_s": files / r.seconds["wall"],
                          "wait_for_slot_s": r.seconds["wait_for_slot"],
                          "wait_for_slot_share": r.seconds["wait_for_slot"] / r.seconds["wall"]}), flush=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _serial(model, listing, os.path.join(folder, f"s{rep}"), dev)
        t = time.perf_counter() - t0
        rates["serial"].append(files / t)
        print(json.dumps({"what": "pipeline", "run": "serial", "rep": rep, "files": files, "s": t, "images_per_s": files / t}),
              flush=True)
    med = {k: sorted(v)[1] for k, v in rates.items()}
    print(json.dumps({"what": "pipeline_summary", "files": files, "size": [400, 600], "files_identical": same,
                      "median_images_per_s": med, "pipelined_over_serial": med["pipelined"] / med["serial"],
                      "all_ratios_same_rep": [p / s for p, s in zip(rates["pipelined"], rates["serial"])]}), flush=True)


MIXED = [(1200, 1800), (1808, 1208), (1400, 2100), (1365, 2048), (1536, 2048), (2048, 1536), (1250, 1875), (1333, 2000)]
BIG = [(4096, 6144)]


def _write_sizes(folder, sizes):
    import numpy as np
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(0)
    for i, (h, w) in enumerate(sizes):
        base = rng.integers(0, 96, size=(h // 16, w // 16, 3), dtype=np.uint8)           # smooth dark content, as _write_folder
        Image.fromarray(base).resize((w, h), Image.BICUBIC).save(os.path.join(folder, f"{i:04d}.bmp"))   # .bmp: no codec time


def large(folder, which, tile, overlap, tile_batch, launches):
    import torch
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import metrics as M
    dev = torch.device("cuda:0")
    sizes = MIXED if which == "mixed" else BIG
    src = os.path.join(folder, "in")
    _write_sizes(src, sizes)
    torch.manual_seed(0)
    model = P.CIDNet().to(dev).eval()
    listing = M.folder_images(src)
    mp = sum(h * w for h, w in sizes) / 1e6
    kw = dict(alpha_s=1.0, alpha=1.0, threads=16, depth=2, tile=tile, overlap=overlap, tile_batch=tile_batch)
    for rep in range(-1, 3):                                     # -1: warm-up (code objects, allocator, every shape)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = P.enhance_folder(model, listing, os.path.join(folder, "out"), **kw)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        print(json.dumps({"what": "large", "images": which, "tile": tile, "overlap": overlap if tile else None,
                          "tile_batch": tile_batch if tile else None, "rep": rep, "files": len(sizes), "megapixels": mp, "s": t,
                          "megapixels_per_s": mp / t, "tiles": r.tiles, "wait_for_slot_s": r.seconds["wait_for_slot"],
                          "max_memory_allocated": torch.cuda.max_memory_allocated()}), flush=True)
    if tile is None:
        return
    h, w = max(sizes, key=lambda s: s[0] * s[1])
    plan = P.tile_plan(h, w, tile, overlap)
    n, (th, tw) = len(plan), plan.tile
    img = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev)
    y = torch.rand((n, 3, th, tw), device=dev) * 1.2 - 0.1
    for gamma in (1.0, 1.4):
        P.ingest_tiles(img, plan, gamma=gamma)
        _line("ingest_tiles", (h, w), launches, _events(lambda: P.ingest_tiles(img, plan, gamma=gamma), launches), 15 * n * th * tw,
              gamma=gamma, tile=[th, tw], tiles=n)
    P.egress_tiles(y, plan)
    _line("egress_tiles", (h, w), launches, _events(lambda: P.egress_tiles(y, plan), launches), 12 * n * th * tw + 3 * h * w,
          tile=[th, tw], tiles=n)
    Hp, Wp = plan.padded
    x = torch.rand((1, 3, Hp, Wp), device=dev)
    P.ingest(img), P.egress(x, (h, w))                           # the untiled kernels on the same image, as yardsticks
    _line("ingest", (1, h, w), launches, _events(lambda: P.ingest(img), launches), image_bytes(h, w, Hp, Wp), gamma=1.0)
    _line("egress", (1, h, w), launches, _events(lambda: P.egress(x, (h, w)), launches), image_bytes(h, w, Hp, Wp))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", choices=("mixed", "big"), default=None, help="the large-image mode (module docstring)")
    ap.add_argument("--tile", type=int, default=None)
    ap.add_argument("--tile_overlap", type=int, default=32)
    ap.add_argument("--tile_batch", type=int, default=8)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--dir", default=None, help="where the synthetic folder and the outputs go (default: a temporary directory)")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-pipeline", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_enhance.py measures on a ROCm device; there is none")
    if a.images or a.tile:
        with tempfile.TemporaryDirectory(dir=a.dir) as d:
            large(d, a.images or "mixed", a.tile, a.tile_overlap, a.tile_batch, max(50, a.launches))
        return
    if not a.skip_kernels:
        kernels(max(200, a.launches))
    if not a.skip_pipeline:
        if a.dir:
            pipeline(a.dir, a.files)
        else:
            with tempfile.TemporaryDirectory() as d:
                pipeline(d, a.files)


if __name__ == "__main__":
    main()
