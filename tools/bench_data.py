"""Cost of on-device training batches (hvi_cidnet_amd.data) at the LOL size: a synthetic resident set of 485 pairs of
400 x 600, B = 8, crops 256 and (400, 600), gamma off and on.  One JSON line per measurement:

  batches        time per batch of the TrainBatches loop (device events around >= 200 batches, host enqueue included) and the
                 bytes a batch moves, from shapes: 2 B 3 S_h S_w (4 + 1)
  to_uint8       the project's existing fp32 <-> uint8 pass (metrics.to_uint8) on the same shape, as a yardstick that is not
                 the code under test
  torch_ops      the same batch composed from torch ops on the same arena (index, slice, flip, .float(), / 255, ** gamma):
                 time per batch and kernel launches per batch
  train          DataParallelTrainer at B = 8, 400 x 600: fed one fixed batch (as bench.py does) and fed by TrainBatches with
                 crop (400, 600), alternated, three times each
  raw            (--raw, a leg of its own) the launch that also writes the un-powered low image (cidnet_augment_crop_flip_raw:
                 x, gt, raw) beside what gives the same three tensors without it -- two launches of the plain entry point,
                 gamma on and gamma 1 -- and beside the plain single launch as it stands; same set, B and crops; the three
                 alternate within one run, five rounds each, into preallocated outputs, timed by device events.  Bytes from
                 shapes: B 3 S_h S_w (2 + 12) / 2 (2 + 8) / (2 + 8).  Lines are appended to profiles/data_raw.jsonl
  load           optional (--decode DIR): PNGs written to DIR, then ResidentPairs.from_folders timed (decode rate, load time)

    python tools/bench_data.py [--pairs 485] [--batches 200] [--train-steps 20] [--skip-train]
    python tools/bench_data.py --raw [--batches 2000] [--out profiles/data_raw.jsonl]
    rocprofv3 --kernel-trace --stats -f csv -d OUT -o run -- python tools/bench_data.py --kernel-only
      (then: python tools/bench_data.py --share OUT/.../run_kernel_stats.csv -> time per launch of crop_flip_kernel and
       to_uint8_kernel, bytes per second, share of the HBM peak)
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12                 # bytes / s, MI355X specification; about 6.3e12 is what a float4 copy achieves
H, W, B = 400, 600, 8
CASES = [(256, 256), (H, W)]


def batch_bytes(sh, sw, b=B):
    return 2 * b * 3 * sh * sw * (4 + 1)


def _share(path):
    """kernel_stats.csv of a --kernel-only run: that run launches every case of CASES x (gamma off, on) equally often, so the
    csv's average mixes them; the per-case split comes from the kernel trace when it is next to the stats file"""
    out = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            for k in ("crop_flip_kernel", "to_uint8_kernel"):
                if k in r["Name"]:
                    out[k] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3,
                              "min_us": float(r.get("MinNs", "nan")) / 1e3, "max_us": float(r.get("MaxNs", "nan")) / 1e3}
    trace = path.replace("kernel_stats.csv", "kernel_trace.csv")
    if os.path.exists(trace):
        by_grid = {}
        with open(trace) as f:
            for r in csv.DictReader(f):
                name = r.get("Kernel_Name", "")
                for k in ("crop_flip_kernel", "to_uint8_kernel"):
                    if k in name:
                        key = (k, int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r.get("Grid_Size", 0)))
                        by_grid.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        # crop_flip grid x = ceil(S_h ceil(S_w / 4) / 512) blocks of 256 threads
        grids = {(-(-sh * -(-sw // 4) // 512)) * 256: (sh, sw) for sh, sw in CASES}
        for (k, gx), us in sorted(by_grid.items()):
            us.sort()
            med = us[len(us) // 2]
            row = {"kernel": k, "grid_x": gx, "calls": len(us), "median_us": med, "min_us": us[0]}
            if k == "crop_flip_kernel" and gx in grids:
                sh, sw = grids[gx]
                row.update(crop=[sh, sw], bytes=batch_bytes(sh, sw), bytes_per_s=batch_bytes(sh, sw) / (med * 1e-6),
                           share_of_hbm_peak=batch_bytes(sh, sw) / (med * 1e-6) / HBM_PEAK)
            if k == "to_uint8_kernel":
                nb = B * 3 * H * W * 5
                row.update(bytes=nb, bytes_per_s=nb / (med * 1e-6), share_of_hbm_peak=nb / (med * 1e-6) / HBM_PEAK)
            print(json.dumps(row))
    print(json.dumps({"kernel_stats": out}))


def _resident(dev, n):
    import torch
    from hvi_cidnet_amd import ResidentPairs
    g = torch.Generator().manual_seed(0)
    distinct = [torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g) for _ in range(16)]
    t0 = time.perf_counter()
    pairs = ResidentPairs([distinct[i % 16] for i in range(n)], [distinct[(i + 5) % 16] for i in range(n)], dev)
    torch.cuda.synchronize()
    return pairs, time.perf_counter() - t0


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


def _torch_batch(pairs, rows, size, gamma, div):
    """the batch from torch ops on the resident arena"""
    import torch
    sh, sw = size
    xs, gs = [], []
    for i, y0, x0, hf, vf in rows:
        dims = [d for d, on in ((2, hf), (1, vf)) if on]
        lo = pairs.low(i)[:, y0:y0 + sh, x0:x0 + sw]
        hi = pairs.high(i)[:, y0:y0 + sh, x0:x0 + sw]
        xs.append(lo.flip(dims) if dims else lo)
        gs.append(hi.flip(dims) if dims else hi)
    x = torch.stack(xs).float() / div
    gt = torch.stack(gs).float() / div
    return (x ** gamma if gamma is not None else x), gt


def _kernel_launches(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    # device-side events, so that launches made outside any ATen op (ours, through ctypes) count as well
    from torch.autograd import DeviceType
    return sum(1 for ev in prof.events() if ev.device_type == DeviceType.CUDA
               and not any(s in ev.name.lower() for s in ("memcpy", "memset")))


def _raw_leg(a, dev, pairs):
    """the --raw leg: one uploaded plan per crop, the same rows and table for the three variants"""
    import ctypes
    import torch
    from hvi_cidnet_amd import data as D, ops
    from hvi_cidnet_amd._lib import lib
    n, rounds = a.batches, 5
    lines = []
    for size in CASES:
        sh, sw = size
        p = D.epoch_plan(pairs.sizes, size, B, seed=0, epoch=0, drop_last=True, gamma=(60, 120))
        buf = D._pack(D.plan_rows(pairs.layout, p.index, p.y0, p.x0, p.hflip, p.vflip, p.crop),
                      [D.gamma_table(g) for g in p.gammas]).to(dev)
        words = p.index.numel() * D.PLAN_WORDS
        steps = len(p.batches)
        x, gt, raw, gt2 = (torch.empty((B, 3, sh, sw), dtype=torch.float32, device=dev) for _ in range(4))
        arena, stream, k = ops._p(pairs.arena), ops._stream(), [0]

        def args():
            k[0] = (k[0] + 1) % steps
            return (ctypes.c_void_p(buf.data_ptr() + 8 * D.PLAN_WORDS * B * k[0]),
                    ctypes.c_void_p(buf.data_ptr() + 8 * (words + k[0] * D._TABLE_WORDS)))

        def raw_launch():
            plan, table = args()
            lib().call("cidnet_augment_crop_flip_raw", arena, plan, table, ops._p(x), ops._p(raw), ops._p(gt), B, sh, sw, stream)

        def two_launches():
            plan, table = args()
            lib().call("cidnet_augment_crop_flip", arena, plan, table, ops._p(x), ops._p(gt), B, sh, sw, stream)
            lib().call("cidnet_augment_crop_flip", arena, plan, None, ops._p(raw), ops._p(gt2), B, sh, sw, stream)

        def single_launch():
            plan, table = args()
            lib().call("cidnet_augment_crop_flip", arena, plan, table, ops._p(x), ops._p(gt), B, sh, sw, stream)
        px = B * 3 * sh * sw
        variants = [("raw_launch", raw_launch, px * 14), ("two_launches", two_launches, px * 20),
                    ("single_launch", single_launch, px * 10)]
        for _, fn, _ in variants:                            # warm-up: code objects, clocks
            _events(fn, 50)
        us = {name: [] for name, _, _ in variants}
        for _ in range(rounds):
            for name, fn, _ in variants:
                us[name].append(_events(fn, n) * 1e3)
        if a.kernel_only:
            continue
        for name, _, nb in variants:
            v = sorted(us[name])
            line = json.dumps({"what": "raw", "variant": name, "crop": list(size), "B": B, "launches_per_round": n,
                               "rounds": rounds, "us_per_batch_median": v[rounds // 2], "us_per_batch_min": v[0],
                               "us_per_batch_max": v[-1], "bytes": nb, "bytes_per_s_at_median": nb / (v[rounds // 2] * 1e-6),
                               "timed": "device events around the launches of a round, host enqueue included"})
            print(line)
            lines.append(line)
    if lines:                                                    # --kernel-only writes nothing and touches no file
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=485)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--train-steps", type=int, default=20)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--kernel-only", action="store_true", help="only launch the kernels (for a rocprofv3 run)")
    ap.add_argument("--raw", action="store_true", help="only the leg that times cidnet_augment_crop_flip_raw")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_raw.jsonl"), help="--raw appends its lines here")
    ap.add_argument("--decode", default=None, help="directory to write PNGs to and load them back from")
    ap.add_argument("--share", default=None, help="kernel_stats.csv of a rocprofv3 run of this tool with --kernel-only")
    a = ap.parse_args()
    if a.share is not None:
        _share(a.share)
        return
    import torch
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd import metrics as M
    dev = torch.device("cuda:0")
    pairs, t_load = _resident(dev, a.pairs)
    print(json.dumps({"what": "resident_set", "pairs": a.pairs, "size": [H, W], "arena_bytes": pairs.arena.numel(),
                      "upload_s": t_load}))
    if a.raw:
        _raw_leg(a, dev, pairs)
        return
    out = torch.rand((B, 3, H, W), device=dev)
    div = torch.full((), 255.0, dtype=torch.float32, device=dev)

    for size in CASES:
        for gamma in (None, (60, 120)):
            tb = P.TrainBatches(pairs, B, size, seed=0, gamma=gamma, drop_last=True)
            epochs = -(-a.batches // len(tb))
            n = epochs * len(tb)

            def loop(e0):
                for e in range(e0, e0 + epochs):
                    for x, gt in tb.epoch(e):
                        pass
            loop(100)                                            # warm-up: allocator, code object
            torch.cuda.synchronize()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            ev0.record()
            loop(0)
            ev1.record()
            t_host = time.perf_counter() - t0
            torch.cuda.synchronize()
            ms = ev0.elapsed_time(ev1) / n
            if a.kernel_only:
                continue
            nb = batch_bytes(*size)
            print(json.dumps({"what": "batches", "crop": list(size), "gamma": gamma is not None, "batches": n,
                              "us_per_batch": ms * 1e3, "host_enqueue_us_per_batch": t_host / n * 1e6, "bytes": nb,
                              "bytes_per_s_of_the_loop": nb / (ms * 1e-3)}))
            p = tb.plan(0)
            lo, hi = p.batches[0]
            rows = list(zip(*[c[lo:hi].tolist() for c in (p.index, p.y0, p.x0, p.hflip, p.vflip)]))
            g = p.gammas[0] if gamma is not None else None
            _torch_batch(pairs, rows, size, g, div)
            launches = _kernel_launches(lambda: _torch_batch(pairs, rows, size, g, div))
            ms_t = _events(lambda: _torch_batch(pairs, rows, size, g, div), a.batches)
            print(json.dumps({"what": "torch_ops", "crop": list(size), "gamma": gamma is not None, "batches": a.batches,
                              "us_per_batch": ms_t * 1e3, "kernel_launches_per_batch": launches,
                              "ours_launches_per_batch": _kernel_launches(lambda: next(iter(tb.epoch(0))))}))
    M.to_uint8(out)
    ms_q = _events(lambda: M.to_uint8(out), a.batches)
    if a.kernel_only:
        return
    nb = B * 3 * H * W * 5
    print(json.dumps({"what": "to_uint8", "shape": [B, 3, H, W], "calls": a.batches, "us_per_call": ms_q * 1e3, "bytes": nb,
                      "bytes_per_s_of_the_loop": nb / (ms_q * 1e-3)}))

    if a.decode:
        import numpy as np
        from PIL import Image
        n_files = 64
        rng = np.random.default_rng(0)
        for d in ("low", "high"):
            os.makedirs(os.path.join(a.decode, d), exist_ok=True)
            for i in range(n_files):
                # smooth content (PNG of noise does not compress and is not what a photograph decodes like)
                base = rng.integers(0, 256, size=(H // 8, W // 8, 3), dtype=np.uint8)
                Image.fromarray(base, "RGB").resize((W, H), Image.BICUBIC).save(os.path.join(a.decode, d, f"{i:04d}.png"))
        t0 = time.perf_counter()
        rp = P.ResidentPairs.from_folders(os.path.join(a.decode, "low"), os.path.join(a.decode, "high"), dev)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        print(json.dumps({"what": "load", "label": "OPTIONAL: synthetic smooth PNGs, this machine's CPUs", "pairs": len(rp),
                          "files": 2 * n_files, "s": t, "files_per_s": 2 * n_files / t,
                          "extrapolated_s_for_485_pairs": t * 485 / n_files}))

    if a.skip_train:
        return
    from hvi_cidnet_amd.dp import DataParallelTrainer
    torch.manual_seed(0)
    model = P.CIDNet().to(dev)
    tr = DataParallelTrainer(model)
    x0, gt0 = torch.rand((B, 3, H, W), device=dev), torch.rand((B, 3, H, W), device=dev)
    tb = P.TrainBatches(pairs, B, (H, W), seed=0, drop_last=True)

    def stream():
        e = 0
        while True:
            yield from tb.epoch(e)
            e += 1
    it = stream()
    for _ in range(5):
        tr.step(x0, gt0)
    for _ in range(5):
        tr.step(*next(it))
    torch.cuda.synchronize()
    for rep in range(3):
        for feed in ("fixed_batch", "train_batches"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.train_steps):
                if feed == "fixed_batch":
                    tr.step(x0, gt0)
                else:
                    tr.step(*next(it))
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            print(json.dumps({"what": "train", "feed": feed, "rep": rep, "steps": a.train_steps, "ms_per_step": t / a.train_steps * 1e3,
                              "img_per_s": a.train_steps * B / t}))


if __name__ == "__main__":
    main()
