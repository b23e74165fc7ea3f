"""GPU: gradient accumulation and the EMA of the weights on the device: the three kernels of csrc/accum.hip against numpy
fp32 bit for bit, and dp.DataParallelTrainer(accum_steps, ema_decay) / fit.fit with them -- an accumulated update against
passes added by hand, the launch list of a step, the average across a skipped step, ema_weights(), hipGraph replay, exact
resume, two ranks.  The poisoned steps below are NaN arithmetic in healthy kernels, not faults."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import cidnet_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import data_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL, SMALL = (36, 36, 72, 144), (12, 12, 24, 48)
SHAPE_SMALL, SHAPE_FULL = (2, 3, 32, 48), (2, 3, 64, 96)
SENTINEL = -7.25


def _model(dev, chans, seed=21):
    import hvi_cidnet_amd as P
    m = P.CIDNet(channels=list(chans))
    p = O.make_params(seed, channels=chans)
    m.load_state_dict({k: p[k] for k in m.state_dict().keys()})
    return m.to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _batches(dev, n, shape, seed=31):
    return [(O.synthetic_batch(seed + i, shape).to(dev), O.synthetic_batch(seed + 100 + i, shape).to(dev)) for i in range(n)]


def _ema_numpy(e, p, decay):
    """e + w (p - e) in fp32, three roundings, w = fp32(1 - decay) formed in double"""
    w = np.float32(1.0 - decay)
    return (e + (w * (p - e).astype(np.float32)).astype(np.float32)).astype(np.float32)


# ---- the kernels ------------------------------------------------------------------------------------------------------------
def _framed(values, off, dev):
    """values inside a sentinel-filled buffer, starting `off` floats behind a 16-byte boundary -> (buffer, view)"""
    n = values.size
    buf = torch.full((n + 16,), SENTINEL, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[4 + off:4 + off + n]
    view.copy_(torch.from_numpy(values))
    return buf, view


def _frame_intact(buf, off, n):
    b = buf.cpu().numpy()
    return (b[:4 + off] == SENTINEL).all() and (b[4 + off + n:] == SENTINEL).all()


@pytest.mark.parametrize("n", [1, 3, 5, 1023, 4103])
def test_kernels_bit_exact_at_every_alignment(dev, n):
    """n = 4103 is more than one block's share (4 floats x 256 lanes) plus a ragged tail; the two bases take every pair of
    offsets 0..3 from a 16-byte boundary, so head, body and tail all meet misaligned partners"""
    from hvi_cidnet_amd import ops
    from hvi_cidnet_amd.dp import ema_weight
    rng = np.random.default_rng(n)
    a = (rng.standard_normal(n) * 3).astype(np.float32)
    b = (rng.standard_normal(n) * 0.01).astype(np.float32)
    decay = 0.999
    w = ema_weight(decay)
    assert np.float32(w) == np.float32(1.0 - decay)
    for oa in range(4):
        for ob in range(4):
            # grad_accumulate, first = 1 then 0
            bd, d = _framed(a, oa, dev)
            bs, s = _framed(b, ob, dev)
            ops.grad_accumulate(d, s, first=True)
            assert d.cpu().numpy().tobytes() == b.tobytes()
            d.copy_(torch.from_numpy(a))
            ops.grad_accumulate(d, s, first=False)
            assert d.cpu().numpy().tobytes() == (a + b).astype(np.float32).tobytes(), (n, oa, ob)
            assert s.cpu().numpy().tobytes() == b.tobytes() and _frame_intact(bd, oa, n) and _frame_intact(bs, ob, n)
            # ema_update: no record, apply = 1, apply = 0
            want = _ema_numpy(a, b, decay)
            for record, expect in ((None, want), (torch.tensor([1.0, 0.5, 0.1, 0.1], device=dev), want),
                                   (torch.tensor([0.0, 0.5, 0.1, 0.1], device=dev), a)):
                be, e = _framed(a, oa, dev)
                bp, p = _framed(b, ob, dev)
                ops.ema_update(e, p, w, record)
                assert e.cpu().numpy().tobytes() == expect.tobytes(), (n, oa, ob, record)
                assert p.cpu().numpy().tobytes() == b.tobytes() and _frame_intact(be, oa, n) and _frame_intact(bp, ob, n)
            # swap, and swap again
            bx, x = _framed(a, oa, dev)
            by, y = _framed(b, ob, dev)
            ops.swap(x, y)
            assert x.cpu().numpy().tobytes() == b.tobytes() and y.cpu().numpy().tobytes() == a.tobytes()
            ops.swap(x, y)
            assert x.cpu().numpy().tobytes() == a.tobytes() and y.cpu().numpy().tobytes() == b.tobytes()
            assert _frame_intact(bx, oa, n) and _frame_intact(by, ob, n)


def test_kernels_reject_what_they_cannot_do(dev):
    from hvi_cidnet_amd import ops
    t = torch.zeros(64, device=dev)
    with pytest.raises(RuntimeError):
        ops.swap(t[:40], t[20:60])                      # overlapping
    with pytest.raises(RuntimeError):
        ops.grad_accumulate(t[:8], t[8:17], True)       # lengths differ
    with pytest.raises(RuntimeError):
        ops.ema_update(t[:8], t[8:16].cpu(), 0.1)


# ---- the trainer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_accumulated_update_equals_three_passes_added_by_hand(dev, precision):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd.dp import DataParallelTrainer, StepLog
    K = 3
    bs = _batches(dev, 2 * K, SHAPE_SMALL)
    kw = dict(lr=1e-3, n_buckets=3, max_grad_norm=0.05, skip_nonfinite=True)
    P.set_precision(precision)
    try:
        log, log2 = StepLog(4), StepLog(4)
        tr = DataParallelTrainer(_model(dev, SMALL), accum_steps=K, step_log=log, **kw)
        hand = DataParallelTrainer(_model(dev, SMALL), step_log=log2, **kw)
        third = float(np.float32(1.0 / K))
        for u in range(2):
            group = bs[u * K:(u + 1) * K]
            for j, (x, gt) in enumerate(group):
                assert tr.pending_passes == j
                tr.step(x, gt)
            assert tr.pending_passes == 0
            total, loss_sum = None, None
            for x, gt in group:
                ls = hand.forward_backward(x, gt).reshape(1)
                torch.cuda.synchronize()
                g = hand.flat_g.clone()
                total = g if total is None else total + g            # fp32, pass order
                loss_sum = ls.clone() if loss_sum is None else loss_sum + ls
            hand.opt.step(total, hand.n_live, grad_scale=1.0 / K, loss=loss_sum * third, log_row=log2.next_row().data_ptr())
            hand.weights_changed()
            torch.cuda.synchronize()
            assert _same(tr.flat_p, hand.flat_p) and _same(tr.opt.m, hand.opt.m) and _same(tr.opt.v, hand.opt.v), u
        rows, rows2 = log.read(), log2.read()
    finally:
        P.set_precision("f32")
    assert rows.shape == (2, 4) and rows.tobytes() == rows2.tobytes(), (rows, rows2)
    assert rows[:, 3].tolist() == [1, 2] and np.isfinite(rows).all()


def _foreign_kernels(fn):
    """{kernel name: [aten op, ...]} of every launch of fn() that is not a cidnet:: kernel (tests/test_guard_gpu.py's check)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    from torch.autograd import DeviceType
    out, ours = {}, set()
    for ev in prof.events():
        # device-side events: launches made outside any ATen op (ours, through ctypes) are listed there as well
        if ev.device_type == DeviceType.CUDA and not any(s in ev.name.lower() for s in ("memcpy", "memset")):
            if "cidnet::" in ev.name:
                ours.add(ev.name)
            else:
                out.setdefault(ev.name, []).append("(device event)")
        for k in getattr(ev, "kernels", []) or []:
            if "cidnet::" in k.name:
                ours.add(k.name)
            else:
                out.setdefault(k.name, []).append(ev.name)
    return out, ours


@pytest.mark.parametrize("guarded", [True, False])
def test_accumulated_ema_step_launches_only_cidnet_kernels(dev, guarded):
    from hvi_cidnet_amd.dp import DataParallelTrainer, StepLog
    x, gt = _batches(dev, 1, SHAPE_FULL, seed=41)[0]
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True, step_log=StepLog(16)) if guarded else {}
    tr = DataParallelTrainer(_model(dev, FULL), lr=1e-3, accum_steps=2, ema_decay=0.999, **kw)
    for _ in range(4):
        tr.step(x, gt)

    def two_updates():
        for _ in range(4):
            tr.step(x, gt)

    fk, ours = _foreign_kernels(two_updates)
    assert not fk, {k: v[:3] for k, v in fk.items()}
    for want in ("grad_accumulate_kernel", "ema_update_kernel", "adam_dev_kernel" if guarded else "adam_kernel"):
        assert any(want in k for k in ours), (want, sorted(ours)[:5])
    assert tr.pending_passes == 0


def test_ema_on_the_device_across_a_skipped_step_and_ema_weights(dev):
    from hvi_cidnet_amd import ops
    from hvi_cidnet_amd.dp import DataParallelTrainer, StepLog
    decay = 0.9
    bs = _batches(dev, 8, SHAPE_FULL, seed=51)
    factor = torch.ones((), device=dev)

    def loss_fn(out, gt):
        return ops.L1LossFn.apply(out, gt) * factor

    def make():
        return DataParallelTrainer(_model(dev, FULL), lr=1e-3, loss_fn=loss_fn, max_grad_norm=1.0, skip_nonfinite=True,
                                   step_log=StepLog(16), ema_decay=decay)

    tr, twin = make(), make()
    want = None
    for i, (x, gt) in enumerate(bs[:6]):
        torch.cuda.synchronize()
        before = tr.ema.clone() if i else None
        factor.fill_(float("nan") if i == 3 else 1.0)
        tr.step(x, gt)
        twin.step(x, gt)
        factor.fill_(1.0)
        torch.cuda.synchronize()
        n = tr.n_live
        if want is None:
            assert tr.ema.numel() == tr.flat_p.numel() > n and _same(tr.ema[n:], tr.flat_p[n:])
            tr0 = DataParallelTrainer(_model(dev, FULL), lr=1e-3)
            tr0.forward_backward(x, gt)
            torch.cuda.synchronize()
            want = tr0.flat_p[:n].cpu().numpy().copy()            # the initial weights in arena order
        if i == 3:
            assert _same(tr.ema, before)                          # bit-unchanged across the skipped step
        else:
            want = _ema_numpy(want, tr.flat_p[:n].cpu().numpy(), decay)
        assert tr.ema[:n].cpu().numpy().tobytes() == want.tobytes(), i
    assert (tr.opt.steps_applied(), tr.opt.steps_skipped()) == (5, 1)
    assert _same(tr.ema[n:], tr.flat_p[n:]) and torch.isfinite(tr.ema).all()
    # ema_weights(): the model computes with the average, and everything comes back bit for bit
    sd = tr.ema_state_dict()
    fresh = _model(dev, FULL, seed=9)
    fresh.load_state_dict(sd, strict=True)
    p0, e0 = tr.flat_p.clone(), tr.ema.clone()
    x = bs[6][0]
    with torch.no_grad():
        plain = tr.model(x)
        with tr.ema_weights():
            inside = tr.model(x)
            torch.cuda.synchronize()
            assert _same(tr.flat_p, e0) and _same(tr.ema, p0)
            assert _same(inside, fresh(x)) and not _same(inside, plain)
            with pytest.raises(RuntimeError, match="ema_weights"):
                tr.step(*bs[6])
        assert _same(tr.model(x), plain)

    class Boom(Exception):
        pass

    with pytest.raises(Boom):
        with tr.ema_weights():
            raise Boom
    torch.cuda.synchronize()
    assert _same(tr.flat_p, p0) and _same(tr.ema, e0)
    # the next steps are those of the twin that never entered: the prepared operands were rebuilt both ways
    for x, gt in bs[6:8]:
        tr.step(x, gt)
        twin.step(x, gt)
    torch.cuda.synchronize()
    assert _same(tr.flat_p, twin.flat_p) and _same(tr.ema, twin.ema) and _same(tr.opt.m, twin.opt.m)
    # an open group refuses the context
    acc = DataParallelTrainer(_model(dev, SMALL), lr=1e-3, accum_steps=2, ema_decay=decay)
    xs, gs = _batches(dev, 1, SHAPE_SMALL)[0]
    acc.step(xs, gs)
    with pytest.raises(RuntimeError, match="open"):
        with acc.ema_weights():
            pass
    with pytest.raises(RuntimeError, match="open"):
        acc.state_dict()
    acc.flush()
    assert acc.pending_passes == 0
    with acc.ema_weights():
        pass


def test_graph_replay_with_accumulation_equals_eager(dev):
    from hvi_cidnet_amd.dp import DataParallelTrainer
    bs = _batches(dev, 5, SHAPE_SMALL, seed=61)
    res = []
    for use_graph in (False, True):
        tr = DataParallelTrainer(_model(dev, SMALL), lr=1e-3, n_buckets=3, use_graph=use_graph, accum_steps=2, ema_decay=0.99)
        losses = [float(tr.step(x, gt).item()) for x, gt in bs]
        assert tr.pending_passes == 1
        tr.flush()
        torch.cuda.synchronize()
        res.append((losses, tr.flat_p.clone(), tr.ema.clone(), tr.opt.m.clone()))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert all(_same(a, b) for a, b in zip(res[0][1:], res[1][1:]))
    assert not _same(res[0][1], res[0][2])


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=False)


def test_fit_accumulates_averages_and_resumes_exactly_on_the_device(dev, tmp_path):
    """three batches per epoch with K = 2: two updates per epoch, the second by flush() from one pass"""
    import hvi_cidnet_amd as P
    crop = (32, 48)

    def batches():
        sizes = [(40, 60), (32, 48), (50, 65)] * 2
        pairs = P.ResidentPairs(R.random_images(23, sizes), R.random_images(1023, sizes), dev)
        return P.TrainBatches(pairs, 2, crop, seed=3, gamma=(60, 120))

    lows, highs = R.random_images(77, [crop] * 2), R.random_images(78, [crop] * 2)
    val = [(torch.from_numpy(a).permute(2, 0, 1).float().div(255) * 0.4, b) for a, b in zip(lows, highs)]
    assert len(batches()) == 3
    at = 2
    kw = dict(nEpochs=4, lr=2e-4, warmup_epochs=1, snapshots=2, max_grad_norm=1.0, accum_steps=2, ema_decay=0.999,
              val_weights="both", val_pairs=val)
    with pytest.raises(ValueError):
        P.fit(_model(dev, SMALL), batches(), **{**kw, "ema_decay": None})
    full = P.fit(_model(dev, SMALL), batches(), out_dir=str(tmp_path / "a"), **kw)
    assert all(r["steps"] == 2 and r["skipped"] == 0 and np.isfinite(r["loss"]) for r in full)
    assert all(("psnr_ema" in r) == ("psnr" in r) == (r["epoch"] % 2 == 0) for r in full)
    first = []

    class Stop(Exception):
        pass

    def stop_there(rec):
        first.append(rec)
        if rec["epoch"] == at:
            raise Stop

    with pytest.raises(Stop):
        P.fit(_model(dev, SMALL), batches(), out_dir=str(tmp_path / "b"), on_epoch=stop_there, **kw)
    rest = P.fit(_model(dev, SMALL, seed=5), batches(), out_dir=str(tmp_path / "b"),
                 resume=str(tmp_path / "b" / f"epoch_{at}.train.pt"), **kw)
    assert first + rest == full, (first + rest, full)
    for name in ("epoch_4.pth", "epoch_4.ema.pth"):
        wa, wb = _load(tmp_path / "a" / name), _load(tmp_path / "b" / name)
        assert wa.keys() == wb.keys() and all(_same(wa[k], wb[k]) for k in wa), name
    sa, sb = _load(tmp_path / "a" / "epoch_4.train.pt")["trainer"], _load(tmp_path / "b" / "epoch_4.train.pt")["trainer"]
    for k in ("exp_avg", "exp_avg_sq", "ema"):
        assert sa[k].keys() == sb[k].keys() and all(_same(sa[k][n], sb[k][n]) for n in sa[k]), k
    assert sa["steps_applied"] == sb["steps_applied"] == 8 and not any(n.startswith("I_LCA5") for n in sa["ema"])
    fresh = _model(dev, SMALL, seed=9)
    fresh.load_state_dict(_load(tmp_path / "a" / "epoch_4.ema.pth"), strict=True)
    res = P.evaluate(fresh, val)
    assert (full[-1]["psnr_ema"], full[-1]["ssim_ema"]) == (res.psnr, res.ssim)
    wm, we = _load(tmp_path / "a" / "epoch_4.pth"), _load(tmp_path / "a" / "epoch_4.ema.pth")
    assert any(not torch.equal(wm[k], we[k]) for k in wm)


# ---- two ranks sharing the GPU over gloo ----------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


K2 = 2


def _micro(world):
    """(ranks, passes) micro-batches for two updates: the second reuses the first's data"""
    g = torch.Generator().manual_seed(5)
    x = torch.rand(world, K2, *SHAPE_SMALL, generator=g) * 0.6 + 0.05
    return x, torch.rand(world, K2, *SHAPE_SMALL, generator=g)


def _rank_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, ROOT)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from hvi_cidnet_amd.dp import DataParallelTrainer
    dev = torch.device("cuda:0")
    tr = DataParallelTrainer(_model(dev, SMALL, seed=7), lr=1e-4, n_buckets=4, accum_steps=K2, ema_decay=0.9)
    x, gt = _micro(world)
    x, gt = x[rank].to(dev), gt[rank].to(dev)
    for j in range(K2):
        tr.step(x[j], gt[j])
    torch.cuda.synchronize()
    g_mean = (tr.flat_g[:tr.n_live] / (world * K2)).cpu().numpy().copy()
    for j in range(K2):
        tr.step(x[j], gt[j])
    torch.cuda.synchronize()
    q.put((rank, g_mean, tr.flat_p.cpu().numpy().copy(), tr.ema.cpu().numpy().copy(), len(tr.buckets)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_accumulate_on_one_gpu_match_one_rank():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r, *rest = q.get(timeout=500)
        res[r] = rest
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert res[0][3] >= 2
    for i in range(3):                                   # the reduced gradient, the parameters, the average: bit-equal
        assert np.array_equal(res[0][i].view(np.int32), res[1][i].view(np.int32)), i
    assert not np.array_equal(res[0][1], res[0][2]) and np.isfinite(res[0][2]).all()
    # one rank, K = 4, the same four micro-batches: the summed gradient of the first update, to the tolerance of
    # tests/test_dp_two_ranks_gpu.py for the same comparison
    from hvi_cidnet_amd.dp import DataParallelTrainer
    dev = torch.device("cuda:0")
    one = DataParallelTrainer(_model(dev, SMALL, seed=7), lr=1e-4, n_buckets=4, accum_steps=world * K2, ema_decay=0.9)
    x, gt = _micro(world)
    for r in range(world):
        for j in range(K2):
            one.step(x[r, j].to(dev), gt[r, j].to(dev))
    torch.cuda.synchronize()
    ref = (one.flat_g[:one.n_live] / (world * K2)).cpu()
    d = (torch.from_numpy(res[0][0]) - ref).abs().max().item()
    assert d <= 2e-5 * ref.abs().max().item() + 1e-9, (d, ref.abs().max().item())
