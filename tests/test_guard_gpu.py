"""GPU: the guard in front of the fused Adam (csrc/guard.hip: cidnet_grad_guard, cidnet_adam_step_dev) and the guarded
step of dp.DataParallelTrainer.  Yardsticks: numpy in fp64 for the norm, torch.nn.utils.clip_grad_norm_ for the clip,
torch.optim.Adam for the update.  The poisoned steps below are NaN / Inf arithmetic in healthy kernels, not faults."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import cidnet_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL, SMALL = (36, 36, 72, 144), (12, 12, 24, 48)


def _model(dev, chans, seed=21):
    import hvi_cidnet_amd as P
    m = P.CIDNet(channels=list(chans))
    p = O.make_params(seed, channels=chans)
    m.load_state_dict({k: p[k] for k in m.state_dict().keys()})
    return m.to(dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Guard:
    """the raw entry point with buffers of its own"""

    def __init__(self, dev):
        self.state = torch.zeros(2, dtype=torch.int64, device=dev)
        self.record = torch.zeros(4, dtype=torch.float32, device=dev)
        self.row = torch.zeros(4, dtype=torch.float64, device=dev)

    def __call__(self, g, grad_scale=1.0, max_norm=None, skip=True, loss=None):
        from hvi_cidnet_amd import ops
        ops.grad_guard(g, grad_scale, max_norm, skip, 0.9, 0.999, loss, self.state, self.record, self.row.data_ptr())
        torch.cuda.synchronize()
        return self.row.cpu().numpy().copy(), self.record.cpu().numpy().copy(), self.state.cpu().numpy().copy()


@pytest.fixture(scope="module")
def real(dev):
    """the full-width trainer after one forward_backward: the real flat_g, n_live and parameter layout"""
    from hvi_cidnet_amd.dp import DataParallelTrainer
    shape = (2, 3, 64, 96)
    tr = DataParallelTrainer(_model(dev, FULL), lr=1e-3, n_buckets=3)
    tr.forward_backward(O.synthetic_batch(31, shape).to(dev), O.synthetic_batch(32, shape).to(dev))
    torch.cuda.synchronize()
    return tr


def _buffers(real, dev):
    n = real.n_live
    gen = torch.Generator().manual_seed(11)
    unit = torch.randn(n, generator=gen)
    out = [(f"normal x {s:g}", (unit * s).to(dev)) for s in (1e-4, 1.0, 30.0)]
    out.append(("flat_g", real.flat_g[:n].clone()))
    return out


def _norm64(g):
    a = g.cpu().numpy().astype(np.float64)
    return float(np.sqrt(np.sum(a ** 2)))


def test_norm_matches_fp64_and_repeats_bit_identically(real, dev):
    """Bound, derived: the squares are exact in fp64, the n - 1 additions lose at most (n - 1) 2^-53 = 2.2e-10 relative at
    n = 1.98 M, the root halves that and rounds once; 1e-9 leaves a factor of four."""
    guard = Guard(dev)
    assert real.n_live > 1_900_000
    for name, g in _buffers(real, dev):
        want = _norm64(g)
        row, rec, _ = guard(g)
        rel = abs(row[1] - want) / want
        print(f"norm [{name}]: kernel {row[1]:.17g}  numpy fp64 {want:.17g}  relative {rel:.3e}")
        assert rel <= 1e-9, (name, rel)
        row2, rec2, _ = guard(g)
        # norm, coefficient, decision and scale repeat bit for bit (the bias corrections follow the applied count, which grew)
        assert row[1:3].tobytes() == row2[1:3].tobytes() and rec[:2].tobytes() == rec2[:2].tobytes()
        assert row2[3] == row[3] + 1
        # a length that is no multiple of four, from an address that is no multiple of 16
        odd = g[1:real.n_live - 2]
        row3, _, _ = guard(odd)
        want3 = _norm64(odd)
        assert abs(row3[1] - want3) / want3 <= 1e-9
        # grad_scale multiplies the norm
        row4, _, _ = guard(g, grad_scale=0.5)
        assert abs(row4[1] - 0.5 * want) / want <= 1e-9
    assert guard.state.cpu().tolist() == [16, 0]


def test_clip_matches_clip_grad_norm(real, dev):
    """The gradient times the logged coefficient (the fp64 value of the log row, the product formed in fp64) against
    clip_grad_norm_ on per-parameter views of the same buffer.  torch forms its norm in fp32, so the bar comes from the
    buffer: torch's own relative distance from the fp64 norm, plus two fp32 roundings to nearest (2^-24 each, 2^-23
    together), relative and elementwise.  The fp32 scale the update reads is pinned separately: it is the logged coefficient
    rounded once.  (With the product formed in fp32 from that scale, one more rounding on each side, the same comparison gave
    1.573e-7 against a bar of 1.461e-7 on the unit-normal buffer, torch's norm being 2.7e-8 from fp64.)"""
    guard = Guard(dev)
    layout = real._live_named()
    assert len(layout) > 150
    for name, g in _buffers(real, dev):
        n64 = _norm64(g)
        max_norm = float(np.float32(0.37 * n64))
        row, rec, _ = guard(g, max_norm=max_norm)
        assert rec[1] == np.float32(row[2])                  # grad_scale = 1: the scale is the coefficient, rounded once
        ours = g.double() * float(row[2])
        twin = g.clone()
        params = []
        for _, off, c, shp in layout:
            p = torch.zeros(shp, device=dev, requires_grad=True)
            p.grad = twin[off:off + c].view(shp)
            params.append(p)
        n32 = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
        dist_t = abs(n32 - n64) / n64
        bar = dist_t + 2.0 ** -23
        nz = twin != 0
        rel = ((ours - twin.double()).abs()[nz] / twin.double().abs()[nz]).max().item()
        print(f"clip [{name}]: torch's norm is {dist_t:.3e} from fp64; clipped gradients differ by {rel:.3e} (bar {bar:.3e}); "
              f"coef {row[2]:.9g}")
        assert abs(row[2] - max_norm / (n64 + 1e-6)) <= 1e-9 * row[2]
        assert rec[0] == 1.0 and rel <= bar, (name, rel, bar)
        assert torch.equal((ours == 0), (twin == 0))
        # max_norm above the norm: coef is exactly 1; clipping off: coef 1 and the scale is grad_scale exactly
        row, rec, _ = guard(g, max_norm=float(np.float32(1.5 * n64)))
        assert row[2] == 1.0 and rec[1] == 1.0
        for off_value in (None, 0.0, -1.0, float("inf")):
            row, rec, _ = guard(g, grad_scale=0.25, max_norm=off_value)
            assert row[2] == 1.0 and rec[1] == np.float32(0.25)


def test_guard_decision_state_and_log(dev):
    """apply / skip, the two counts, the bias corrections of the new count and the signed count of the log row"""
    guard = Guard(dev)
    g = torch.linspace(-1, 1, 1001, device=dev)
    loss = torch.tensor(0.625, device=dev)
    bad = g.clone()
    bad[777] = float("nan")
    inf = g.clone()
    inf[1000] = float("-inf")
    applied = 0
    for buf, ok in ((g, True), (bad, False), (g, True), (inf, False), (g, True)):
        row, rec, st = guard(buf, loss=loss)
        applied += ok
        assert rec[0] == (1.0 if ok else 0.0) and row[0] == 0.625
        assert row[3] == (applied if ok else -(applied + 1))
        t = max(applied, 1)
        b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))          # the betas cross the ABI as fp32
        assert abs(rec[2] - (1 - b1 ** t)) <= 2.0 ** -24 and abs(rec[3] - (1 - b2 ** t) ** 0.5) <= 2.0 ** -24
    assert st.tolist() == [3, 2]
    # skip_nonfinite off: the step is applied whatever the sum is
    row, rec, st = guard(bad, skip=False)
    assert rec[0] == 1.0 and st.tolist() == [4, 2] and np.isnan(row[1]) and np.isnan(row[0])


def test_adam_step_dev_leaves_everything_alone_when_skipped(dev):
    from hvi_cidnet_amd import ops
    gen = torch.Generator().manual_seed(3)
    p, g, m, v = (torch.randn(5000, generator=gen).to(dev) for _ in range(4))
    v = v.abs() + 0.1
    keep = [t.clone() for t in (p, m, v)]
    rec = torch.tensor([0.0, 1.0, 0.1, 0.03], device=dev)
    ops.adam_step_dev(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.0, rec)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(keep, (p, m, v)))
    # applied: the arithmetic of cidnet_adam_step with the same scalars
    f = np.float32                                          # cidnet_adam_step forms its corrections in fp32 from fp32 betas
    rec = torch.tensor([1.0, 0.5, float(f(1) - np.power(f(0.9), f(3))), float(np.sqrt(f(1) - np.power(f(0.999), f(3))))],
                       device=dev)
    p2, m2, v2 = (t.clone() for t in keep)
    ops.adam_step_dev(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, rec)
    ops.adam_step(p2, g, m2, v2, 1e-3, 0.9, 0.999, 1e-8, 0.01, 3, 0.5)
    torch.cuda.synchronize()
    for a, b in ((p, p2), (m, m2), (v, v2)):
        assert torch.allclose(a, b, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("chans,shape", [(SMALL, (2, 3, 32, 48)), (FULL, (2, 3, 64, 96))])
def test_guarded_update_matches_torch_adam(dev, chans, shape):
    """Three consecutive guarded steps.  Before each the twin gets the harness's p, m, v and count, then the harness's own
    gradient times the logged coefficient (why its own: tests/test_trainer_gpu.py), and torch.optim.Adam's step must land on
    the harness's p, exp_avg, exp_avg_sq."""
    from hvi_cidnet_amd.dp import DataParallelTrainer, StepLog
    log = StepLog(8)
    tr = DataParallelTrainer(_model(dev, chans), lr=1e-3, n_buckets=3, max_grad_norm=0.05, skip_nonfinite=True, step_log=log)
    batches = [(O.synthetic_batch(31 + i, shape).to(dev), O.synthetic_batch(41 + i, shape).to(dev)) for i in range(3)]
    tr.forward_backward(*batches[0])                          # builds the arena; no update
    n = tr.n_live
    for i, (x, gt) in enumerate(batches):
        torch.cuda.synchronize()
        t = tr.flat_p[:n].clone().requires_grad_(True)
        opt = torch.optim.Adam([t], lr=1e-3)
        if i:
            opt.state[t] = {"step": torch.tensor(float(i)), "exp_avg": tr.opt.m[:n].clone(), "exp_avg_sq": tr.opt.v[:n].clone()}
        loss = tr.step(x, gt)
        torch.cuda.synchronize()
        row = log.read()[i]
        assert row[3] == i + 1 and row[0] == float(loss.item())
        t.grad = tr.flat_g[:n] * float(np.float32(row[2]))
        opt.step()
        print(f"step {i}: norm {row[1]:.6g} coef {row[2]:.6g}")
        for got, want, what in ((tr.flat_p[:n], t.detach(), "p"), (tr.opt.m[:n], opt.state[t]["exp_avg"], "exp_avg"),
                                (tr.opt.v[:n], opt.state[t]["exp_avg_sq"], "exp_avg_sq")):
            assert torch.allclose(got, want, atol=1e-7, rtol=1e-6), (i, what, (got - want).abs().max().item())
    assert tr.opt.steps_applied() == 3 and tr.opt.steps_skipped() == 0


@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_poisoned_step_is_skipped(dev, poison):
    from hvi_cidnet_amd import ops
    from hvi_cidnet_amd.dp import DataParallelTrainer, StepLog
    shape = (2, 3, 64, 96)
    batches = [(O.synthetic_batch(51 + i, shape).to(dev), O.synthetic_batch(61 + i, shape).to(dev)) for i in range(5)]
    factor = torch.ones((), device=dev)

    def loss_fn(out, gt):
        return ops.L1LossFn.apply(out, gt) * factor

    def run(bs, bad=None):
        factor.fill_(1.0)
        log = StepLog(8)
        tr = DataParallelTrainer(_model(dev, FULL), lr=1e-3, loss_fn=loss_fn, max_grad_norm=1.0, skip_nonfinite=True,
                                 step_log=log)
        across = None
        for i, (x, gt) in enumerate(bs):
            if i == bad:
                torch.cuda.synchronize()
                before = [t.clone() for t in (tr.flat_p, tr.opt.m, tr.opt.v)]
                factor.fill_(poison)
                tr.step(x, gt)
                factor.fill_(1.0)
                torch.cuda.synchronize()
                across = all(torch.equal(_bits(a), _bits(b)) for a, b in zip(before, (tr.flat_p, tr.opt.m, tr.opt.v)))
            else:
                tr.step(x, gt)
        torch.cuda.synchronize()
        return tr, log.read(), across

    tr, rows, across = run(batches, bad=2)
    assert across, "the skipped step changed p, m or v"
    assert (tr.opt.steps_applied(), tr.opt.steps_skipped()) == (4, 1)
    assert rows[:, 3].tolist() == [1, 2, -3, 3, 4] and not np.isfinite(rows[2, 1])
    assert torch.isfinite(tr.flat_p).all()
    ref, rows4, _ = run(batches[:2] + batches[3:])
    assert rows4[:, 3].tolist() == [1, 2, 3, 4]
    for a, b in ((tr.flat_p, ref.flat_p), (tr.opt.m, ref.opt.m), (tr.opt.v, ref.opt.v)):
        assert torch.equal(_bits(a), _bits(b))
    assert np.array_equal(rows[[0, 1, 3, 4], :3], rows4[:, :3])


def _foreign_kernels(trainer, x, gt, steps=1):
    """{kernel name: [aten op, ...]} of every launch of `steps` steps that is not a cidnet:: kernel"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            trainer.step(x, gt)
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


@pytest.mark.parametrize("two_streams", [True, False])
def test_guarded_step_launches_only_cidnet_kernels(dev, two_streams):
    from hvi_cidnet_amd.dp import DataParallelTrainer, StepLog
    shape = (2, 3, 64, 96)
    x, gt = O.synthetic_batch(41, shape).to(dev), O.synthetic_batch(42, shape).to(dev)
    m = _model(dev, FULL)
    m.two_streams = two_streams
    tr = DataParallelTrainer(m, lr=1e-3, wgrad_stream=two_streams, max_grad_norm=1.0, skip_nonfinite=True, step_log=StepLog(16))
    for _ in range(3):
        tr.step(x, gt)
    fk, ours = _foreign_kernels(tr, x, gt)
    assert not fk, {k: v[:3] for k, v in fk.items()}
    for want in ("sumsq_kernel", "guard_finish_kernel", "adam_dev_kernel"):
        assert any(want in k for k in ours), (want, sorted(ours)[:5])
    assert not any("adam_kernel" in k for k in ours)


# ---- two ranks sharing the GPU over gloo ----------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.path.insert(0, ROOT)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from hvi_cidnet_amd import ops
    from hvi_cidnet_amd.dp import DataParallelTrainer, StepLog
    dev = torch.device("cuda:0")
    factor = torch.ones((), device=dev)
    log = StepLog(8)
    tr = DataParallelTrainer(_model(dev, FULL, seed=7), lr=1e-4, n_buckets=4, loss_fn=lambda o, g: ops.L1LossFn.apply(o, g) * factor,
                             max_grad_norm=1.0, skip_nonfinite=True, step_log=log)
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand(4, world * 2, 3, 64, 96, generator=gen) * 0.6 + 0.05)[:, rank * 2:(rank + 1) * 2].to(dev)
    gt = torch.rand(4, world * 2, 3, 64, 96, generator=gen)[:, rank * 2:(rank + 1) * 2].to(dev)
    for i in range(4):
        if i == 1 and rank == 1:                     # only rank 1's loss is poisoned; rank 0 learns of it through the sum
            factor.fill_(float("nan"))
        tr.step(x[i], gt[i])
        factor.fill_(1.0)
    torch.cuda.synchronize()
    q.put((rank, tr.flat_p[:tr.n_live].cpu().numpy().copy(), tr.opt.steps_applied(), tr.opt.steps_skipped(),
           log.read()[:, 3].tolist()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_skip_together():
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
        r, p_, applied, skipped, counts = q.get(timeout=500)
        res[r] = (p_, applied, skipped, counts)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    for r in range(world):
        assert res[r][1:] == (3, 1, [1, -2, 2, 3]), res[r][1:]
    assert np.array_equal(res[0][0].view(np.int32), res[1][0].view(np.int32))
    assert np.isfinite(res[0][0]).all()
