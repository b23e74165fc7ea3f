"""Data-parallel training step for CIDNet: one process per GPU, RCCL (torch.distributed backend
"nccl") over xGMI, gradients all-reduced in a few flat buckets that overlap with the backward.

The reference trains on a single GPU (train.py:34 pins CUDA_VISIBLE_DEVICES='0') and has no
distributed code; this harness restates its step semantics (train.py:56-73: forward, loss,
zero_grad, backward, Adam.step) for N ranks:

  * parameters live in ONE flat fp32 buffer (the modules' Parameters are views into it); weight
    gradients are written by the HIP backward kernels straight into the matching flat gradient
    buffer (the trainer's ops.grad_arena), so there is no per-tensor packing before communication;
  * the flat gradient buffer is cut into `n_buckets` contiguous buckets.  Parameters are laid out
    in the order in which their gradients become ready (learned from one probing backward), so
    bucket b is complete while the backward of earlier layers is still running; its all-reduce is
    launched from a post-accumulate-grad hook and runs on RCCL's stream concurrently;
  * the message is small (7.9 MB for CIDNet) and xGMI is point-to-point, so the collective is
    latency-bound: few large buckets, never one collective per tensor;
  * after the last bucket lands, one fused Adam kernel updates the flat parameter buffer
    (1/world_size folded into the gradient scale).

Parameters that receive no gradient (the reference's dead I_LCA5.* block, SURVEY.md quick fact 1)
are detected in the probing backward and left out of buckets and optimizer, as torch.optim does
for grad=None parameters.  Nothing here is CIDNet-specific: any nn.Module works, which is what the
gloo/CPU tests use.
"""
from __future__ import annotations

from typing import Callable, List, Optional

import contextlib
import math
import os

import torch
import torch.distributed as dist


def _default_loss(out, gt):
    from . import ops
    return ops.L1LossFn.apply(out, gt)


class FlatAdam:
    """torch.optim.Adam semantics on one flat buffer; `kernel` selects the fused HIP update.

    max_grad_norm / skip_nonfinite / device_state: any of them selects the device-state path -- the step count lives on the
    device (`state`: applied, skipped), and every step runs the guard first (ops.grad_guard: fp64 norm of the averaged
    gradient, clip_grad_norm_'s coefficient, skip when the gradient holds a NaN or an Inf and skip_nonfinite is set), then an
    Adam update that reads the guard's record; nothing of it reaches the host.  With all three off this is the plain update
    with a host step count.  kernel=False restates the same decisions in torch (CPU tests; it synchronises).

    ema_decay: keep `ema`, an exponential moving average of the whole buffer (a copy of flat_p at construction): after every
    Adam launch, on the same stream, ema += w * (p - ema) over the live part with w = fp32(1 - decay) (ops.ema_update; three
    fp32 roundings).  On the device-state path the launch reads the guard's record, so a skipped step leaves the average
    where it is.
    accum_steps > 1: the optimizer also owns `acc`, the buffer the passes of an accumulated update are summed in, and
    accumulate(), the one operation on it (dst = src or dst += src, ops.grad_accumulate); the trainer decides when."""

    def __init__(self, flat_p, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, kernel: bool = True,
                 max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False, device_state: bool = False,
                 accum_steps: int = 1, ema_decay: Optional[float] = None):
        self.p = flat_p
        self.accum_steps = int(accum_steps)
        if self.accum_steps < 1:
            raise ValueError("accum_steps must be at least 1")
        if self.accum_steps > 1:
            self.acc = torch.zeros_like(flat_p)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        if self.ema_decay is not None:
            self.ema_w = ema_weight(self.ema_decay)
            self.ema = flat_p.detach().clone()
        self.m = torch.zeros_like(flat_p)
        self.v = torch.zeros_like(flat_p)
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.t = 0
        self.kernel = kernel
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = bool(device_state) or self.skip_nonfinite or max_grad_norm is not None
        if self.guarded:
            self.state = torch.zeros(2, dtype=torch.int64, device=flat_p.device)       # steps applied, steps skipped
            self.record = torch.zeros(4, dtype=torch.float32, device=flat_p.device)    # apply, scale, 1 - b1^t, sqrt(1 - b2^t)

    def _clips(self):
        c = self.max_grad_norm
        return c is not None and c > 0 and c != float("inf")

    def steps_applied(self) -> int:
        """updates applied so far (device-state path: reads the device, so it waits for the queued steps)"""
        return int(self.state[0].item()) if self.guarded else self.t

    def steps_skipped(self) -> int:
        """steps the guard skipped so far (synchronises as steps_applied)"""
        return int(self.state[1].item()) if self.guarded else 0

    def set_counts(self, applied: int, skipped: int = 0):
        if self.guarded:
            self.state.copy_(torch.tensor([int(applied), int(skipped)], dtype=torch.int64))
        else:
            self.t = int(applied)

    def step(self, flat_g, n_live: int, grad_scale: float = 1.0, loss=None, log_row=None):
        """loss (the step's scalar) and log_row (a device address for the kernel path, a (4,) fp64 tensor for the torch
        restatement) only matter on the device-state path: the guard writes loss, norm, coef and the signed count there."""
        b1, b2 = self.betas
        p, g, m, v = self.p[:n_live], flat_g[:n_live], self.m[:n_live], self.v[:n_live]
        if self.guarded:
            return self._guarded_step(p, g, m, v, grad_scale, loss, log_row)
        self.t += 1
        if self.kernel:
            from . import ops
            ops.adam_step(p, g, m, v, self.lr, b1, b2, self.eps, self.wd, self.t, grad_scale)
        else:
            # plain-torch restatement of the same update (used by the CPU/gloo tests of the harness only)
            self._torch_update(p, g, m, v, grad_scale, self.t)
        self._ema_update(n_live, None)

    def _ema_update(self, n_live, record, applied=True):
        """the average follows the update that was just launched: same stream, behind the Adam kernel"""
        if self.ema_decay is None:
            return
        e, p = self.ema[:n_live], self.p[:n_live]
        if self.kernel:
            from . import ops
            ops.ema_update(e, p, self.ema_w, record)
        elif applied:
            e.add_((p - e).mul_(self.ema_w))           # three roundings, as the kernel: difference, product, sum

    def accumulate(self, dst, src, first: bool):
        """dst = src (first) or dst += src, one rounding per element, on the current stream"""
        if self.kernel:
            from . import ops
            ops.grad_accumulate(dst, src, first)
        elif first:
            dst.copy_(src)
        else:
            dst.add_(src)

    def swap_ema(self):
        """exchange p and ema in place (whole buffers: the dead tail is the same on both sides)"""
        if self.kernel:
            from . import ops
            ops.swap(self.p, self.ema)
        else:
            t = self.p.clone()
            self.p.copy_(self.ema)
            self.ema.copy_(t)

    def _torch_update(self, p, g, m, v, gscale, t):
        b1, b2 = self.betas
        g = g * gscale
        if self.wd:
            g = g + self.wd * p
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        bc1 = 1 - b1 ** t
        bc2 = 1 - b2 ** t
        p.sub_((self.lr / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + self.eps)))

    def _guarded_step(self, p, g, m, v, grad_scale, loss, log_row):
        b1, b2 = self.betas
        if self.kernel:
            from . import ops
            if loss is not None and not (loss.is_cuda and loss.dtype == torch.float32 and loss.numel() == 1):
                raise RuntimeError("the guarded step logs a scalar fp32 device loss")
            ops.grad_guard(g, grad_scale, self.max_grad_norm if self._clips() else None, self.skip_nonfinite, b1, b2, loss,
                           self.state, self.record, log_row)
            ops.adam_step_dev(p, g, m, v, self.lr, b1, b2, self.eps, self.wd, self.record)
            self._ema_update(p.numel(), self.record)
            return
        # plain-torch restatement of the guard's decisions (CPU/gloo tests; reads the sum on the host)
        ss = float(g.double().pow(2).sum().item())
        norm = math.sqrt(ss) * grad_scale if ss == ss and ss >= 0 else float("nan")
        coef = 1.0
        if self._clips():
            coef = self.max_grad_norm / (norm + 1e-6)
            if coef > 1.0:
                coef = 1.0
        apply = math.isfinite(ss) or not self.skip_nonfinite
        self.state[0 if apply else 1] += 1
        applied = int(self.state[0].item())
        if log_row is not None:
            log_row.copy_(torch.tensor([float(loss) if loss is not None else float("nan"), norm, coef,
                                        applied if apply else -(applied + 1)], dtype=torch.float64))
        if apply:
            self._torch_update(p, g, m, v, grad_scale * coef, applied)
        self._ema_update(p.numel(), None, applied=apply)


def ema_weight(decay) -> float:
    """w = fp32(1 - decay), the difference formed in double: the factor of ema += w * (p - ema)"""
    import ctypes
    d = float(decay)
    if not 0.0 <= d < 1.0:
        raise ValueError(f"ema_decay must be in [0, 1) (got {decay!r})")
    return ctypes.c_float(1.0 - d).value


class StepLog:
    """A (capacity, 4) fp64 device buffer the guarded step writes one row into: loss, gradient norm, clip coefficient, and
    the applied-step count after the step (negative, -(count + 1), when the step was skipped).  Step i since the last
    reset() writes row i % capacity; the row index is a host integer -- the host knows how many steps it issued whether or
    not they were applied.  read() is the only transfer: one device-to-host copy."""
    LOSS, NORM, COEF, COUNT = 0, 1, 2, 3

    def __init__(self, capacity: int):
        self.capacity = int(capacity)
        if self.capacity <= 0:
            raise ValueError("StepLog: capacity must be positive")
        self.buf = None
        self.issued = 0

    def bind(self, device):
        """allocate the buffer on `device` (the trainer does this when it builds its arena)"""
        if self.buf is None or self.buf.device != torch.device(device):
            self.buf = torch.zeros((self.capacity, 4), dtype=torch.float64, device=device)
        return self

    def reset(self):
        self.issued = 0

    def next_row(self):
        """-> the row tensor of the step that is issued now"""
        row = self.buf[self.issued % self.capacity]
        self.issued += 1
        return row

    def read(self):
        """rows written since reset() (the last `capacity` of them when more were issued), in step order, as a numpy array"""
        import numpy as np
        n = min(self.issued, self.capacity)
        if n == 0 or self.buf is None:
            return np.zeros((0, 4), dtype=np.float64)
        rows = self.buf[:n].cpu().numpy()
        if self.issued > self.capacity:
            rows = np.roll(rows, -(self.issued % self.capacity), axis=0)
        return rows


def tensor_stats_plan(offsets, lengths, n, device, kernel: Optional[bool] = None):
    """-> the plan ops.tensor_stats takes for the segments (offsets[t], lengths[t]) of a flat fp32 buffer of n elements on
    `device`: tile table and segment arrays uploaded once, workspace owned.  kernel None: the HIP kernel on a GPU, the
    plain-torch restatement on the CPU; False: the restatement everywhere."""
    from . import ops
    return ops.TensorStatsPlan(offsets, lengths, n, device, kernel)


class TensorLog:
    """Beside StepLog: a (capacity, len(what), T, 4) fp64 device ring of per-tensor statistics (ops.tensor_stats: norm, maxabs,
    nonfinite, first), one row per update, written on the stream of the update immediately before the guard.  what: "grad"
    (the gradient the guard sees, with the guard's scale) and / or "weight" (the weights that produced it, scale 1).  T and
    `names` -- the live parameters in arena order -- are only known when the trainer builds its arena, which binds the
    log.  Update i since the last reset() writes row i % capacity; the index is a host integer, the same as the StepLog
    row's.  read() is the only transfer: one device-to-host copy."""
    NORM, MAXABS, NONFINITE, FIRST = 0, 1, 2, 3
    WHAT = ("grad", "weight")

    def __init__(self, capacity: int, what=("grad", "weight")):
        self.capacity = int(capacity)
        if self.capacity <= 0:
            raise ValueError("TensorLog: capacity must be positive")
        self.what = tuple(what)
        if not self.what or len(set(self.what)) != len(self.what) or any(w not in self.WHAT for w in self.what):
            raise ValueError(f"TensorLog: what must be a non-empty choice of {self.WHAT} (got {what!r})")
        self.buf = None
        self.names = None
        self.issued = 0

    def bind(self, device, names):
        """allocate the ring on `device` for the tensors `names` (the trainer does this when it builds its arena)"""
        names = tuple(names)
        if self.buf is None or self.buf.device != torch.device(device) or names != self.names:
            self.buf = torch.zeros((self.capacity, len(self.what), len(names), 4), dtype=torch.float64, device=device)
            self.names = names
        return self

    def reset(self):
        self.issued = 0

    def next_row(self):
        """-> the (len(what), T, 4) tensor of the update that is issued now"""
        row = self.buf[self.issued % self.capacity]
        self.issued += 1
        return row

    def read(self):
        """rows written since reset() (the last `capacity` of them when more were issued), in step order, as a numpy array
        (rows, len(what), T, 4)"""
        import numpy as np
        n = min(self.issued, self.capacity)
        if n == 0 or self.buf is None:
            return np.zeros((0, len(self.what), len(self.names or ()), 4), dtype=np.float64)
        rows = self.buf[:n].cpu().numpy()
        if self.issued > self.capacity:
            rows = np.roll(rows, -(self.issued % self.capacity), axis=0)
        return rows

    def first_nonfinite(self, row, what="grad"):
        """row: one row of read(), (len(what), T, 4).  -> (tensor index, name, element index) of the first tensor in arena
        order that holds a non-finite element, or None.  Arena order is gradient-ready order: for "grad" this is the
        parameter nearest the loss among the affected ones (DESIGN 6.16 for what that does and does not prove)."""
        stats = row[self.what.index(what)]
        for t in range(stats.shape[0]):
            if stats[t, self.NONFINITE] > 0:
                return t, self.names[t], int(stats[t, self.FIRST])
        return None


def rank_cpu_set(cpus, local_rank: int, local_world: int):
    """The contiguous share of `cpus` (sorted ids) that local rank `local_rank` of `local_world` ranks on this node gets:
    equal chunks, the remainder to the first ranks; every rank at least one CPU (ranks then share when CPUs are fewer)."""
    cpus = sorted(cpus)
    n = len(cpus)
    if local_world <= 1 or n == 0:
        return list(cpus)
    if n < local_world:
        return [cpus[local_rank % n]]
    base, rem = divmod(n, local_world)
    lo = local_rank * base + min(local_rank, rem)
    return cpus[lo:lo + base + (1 if local_rank < rem else 0)]


def pin_rank_to_cpus(local_rank: Optional[int] = None, local_world: Optional[int] = None) -> Optional[List[int]]:
    """One process per GPU: give every local rank its own slice of the CPUs this job may use (sched_setaffinity) and size
    torch's intra-op pool to it.  Without it the N enqueue threads (13 ms of Python per 26 ms step each) and their helper
    threads migrate over all cores and evict each other.  LOCAL_RANK / LOCAL_WORLD_SIZE from the launcher are the
    defaults; CIDNET_CPU_AFFINITY=0 disables.  Returns the CPU list that was set (None when nothing was done)."""
    if os.environ.get("CIDNET_CPU_AFFINITY", "1") == "0" or not hasattr(os, "sched_setaffinity"):
        return None
    lr = int(os.environ.get("LOCAL_RANK", "0")) if local_rank is None else local_rank
    lw = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1"))) if local_world is None else local_world
    if lw <= 1:
        return None
    mine = rank_cpu_set(os.sched_getaffinity(0), lr, lw)
    os.sched_setaffinity(0, mine)
    torch.set_num_threads(max(1, min(len(mine), 8)))
    return mine


class DataParallelTrainer:
    def __init__(self, model: torch.nn.Module, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, n_buckets: int = 4, loss_fn: Optional[Callable] = None,
                 process_group=None, use_hip_kernels: bool = True, wgrad_stream: bool = True, use_graph: bool = False,
                 max_steps_in_flight: int = 3, max_queued_bytes: Optional[int] = None,
                 prepared_weights: Optional[bool] = None, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False, step_log: Optional[StepLog] = None, accum_steps: int = 1,
                 ema_decay: Optional[float] = None, tensor_log: Optional["TensorLog"] = None):
        """max_grad_norm / skip_nonfinite / step_log: the guarded step (FlatAdam's device-state path).  The guard runs after
        the all-reduce, where every rank holds the same gradient, so every rank takes the same decision without talking;
        step_log (a StepLog) receives one row per step.

        accum_steps = K > 1: step() is called once per micro-batch and every K-th call applies one update from the sum of the
        K gradients, added in fp32 in pass order, with grad_scale 1 / (world * K); the first K - 1 calls launch no
        collective, the K-th one all-reduce per bucket.  A micro-batch's gradient is the gradient of its OWN mean loss, so a
        short last batch weighs as much as a full one.  The step log gets one row per update (the loss: the fp32 sum of the
        passes' losses in pass order, times fp32(1 / K)); pending_passes, flush().
        ema_decay: an exponential moving average of the weights, updated on the device behind every Adam launch and left
        alone by a step the guard skips (FlatAdam); ema_state_dict(), ema_weights().
        tensor_log (a TensorLog): per-tensor statistics of every update's gradient (the buffer and the scale the guard gets,
        after the all-reduce, so every rank logs the same rows) and / or of the weights that produced it, launched on the
        update's stream immediately before the guard (unguarded: before Adam); one row per update, the StepLog row's index.
        With the defaults none of the three adds a launch, a value or a state_dict key."""
        self.model = model
        self.tensor_log = tensor_log
        self._stats_plan = None
        self.accum_steps = int(accum_steps)
        if self.accum_steps < 1:
            raise ValueError("accum_steps must be at least 1")
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        if self.ema_decay is not None:
            ema_weight(self.ema_decay)               # range check now, not at the first step
        self._passes = 0                             # passes of the open accumulation group
        self._comm_pass = True                       # this pass's buckets are all-reduced as they complete ...
        self._fold_pass = False                      # ... after they took the earlier passes' sum (step() sets both)
        self._in_ema = False                         # inside ema_weights(): flat_p holds the average
        self.step_log = step_log
        self.prepared_weights = (os.environ.get("CIDNET_PREPARED_WEIGHTS", "1") == "1") if prepared_weights is None else bool(prepared_weights)
        # Back-pressure.  Nothing in a training step synchronises host and device, and the host enqueues a step in ~13 ms
        # while the GPU needs ~31 ms.  Root cause of the multi-second stalls of round 1 (tools/stall_probe.py,
        # profiles/r02_stall_probe_*.txt): every tensor the host frees after it was used on a side stream
        # (record_stream) stays "active" in the caching allocator until the GPU reaches that point, so nothing of a
        # still-queued step can be reused -- each queued step pins ~6 GiB, and the allocator hipMallocs that much in NEW
        # segments per step the host is ahead (reserved memory 30 -> 130 GiB over 24 unthrottled steps, 20-40 device
        # mallocs per step, single hipMalloc calls of 60 ms once the queue is deep; at ~45 steps ahead the 288 GB are
        # gone and the allocator falls into its synchronise-free-retry path).  Bounding the run-ahead removes the cause;
        # the bound is in steps AND in bytes the allocator holds for queued work, so a configuration with more launches
        # or larger activations per step (TNSM, the full objective, bigger batches) is covered as well.
        # Three steps, not two: a queue of two steps (62 ms of work) is drained by an ordinary 65 ms host hiccup.
        self.max_steps_in_flight = max(1, int(max_steps_in_flight))
        # None: a third of the device's memory, resolved at the first step (96 GiB on a 288 GB MI355X)
        self.max_queued_bytes = None if max_queued_bytes is None else int(max_queued_bytes)
        self._step_events = []
        self.loss_fn = loss_fn or _default_loss
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        # rehearsal switch: run the bucket all-reduces even on a 1-rank group (exercises the RCCL path on one GPU)
        self._force_comm = dist.is_initialized() and os.environ.get("CIDNET_DP_FORCE_ALLREDUCE") == "1"
        self.rank = dist.get_rank(process_group) if dist.is_initialized() else 0
        self.n_buckets = max(1, n_buckets)
        self.use_hip = use_hip_kernels
        # weight-gradient GEMMs on a third stream (they feed nothing but the optimizer): 35.9 -> 34.4 ms/step at
        # bs=8 400x600 -- the data-gradient chain of short, latency-bound launches no longer waits behind them
        self.wgrad_stream = wgrad_stream
        self._opt_args = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                              skip_nonfinite=skip_nonfinite, device_state=step_log is not None)
        self._pending_state = None
        self._ready = False
        self._handles: List = []
        self._launch_stream = None
        self._main_stream = None
        # replay forward + loss + backward as ONE hipGraph (captured over all three streams) instead of ~700 launches
        # issued from Python: at bs=8 about 5 ms of every 34 ms step are launch-bound phases (the 50x75 level)
        self.use_graph = use_graph
        self._graph = None
        self._graw = None
        self._capturing = False
        # gradient arena and prepared-weight cache of this trainer (set up in _setup), installed for its passes only
        self._arena = None
        self._prep = None
        self.params = [p for p in model.parameters() if p.requires_grad]

    # ---- one-time setup: probe gradient order, flatten, hook -----------------------------------
    def _setup(self, x, gt, raw_input=None):
        # 1) probing backward: which parameters get gradients, in which order, and how often
        order, fired = [], {}
        hooks = []
        for p in self.params:
            def h(param, _p=p):
                if id(_p) not in fired:
                    fired[id(_p)] = 0
                    order.append(_p)
                fired[id(_p)] += 1
            hooks.append(p.register_post_accumulate_grad_hook(h))
        ln_uses = [m._use for m in self.model.modules() if hasattr(m, "_use")] if self.use_hip else []
        if self.use_hip:
            from . import ops
            ops.start_grad_probe()
            for st in ln_uses:
                st.acc, st.fwd, st.bwd, st.probe = False, 0, 0, [0, 0]
        self.model.zero_grad(set_to_none=True)
        with self._pass_scope():                    # no arena, no cache yet
            loss = self._loss(self.model(x), gt, x, raw_input)
            loss.backward()
        for h in hooks:
            h.remove()
        # a parameter whose gradient is produced by several kernel launches per step (LayerNorm affine:
        # 3 uses per LCA) must be summed by autograd, not written in place
        counts = ops.stop_grad_probe() if self.use_hip else {}
        multi_ids = {id(p) for p in self.params if counts.get(p.data_ptr(), 0) > 1}
        # LayerNorm modules applied several times per step whose every forward use came back in the probing backward: their
        # uses sum the weight / bias gradients in place in the arena (ops.LNUse), so they count as arena parameters
        ln_acc_ids = set()
        for m in (self.model.modules() if self.use_hip else ()):
            st = getattr(m, "_use", None)
            if st is not None and st.probe[0] > 0 and st.probe[0] == st.probe[1]:
                st.acc, st.fwd, st.bwd = True, 0, 0
                ln_acc_ids.update((id(m.weight), id(m.bias)))
        multi_ids -= ln_acc_ids
        # single-use parameters whose gradient a kernel writes in place into the arena, possibly on the weight-gradient stream
        self._arena_ids = {id(p) for p in self.params if counts.get(p.data_ptr(), 0) == 1} | ln_acc_ids
        self.model.zero_grad(set_to_none=True)
        live = order
        dead = [p for p in self.params if id(p) not in fired]
        # 2) flat buffers in gradient-ready order; dead parameters parked at the tail
        layout = live + dead
        n_live = sum(p.numel() for p in live)
        n_all = sum(p.numel() for p in layout)
        dev = layout[0].device
        flat_p = torch.empty(n_all, device=dev, dtype=torch.float32)
        self.flat_g = torch.zeros(n_all, device=dev, dtype=torch.float32)
        off = 0
        self._slices = {}
        for p in layout:
            n = p.numel()
            flat_p[off:off + n].copy_(p.data.reshape(-1))
            p.data = flat_p[off:off + n].view(p.shape)
            self._slices[id(p)] = (off, n)
            off += n
        self.flat_p, self.n_live = flat_p, n_live
        # identical initial weights on every rank
        if self.world > 1 or self._force_comm:
            dist.broadcast(self.flat_p, src=0, group=self.pg)
        # 3) buckets: contiguous, roughly equal, cut at parameter boundaries
        target = (n_live + self.n_buckets - 1) // self.n_buckets
        self.buckets, cur_start, cur_n, members = [], 0, 0, []
        for p in live:
            members.append(p)
            cur_n += p.numel()
            if cur_n >= target and len(self.buckets) < self.n_buckets - 1:
                self.buckets.append((cur_start, cur_n, members))
                cur_start += cur_n
                cur_n, members = 0, []
        if members:
            self.buckets.append((cur_start, cur_n, members))
        self._bucket_of = {}
        for bi, (_, _, mem) in enumerate(self.buckets):
            for p in mem:
                self._bucket_of[id(p)] = bi
        self._pending = [0] * len(self.buckets)
        self._ln_uses = [st for st in ln_uses if st.acc]
        self._check_layout_across_ranks(layout, n_live)
        # 4) gradients written in place by the HIP backward kernels (single-use parameters only)
        multi = [p.data_ptr() for p in live if id(p) in multi_ids]      # pointers AFTER re-homing into flat_p
        if self.use_hip:
            from . import ops
            self._arena = ops.grad_arena(self.flat_p, self.flat_g, exclude_ptrs=multi)
            ops.enable_wgrad_stream(self.wgrad_stream)
            # this trainer's fused Adam is the only writer of flat_p: inside its passes (_pass_scope) prepared (split,
            # fragment-ordered) weight operands are kept across launches in its own cache, and re-prepared in two launches
            # after every update (_weights_changed); anything else that writes the weights without torch's version counter
            # seeing it (p.data.copy_, raw kernels) must call weights_changed()
            self._prep = ops.PreparedWeights() if self.prepared_weights else None
        for p in live:
            p.register_post_accumulate_grad_hook(self._on_grad)
        # after the broadcast: the average starts as a copy of the weights every rank holds
        self.opt = FlatAdam(self.flat_p, kernel=self.use_hip, accum_steps=self.accum_steps, ema_decay=self.ema_decay,
                            **self._opt_args)
        if self.accum_steps > 1:
            self._loss_acc = torch.zeros(1, device=dev, dtype=torch.float32)     # the open group's loss sum
            self._loss_mean = torch.zeros(1, device=dev, dtype=torch.float32)    # what the guard logs for the update
        if self.step_log is not None:
            self.step_log.bind(dev)
        if self.tensor_log is not None:
            named = self._live_named()
            self._stats_plan = tensor_stats_plan([r[1] for r in named], [r[2] for r in named], n_live, dev, kernel=self.use_hip)
            self.tensor_log.bind(dev, [r[0] for r in named])
        self._ready = True
        if self._pending_state is not None:
            state, self._pending_state = self._pending_state, None
            self._apply_state(state)

    def _check_layout_across_ranks(self, layout, n_live):
        """Every rank derives the arena layout from its OWN probing backward (gradient-ready order).  The order is a
        property of the graph, so it is the same everywhere -- but if it ever were not (a data-dependent branch, another
        library version on one node), the all-reduce would silently add different parameters into each other.  Rank 0
        broadcasts a digest of (parameter name, offset, size) in layout order plus the bucket cuts; a mismatch raises."""
        if not (self.world > 1 or self._force_comm):
            return
        import hashlib
        names = {id(p): n for n, p in self.model.named_parameters()}
        h = hashlib.sha256()
        for p in layout:
            off, n = self._slices[id(p)]
            h.update(f"{names.get(id(p), '?')}:{off}:{n};".encode())
        h.update(f"live={n_live};buckets={[(s0, c) for s0, c, _ in self.buckets]}".encode())
        mine = torch.tensor(list(h.digest()), dtype=torch.int64, device=self.flat_g.device)
        ref = mine.clone()
        dist.broadcast(ref, src=0, group=self.pg)
        same = torch.equal(mine.cpu(), ref.cpu())
        flag = torch.tensor([0 if same else 1], dtype=torch.int64, device=self.flat_g.device)
        dist.all_reduce(flag, op=dist.ReduceOp.SUM, group=self.pg)
        if int(flag.item()) != 0:
            raise RuntimeError(f"rank {self.rank}: gradient-arena layout differs between ranks "
                               f"({'this rank differs from rank 0' if not same else 'another rank differs'}); "
                               "the bucket all-reduce would mix parameters")

    def _begin_pass(self, x):
        """state every forward+backward starts from: all gradients of every bucket pending, no collective in flight, and
        the in-place LayerNorm gradient counters at zero -- a stray grad-mode forward without a backward (validation
        without no_grad, model(x) for logging, an exception between forward and backward) would otherwise leave
        `fwd` ahead of `bwd` for good and the LayerNorm gradients would never be handed over again."""
        for bi, (_, _, mem) in enumerate(self.buckets):
            self._pending[bi] = len(mem)
        self._handles = []
        self._main_stream = torch.cuda.current_stream() if x.is_cuda else None
        for st in self._ln_uses:
            st.fwd = st.bwd = 0

    def _end_pass(self):
        """every live parameter's gradient must have arrived in the arena (and its bucket been launched)"""
        if any(self._pending):
            missing = [i for i, n in enumerate(self._pending) if n]
            raise RuntimeError(f"backward left gradients pending in buckets {missing}: a parameter that received a gradient "
                               "in the probing step got none now (graph changed?), or a LayerNorm's uses were not all "
                               "run backward")

    def _join_wgrad_stream(self):
        """make the current stream wait for the weight-gradient stream (ops._offload_wgrad)"""
        if self.use_hip:
            from . import ops
            torch.cuda.current_stream().wait_stream(ops.wgrad_stream(self.flat_g.device))

    def _on_grad(self, p):
        off, n = self._slices[id(p)]
        slot = self.flat_g[off:off + n]
        if p.grad.data_ptr() != slot.data_ptr():
            # multi-use parameters and gradients not produced through grad_like() (summed / allocated by autograd on the
            # branch streams) -- or a single-use arena gradient that autograd cloned instead of stealing: that one may
            # still be in flight on the weight-gradient stream, so the copy waits for it (never seen in practice;
            # without the wait it would read a stale gradient)
            if self.use_hip and self.wgrad_stream and p.grad.is_cuda and id(p) in self._arena_ids:
                self._join_wgrad_stream()
            slot.copy_(p.grad.reshape(-1))
        p.grad = None                               # the arena is the single home of gradients
        bi = self._bucket_of[id(p)]
        self._pending[bi] -= 1
        if self._pending[bi] == 0 and (self.world > 1 or self._force_comm) and not self._capturing and self._comm_pass:
            self._launch_bucket(bi)

    def _launch_bucket(self, bi):
        """All-reduce one finished bucket without stalling the compute streams.  The bucket's gradients were written
        by kernels on up to three streams (the two branch streams and the weight-gradient stream) and this hook only
        runs in CPU order, so the collective is issued from a dedicated launch stream that first waits for the
        current tail of every producer stream; RCCL orders its own stream after the launch stream.
        In the last pass of an accumulated update the bucket first takes the sum of the earlier passes (flat_acc, complete
        since the previous pass's accumulate on the main stream, which the launch stream waits for as a producer), on the
        launch stream and in front of the collective: one all-reduce per bucket per update, still overlapped."""
        start, cnt, _ = self.buckets[bi]
        dev = self.flat_g.device
        fold = self._fold_pass                    # earlier passes of this update wait in flat_acc
        if dev.type != "cuda":                    # gloo / CPU rehearsal: no streams
            if fold:
                self.opt.accumulate(self.flat_g[start:start + cnt], self.opt.acc[start:start + cnt], first=False)
            self._handles.append(dist.all_reduce(self.flat_g[start:start + cnt], op=dist.ReduceOp.SUM, group=self.pg,
                                                 async_op=True))
            return
        if self._launch_stream is None:
            self._launch_stream = torch.cuda.Stream(device=dev)
        st = self._launch_stream
        producers = [torch.cuda.current_stream(), self._main_stream, getattr(self.model, "_side_stream", None)]
        if self.use_hip and self.wgrad_stream:
            from . import ops
            producers.append(ops.wgrad_stream(dev))
        for ps in producers:
            if ps is not None:
                st.wait_stream(ps)
        with torch.cuda.stream(st):
            if fold:
                self.opt.accumulate(self.flat_g[start:start + cnt], self.opt.acc[start:start + cnt], first=False)
            self._handles.append(dist.all_reduce(self.flat_g[start:start + cnt], op=dist.ReduceOp.SUM, group=self.pg,
                                                 async_op=True))

    def set_lr(self, lr: float):
        """learning rate of the fused Adam from the next step on (see schedule.WarmupCosineLR)"""
        self._opt_args["lr"] = float(lr)
        if getattr(self, "opt", None) is not None:
            self.opt.lr = float(lr)

    # ---- hipGraph replay of forward + loss + backward ---------------------------------------------
    def _backward(self, loss):
        """loss.backward() with a cached unit gradient: autograd would otherwise launch an ATen fill for its implicit
        ones_like(loss) every step (the step launches only cidnet:: kernels, tests/test_trainer_gpu.py)"""
        one = getattr(self, "_unit_grad", None)
        if one is None or one.device != loss.device or one.dtype != loss.dtype or one.shape != loss.shape:
            one = self._unit_grad = torch.ones_like(loss)
        loss.backward(gradient=one)

    def _pass_scope(self):
        """this trainer's arena and prepared-weight cache, installed for one pass; the previous ones come back after it"""
        if not self.use_hip:
            return contextlib.nullcontext()
        from . import ops
        return ops.installed(self._arena, self._prep)

    def _check_raw(self, raw_input):
        if raw_input is not None and not getattr(self.loss_fn, "wants_input", False):
            raise ValueError("raw_input was given, but the loss function takes no input image (no true `wants_input` "
                             "attribute, as losses.CIDNetLoss has): it would be dropped")

    def _loss(self, out, gt, x, raw_input=None):
        """loss_fn(model(x), gt); a loss function with a true `wants_input` attribute (losses.CIDNetLoss: the TNSM noise terms
        compare the output with the low image, train_tnsm.py:68-69) also gets im1: raw_input where the caller has one (the
        low image before `** gamma`, as train_tnsm.py:55,68 keeps it), else the network input x.  Tuple results of the
        model (CIDNet_TNSM in train mode) are handed to the loss function as they are."""
        if getattr(self.loss_fn, "wants_input", False):
            return self.loss_fn(out, gt, im1=raw_input if raw_input is not None else x)
        return self.loss_fn(out, gt)

    def _fwd_bwd(self, x, gt, raw_input=None):
        with self._pass_scope():
            self._begin_pass(x)
            loss = self._loss(self.model(x), gt, x, raw_input)
            self._backward(loss)
            self._end_pass()
        return loss

    def _capture(self, x, gt, raw_input=None):
        """Static input buffers (the raw input's too, where the call has one), two eager passes on the capture stream
        (scratch buffers reach their final size), then
        capture.  The side stream of the model and the weight-gradient stream fork from / join the capture stream
        exactly as in eager mode, so the graph keeps the three-stream concurrency.  Collectives and Adam stay outside
        (Adam's bias correction is a host scalar that changes every step)."""
        self._gx, self._ggt = x.clone(), gt.clone()
        self._graw = raw_input.clone() if raw_input is not None else None
        st = torch.cuda.Stream(device=x.device)
        st.wait_stream(torch.cuda.current_stream())
        self._capturing = True
        try:
            with torch.cuda.stream(st):
                for _ in range(2):
                    self._fwd_bwd(self._gx, self._ggt, self._graw)
                    self._join_wgrad_stream()
            torch.cuda.current_stream().wait_stream(st)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                loss = self._fwd_bwd(self._gx, self._ggt, self._graw)
                self._join_wgrad_stream()
                self._gloss = loss.detach()
            self._graph = g
            self._graph_clears = self._prep.clears if self._prep is not None else 0
        finally:
            self._capturing = False

    def _graph_step(self, x, gt, raw_input=None):
        self._graph_replay(x, gt, raw_input)
        if self.world > 1 or self._force_comm:
            dist.all_reduce(self.flat_g[:self.n_live], op=dist.ReduceOp.SUM, group=self.pg)
        self._opt_step(self._gloss)
        self._weights_changed()          # the captured pass reads prepared operands that the eager passes before it created
        return self._gloss

    def _graph_replay(self, x, gt, raw_input=None):
        """forward + loss + backward by replay (captured first where needed); gradients in flat_g, the loss in _gloss"""
        # the graph reads the prepared operands' buffers: recapture once they were dropped, and re-prepare them when a
        # weight was written through torch since the last step (load_state_dict)
        if self._graph is not None and self._prep is not None:
            if self._prep.clears != self._graph_clears:
                self._graph = None
            elif self._prep.stale():
                self._prep.refresh(self.flat_p.device)
        if self._graph is not None and (raw_input is None) != (self._graw is None):
            self._graph = None               # captured with / without a raw input: the loss reads another buffer
        if self._graph is None:
            self._capture(x, gt, raw_input)
        self._gx.copy_(x)
        self._ggt.copy_(gt)
        if raw_input is not None:
            self._graw.copy_(raw_input)
        self._graph.replay()

    # ---- the step ---------------------------------------------------------------------------------
    def step(self, x, gt, raw_input=None):
        """forward, loss, backward (+ overlapped bucket all-reduce), fused Adam.  Returns the loss.  raw_input: what a
        `wants_input` loss function gets as im1 in place of x (the low image before the gamma power, train_tnsm.py:55,68;
        data.TrainBatches(raw=True) yields it); ValueError with a loss function that takes no input."""
        self._check_raw(raw_input)
        if self._in_ema:
            raise RuntimeError("step() inside ema_weights(): the model holds the averaged weights")
        if not self._ready:
            self._setup(x, gt, raw_input)
        if x.is_cuda:
            while len(self._step_events) >= self.max_steps_in_flight:
                self._step_events.pop(0).synchronize()
            # bytes pinned for queued work = "active" (in use or waiting for a stream event) minus what the host still holds;
            # only looked at while more than one step is queued (the stats call walks the allocator's counters)
            if self.max_queued_bytes is None:
                self.max_queued_bytes = torch.cuda.get_device_properties(x.device).total_memory // 3
            while len(self._step_events) > 1 and self._queued_bytes(x.device) > self.max_queued_bytes:
                self._step_events.pop(0).synchronize()
        if self.accum_steps > 1:
            loss = self._accum_pass(x, gt, raw_input)
        elif self.use_graph and x.is_cuda:
            loss = self._graph_step(x, gt, raw_input)
        else:
            loss = self._fwd_bwd(x, gt, raw_input)
            for h in self._handles:
                h.wait()
            self._join_wgrad_stream()
            self._opt_step(loss)
            self._weights_changed()          # also after a skipped step: the host cannot know and must not ask
            loss = loss.detach()
        if x.is_cuda:
            ev = torch.cuda.Event()
            ev.record()
            self._step_events.append(ev)
        return loss

    def _opt_step(self, loss, flat_g=None, passes: int = 1):
        """fused Adam on the arena; guarded: the guard's two launches first, fed the loss tensor the step returns.
        flat_g / passes: the buffer that holds the summed gradient of an accumulated update and how many passes it sums."""
        flat_g = self.flat_g if flat_g is None else flat_g
        scale = 1.0 / (self.world * passes)
        if self.tensor_log is not None:
            self._log_tensors(flat_g, scale)
        if not self.opt.guarded:
            self.opt.step(flat_g, self.n_live, grad_scale=scale)
            return
        row = self.step_log.next_row() if self.step_log is not None else None
        if row is not None and self.opt.kernel:
            row = row.data_ptr()
        self.opt.step(flat_g, self.n_live, grad_scale=scale, loss=loss.detach(), log_row=row)

    def _log_tensors(self, flat_g, scale):
        """the update's row of the tensor log: two launches per entry of its `what`, on the current stream"""
        from . import ops
        row, n = self.tensor_log.next_row(), self.n_live
        for i, what in enumerate(self.tensor_log.what):
            if what == "grad":
                ops.tensor_stats(flat_g[:n], self._stats_plan, scale, out=row[i])
            else:
                ops.tensor_stats(self.flat_p[:n], self._stats_plan, 1.0, out=row[i])

    # ---- gradient accumulation --------------------------------------------------------------------------
    @property
    def pending_passes(self) -> int:
        """passes of the open accumulation group (0: no group is open)"""
        return self._passes

    @property
    def flat_acc(self):
        """the sum of the open group's passes (accum_steps > 1, after the first step)"""
        return self.opt.acc

    @property
    def ema(self):
        """the flat average, laid out as flat_p (ema_decay set, after the first step)"""
        return self.opt.ema

    def _accum_pass(self, x, gt, raw_input):
        """One micro-batch of an accumulated update.  Passes 1 .. K-1: forward, loss, backward without a collective, then
        flat_acc (+)= flat_g and the loss sum on the current stream, behind the join with the weight-gradient stream.  Pass
        K: its buckets take flat_acc on the launch stream before their all-reduce (one rank: flat_g += flat_acc behind the
        join), then guard and Adam with 1 / (world * K).  The sum handed on is fl(..fl(fl(g1 + g2) + g3).. + gK)."""
        K, n = self.accum_steps, self.n_live
        last = self._passes == K - 1
        comm = self.world > 1 or self._force_comm
        graph = self.use_graph and x.is_cuda
        self._comm_pass, self._fold_pass = last, last
        try:
            if graph:
                self._graph_replay(x, gt, raw_input)
                loss = self._gloss
            else:
                loss = self._fwd_bwd(x, gt, raw_input)
                for h in self._handles:
                    h.wait()
                self._join_wgrad_stream()
        finally:
            self._comm_pass, self._fold_pass = True, False
        loss = loss.detach()
        self.opt.accumulate(self._loss_acc, loss.reshape(1), first=self._passes == 0)
        if not last:
            self.opt.accumulate(self.flat_acc[:n], self.flat_g[:n], first=self._passes == 0)
            self._passes += 1
            return loss
        if graph or not comm:                    # eager with ranks: every bucket took its share in _launch_bucket
            self.opt.accumulate(self.flat_g[:n], self.flat_acc[:n], first=False)
        if graph and comm:
            dist.all_reduce(self.flat_g[:n], op=dist.ReduceOp.SUM, group=self.pg)
        self._apply_update(self.flat_g, K)
        return loss

    def _apply_update(self, flat_g, passes):
        """guard + Adam (+ EMA) from the summed gradient of `passes` passes; the logged loss is their fp32 mean"""
        self._scale_loss(1.0 / passes)
        self._opt_step(self._loss_mean, flat_g=flat_g, passes=passes)
        self._passes = 0
        self._weights_changed()

    def _scale_loss(self, mult):
        if self.use_hip:
            from . import ops
            ops.scale_into(self._loss_mean, self._loss_acc, mult)
        else:
            torch.mul(self._loss_acc, mult, out=self._loss_mean)

    def flush(self):
        """Apply the open group of j < K passes as one update with grad_scale 1 / (world * j); on several ranks flat_acc is
        all-reduced in one collective.  Nothing happens without an open group.  Every rank must call it alike."""
        j, n = self._passes, self.n_live
        if j == 0:
            return
        if self.world > 1 or self._force_comm:
            dist.all_reduce(self.flat_acc[:n], op=dist.ReduceOp.SUM, group=self.pg)
        self._apply_update(self.flat_acc, j)

    # ---- optimizer state ----------------------------------------------------------------------------
    def _live_named(self):
        """(name, offset, numel, shape) of every parameter the optimizer updates, in arena order"""
        names = {id(p): n for n, p in self.model.named_parameters()}
        out = []
        for p in self.params:
            off, n = self._slices[id(p)]
            if off < self.n_live:
                out.append((names[id(p)], off, n, tuple(p.shape)))
        return sorted(out, key=lambda r: r[1])

    def state_dict(self):
        """Adam's state, keyed by parameter NAME (arena offsets follow the gradient-ready order probed at run time): exp_avg
        and exp_avg_sq per live parameter as CPU tensors, the applied / skipped step counts, lr, betas, eps, weight_decay.
        Parameters that get no gradient (I_LCA5.*) have no entry.  Synchronises."""
        if not self._ready:
            if self._pending_state is not None:
                return self._pending_state
            raise RuntimeError("state_dict: the optimizer exists after the first step (or after load_state_dict)")
        if self._passes:
            raise RuntimeError(f"state_dict: an accumulation group is open ({self._passes} of {self.accum_steps} passes); "
                               "finish it or flush() first")
        if self._in_ema:
            raise RuntimeError("state_dict inside ema_weights(): weights and average are exchanged")
        o = self.opt
        out = {"exp_avg": {n: o.m[off:off + c].view(shp).cpu().clone() for n, off, c, shp in self._live_named()},
               "exp_avg_sq": {n: o.v[off:off + c].view(shp).cpu().clone() for n, off, c, shp in self._live_named()},
               "steps_applied": o.steps_applied(), "steps_skipped": o.steps_skipped(), "lr": float(o.lr),
               "betas": tuple(float(b) for b in o.betas), "eps": float(o.eps), "weight_decay": float(o.wd)}
        if self.ema_decay is not None:
            out["ema"] = {n: o.ema[off:off + c].view(shp).cpu().clone() for n, off, c, shp in self._live_named()}
            out["ema_decay"] = self.ema_decay
        return out

    def load_state_dict(self, state):
        """Strict: the names must be exactly the live parameters, the shapes theirs.  Before the first step the state is
        checked against the model's names and shapes and applied once the arena exists; which parameters are live is only
        known then, so a missing or dead name raises there.  lr, betas, eps and weight decay are taken over at once.
        The average: with ema_decay set the state must carry "ema" (same names as exp_avg) and "ema_decay"; without it the
        state must carry neither.  The trainer keeps its own ema_decay."""
        for k in ("exp_avg", "exp_avg_sq", "steps_applied", "steps_skipped", "lr", "betas", "eps", "weight_decay"):
            if k not in state:
                raise KeyError(f"load_state_dict: missing entry '{k}'")
        if self.ema_decay is not None:
            for k in ("ema", "ema_decay"):
                if k not in state:
                    raise KeyError(f"load_state_dict: this trainer keeps an EMA (ema_decay={self.ema_decay}), the state has no '{k}'")
        elif "ema" in state or "ema_decay" in state:
            raise KeyError("load_state_dict: the state carries an EMA, this trainer was built without ema_decay")
        if self._passes:
            raise RuntimeError("load_state_dict: an accumulation group is open; finish it or flush() first")
        if self._in_ema:
            raise RuntimeError("load_state_dict inside ema_weights()")
        moments = ("exp_avg", "exp_avg_sq") + (("ema",) if self.ema_decay is not None else ())
        shapes = {n: tuple(p.shape) for n, p in self.model.named_parameters()}
        if "ema" in moments and set(state["ema"]) != set(state["exp_avg"]):
            raise KeyError("load_state_dict: ema and exp_avg name different parameters")
        for k in moments:
            for n, t in state[k].items():
                if n not in shapes:
                    raise KeyError(f"load_state_dict: {k} has an entry for '{n}', which is no parameter of the model")
                if tuple(t.shape) != shapes[n]:
                    raise ValueError(f"load_state_dict: {k}['{n}'] has shape {tuple(t.shape)}, the parameter {shapes[n]}")
        if set(state["exp_avg"]) != set(state["exp_avg_sq"]):
            raise KeyError("load_state_dict: exp_avg and exp_avg_sq name different parameters")
        # the hyper-parameters take effect now, so a set_lr() that follows this call wins in either order of events; the
        # moments and counts need the arena
        betas, eps, wd = tuple(float(b) for b in state["betas"]), float(state["eps"]), float(state["weight_decay"])
        self._opt_args.update(betas=betas, eps=eps, weight_decay=wd)
        if getattr(self, "opt", None) is not None:
            self.opt.betas, self.opt.eps, self.opt.wd = betas, eps, wd
        self.set_lr(state["lr"])
        if self._ready:
            self._apply_state(state)
        else:
            self._pending_state = state

    def _apply_state(self, state):
        live = self._live_named()
        want, got = {n for n, *_ in live}, set(state["exp_avg"])
        if want != got:
            raise KeyError(f"load_state_dict: missing {sorted(want - got)[:5]}, unexpected {sorted(got - want)[:5]} "
                           f"({len(want - got)} / {len(got - want)} names)")
        o = self.opt
        for n, off, c, shp in live:
            o.m[off:off + c].copy_(state["exp_avg"][n].reshape(-1))
            o.v[off:off + c].copy_(state["exp_avg_sq"][n].reshape(-1))
        o.set_counts(state["steps_applied"], state["steps_skipped"])
        if self.ema_decay is not None:
            for n, off, c, shp in live:
                o.ema[off:off + c].copy_(state["ema"][n].reshape(-1))
            o.ema[self.n_live:].copy_(self.flat_p[self.n_live:])      # the dead tail stays the copy of the weights

    # ---- the averaged weights -------------------------------------------------------------------------
    def _need_ema(self, what):
        if self.ema_decay is None:
            raise RuntimeError(f"{what}: this trainer was built without ema_decay")
        if not self._ready:
            raise RuntimeError(f"{what}: the average exists after the first step")

    def ema_state_dict(self):
        """The averaged model: the keys of model.state_dict(), CPU tensors; the trainer's parameters come from `ema` by the
        arena's slices (the ones that get no gradient as the copy of their weights), buffers and anything else are copied
        from the model.  Loads into a fresh model with strict=True.  Synchronises."""
        self._need_ema("ema_state_dict")
        if self._in_ema:
            raise RuntimeError("ema_state_dict inside ema_weights(): weights and average are exchanged")
        names = {n: p for n, p in self.model.named_parameters()}
        out = {}
        for k, v in self.model.state_dict().items():
            sl = self._slices.get(id(names[k])) if k in names else None
            if sl is None:
                out[k] = v.detach().cpu().clone()
            else:
                out[k] = self.opt.ema[sl[0]:sl[0] + sl[1]].view(v.shape).cpu().clone()
        return out

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside, the model computes with the averaged weights: `ema` and flat_p are exchanged in place (ops.swap: no
        third copy of the weights) and the prepared operands rebuilt; on exit, also after an exception, the same again, which
        restores both bit for bit.  Raises inside an open accumulation group; a training step inside raises."""
        self._need_ema("ema_weights")
        if self._passes:
            raise RuntimeError(f"ema_weights: an accumulation group is open ({self._passes} of {self.accum_steps} passes); "
                               "finish it or flush() first")
        if self._in_ema:
            raise RuntimeError("ema_weights: already inside")
        self.opt.swap_ema()
        self._weights_changed()
        self._in_ema = True
        try:
            yield self
        finally:
            self.opt.swap_ema()
            self._weights_changed()
            self._in_ema = False

    def _weights_changed(self):
        if self._prep is not None and self.flat_p.is_cuda:
            self._prep.refresh(self.flat_p.device)

    def weights_changed(self):
        """call after anything that writes the parameters outside torch's version tracking (p.data.copy_, raw kernels): the
        prepared weight operands are rebuilt.  load_state_dict / in-place torch ops are seen without it."""
        if self._ready:
            self._weights_changed()

    @staticmethod
    def _queued_bytes(device):
        st = torch.cuda.memory_stats_as_nested_dict(device)
        return st["active_bytes"]["all"]["current"] - st["allocated_bytes"]["all"]["current"]

    def forward_backward(self, x, gt, raw_input=None):
        """forward + loss + backward only (gradients left in the flat arena); for timing splits.  raw_input: as step()."""
        self._check_raw(raw_input)
        if not self._ready:
            self._setup(x, gt, raw_input)
        loss = self._fwd_bwd(x, gt, raw_input)
        for h in self._handles:
            h.wait()
        self._join_wgrad_stream()
        return loss.detach()
