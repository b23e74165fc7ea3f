"""What tests/test_evaluate_gpu.py and tests/test_evaluate_unpaired_gpu.py share: the reduced-width model with the oracle's
parameters, a runner that executes one case in a fresh spawned process, and a launcher of two gloo ranks.

Every case runs in a child: the models, trainers and captured graphs built there -- a trainer is never freed (its gradient
hooks sit on the model's parameters) -- stay out of the pytest process, whose later tests capture graphs of their own.  The
case functions live in the test modules and are passed as they are: under `spawn` the child imports their module by name."""
import os
import queue
import socket
import sys
import traceback

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import cidnet_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CHANS = (12, 12, 24, 48)


def model(cls_name="CIDNet", seed=5):
    import hvi_cidnet_amd as P
    m = getattr(P, cls_name)(channels=list(CHANS))
    variant = {"CIDNet": "base", "CIDNet_MSSA": "mssa", "CIDNet_TNSM": "tnsm"}[cls_name]
    p = O.make_params(seed, channels=CHANS, variant=variant)
    m.load_state_dict({k: p[k] for k in m.state_dict().keys()})
    return m.to("cuda:0")


def _child(fn, args, q):
    try:
        q.put((True, fn(*args)))
    except BaseException:
        q.put((False, traceback.format_exc()))


def in_child(fn, *args):
    """fn(*args) in a fresh spawned process; returns its result, or fails the test with the child's traceback"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_child, args=(fn, args, q))
    p.start()
    res = None
    try:
        for _ in range(100):                                     # <= 500 s; stop waiting once the child has died
            try:
                res = q.get(timeout=5)
                break
            except queue.Empty:
                if not p.is_alive():
                    break
    finally:
        p.join(120)
    assert res is not None and p.exitcode == 0, f"child process exit code {p.exitcode}"
    ok, val = res
    if not ok:
        pytest.fail(val, pytrace=False)
    return val


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, fn, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    q.put((rank, fn()))
    dist.barrier()
    dist.destroy_process_group()


def two_ranks(fn):
    """fn() on two ranks that share the GPU over gloo -> {rank: its result}"""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, world, port, fn, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        r, v = q.get(timeout=500)
        got[r] = v
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    return got
