"""GPU: the trainer's raw_input (hvi-cidnet_amd/dp.py) -- the low image before `** gamma`, which train_tnsm.py:55,68 keeps for
the noise-consistency term while the network is fed the powered one: routing to a wants_input loss function, fit.run_epoch
passing a batch's third element on, refusal with a loss function that takes no input, and the hipGraph path.  Reduced-width
models, as tests/test_trainer_gpu.py uses them."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import data_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CHANS, SIZE = (12, 12, 24, 48), (32, 48)
SIZES = [(37, 51), (40, 60), (64, 64), (33, 49), (40, 60), (37, 51)]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _pairs(dev, seed=61):
    import hvi_cidnet_amd as P
    lows, highs = R.random_images(seed, SIZES), R.random_images(seed + 1000, SIZES)
    return P.ResidentPairs(lows, highs, dev), lows, highs


def _batches(dev, n, gamma=0.7):
    """n batches (x, gt, raw) of shape (2,3,32,48) from the batch kernel: x = raw ** gamma"""
    import hvi_cidnet_amd as P
    pairs, _, _ = _pairs(dev)
    rng = np.random.default_rng(3)
    out = []
    for _ in range(n):
        index = rng.integers(0, len(SIZES), size=2).tolist()
        y0 = [int(rng.integers(0, SIZES[i][0] - 32 + 1)) for i in index]
        x0 = [int(rng.integers(0, SIZES[i][1] - 48 + 1)) for i in index]
        out.append(P.crop_flip(pairs, index, y0, x0, [0, 1], [1, 0], SIZE, gamma=gamma, raw=True))
    return out


@pytest.fixture(scope="module")
def tnsm_state():
    import hvi_cidnet_amd as P
    torch.manual_seed(3)
    return {k: v.clone() for k, v in P.CIDNet_TNSM(channels=list(CHANS)).state_dict().items()}


def _tnsm(dev, state):
    import hvi_cidnet_amd as P
    m = P.CIDNet_TNSM(channels=list(CHANS))
    m.load_state_dict(state)
    return m.to(dev).train()


def test_raw_input_reaches_the_tnsm_loss(dev, tnsm_state):
    """(A) step(x, gt, raw_input=raw) ends bit-identical to (B) step(x, gt) under a wrapper that hands the same loss im1=raw,
    and differs from (C) step(x, gt), whose noise terms see the powered input"""
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd.dp import DataParallelTrainer
    batches = _batches(dev, 2)
    assert not torch.equal(batches[0][0], batches[0][2])
    finals = {}
    for which in "ABC":
        m = _tnsm(dev, tnsm_state)
        lf = P.CIDNetLoss(m, tnsm_weight=1.0).to(dev)
        now = {}

        def wrapped(out, gt, _lf=lf, _now=now):
            return _lf(out, gt, im1=_now["raw"])
        tr = DataParallelTrainer(m, lr=1e-3, loss_fn=wrapped if which == "B" else lf)
        for x, gt, raw in batches:
            now["raw"] = raw
            if which == "A":
                tr.step(x, gt, raw_input=raw)
            else:
                tr.step(x, gt)
        torch.cuda.synchronize()
        assert torch.isfinite(tr.flat_p).all()
        finals[which] = tr.flat_p.clone()
    assert torch.equal(_bits(finals["A"]), _bits(finals["B"]))
    assert not torch.equal(_bits(finals["A"]), _bits(finals["C"]))


def test_run_epoch_hands_the_third_element_to_the_step(dev, tnsm_state):
    """one epoch of fit.run_epoch over TrainBatches(raw=True, gamma=(60, 120)) ends bit-identical to the same steps taken by
    hand with the (x, gt, raw) of the restatement (tests/data_ref.py) built on the host from the epoch's plan"""
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd.fit import run_epoch
    from hvi_cidnet_amd.dp import DataParallelTrainer, StepLog
    pairs, lows, highs = _pairs(dev)
    tb = P.TrainBatches(pairs, 2, SIZE, seed=5, gamma=(60, 120), raw=True)
    p = tb.plan(1)
    assert len(tb) == len(p.batches) == 3
    finals = []
    for source in ("run_epoch", "hand"):
        m = _tnsm(dev, tnsm_state)
        log = StepLog(len(tb))
        tr = DataParallelTrainer(m, lr=1e-3, loss_fn=P.CIDNetLoss(m, tnsm_weight=1.0).to(dev), step_log=log)
        if source == "run_epoch":
            rows = run_epoch(tr, tb, 1, log)
            assert rows.shape[0] == 3
        else:
            log.reset()
            for k, (lo, hi) in enumerate(p.batches):
                cols = [c[lo:hi].tolist() for c in (p.index, p.y0, p.x0, p.hflip, p.vflip)]
                raw, gt = R.batch(lows, highs, None, *cols, SIZE)
                x = torch.from_numpy(P.gamma_table(p.gammas[k]))[torch.round(raw * 255).long()]
                tr.step(x.to(dev), gt.to(dev), raw_input=raw.to(dev))
        torch.cuda.synchronize()
        finals.append(tr.flat_p.clone())
    assert torch.equal(_bits(finals[0]), _bits(finals[1]))


def test_raw_input_is_refused_by_a_loss_that_takes_no_input(dev):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd.dp import DataParallelTrainer
    (x, gt, raw), = _batches(dev, 1)
    tr = DataParallelTrainer(P.CIDNet(channels=list(CHANS)).to(dev), lr=1e-3)
    with pytest.raises(ValueError, match="raw_input"):
        tr.step(x, gt, raw_input=raw)
    with pytest.raises(ValueError, match="raw_input"):
        tr.forward_backward(x, gt, raw_input=raw)
    assert not tr._ready                                         # refused before the probing pass: nothing was launched


class _L1ToBoth:
    """a small wants_input loss: L1(out, gt) + L1(out, im1)"""
    wants_input = True

    def __init__(self):
        import hvi_cidnet_amd as P
        self.l1 = P.L1Loss()

    def __call__(self, out, gt, im1=None):
        return self.l1(out, gt) + self.l1(out, im1)


def test_graph_replays_with_a_raw_input_and_recaptures_without(dev):
    """three steps with a different raw_input each: use_graph=True ends bit-identical to eager (the raw input has a static
    buffer that is refreshed before every replay); a fourth step without raw_input recaptures and still equals eager"""
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd.dp import DataParallelTrainer
    batches = _batches(dev, 4)
    torch.manual_seed(4)
    state = {k: v.clone() for k, v in P.CIDNet(channels=list(CHANS)).state_dict().items()}
    res = []
    for use_graph in (False, True):
        m = P.CIDNet(channels=list(CHANS))
        m.load_state_dict(state)
        tr = DataParallelTrainer(m.to(dev), lr=1e-3, loss_fn=_L1ToBoth(), use_graph=use_graph)
        losses = [float(tr.step(x, gt, raw_input=raw).item()) for x, gt, raw in batches[:3]]
        torch.cuda.synchronize()
        after3 = tr.flat_p.clone()
        captured = tr._graph
        x, gt, _ = batches[3]
        losses.append(float(tr.step(x, gt).item()))
        torch.cuda.synchronize()
        if use_graph:
            assert captured is not None and tr._graph is not None and tr._graph is not captured and tr._graw is None
        res.append((losses, after3, tr.flat_p.clone()))
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert torch.equal(_bits(res[0][1]), _bits(res[1][1])) and torch.equal(_bits(res[0][2]), _bits(res[1][2]))
    assert not torch.equal(_bits(res[0][1]), _bits(res[0][2]))
