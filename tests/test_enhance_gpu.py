"""GPU: enhance_u8 (ingest -> model -> egress), enhance_folder (the pipelined folder driver) and evaluate(save_dir=) with the
reduced-width model -- every output byte equals to_uint8 of the model's own output on the restated input, the model is left
as it was found, the files do not depend on batch size / threads / depth, and a corrupt file stops the pipeline with its name.

Every case runs in a fresh spawned process (tests/evaluate_harness.py: in_child)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from evaluate_harness import in_child as _in_child, model as _model  # noqa: E402
from test_evaluate_gpu import SIZES, _pairs  # noqa: E402

pytestmark = pytest.mark.gpu
CFGS = [dict(gamma=1.0, gated=False, alpha_s=1.3, gated2=False, alpha=1.0),
        dict(gamma=1.4, gated=True, alpha_s=1.2, gated2=True, alpha=0.9)]
EXTS = [".png", ".png", ".bmp", ".png", ".jpg", ".png"]


def _images(sizes, seed=21):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 160, size=(h, w, 3), dtype=np.uint8) for h, w in sizes]


def _reference(m, img, gamma, gated, alpha_s, gated2, alpha):
    """to_uint8(model(ref_x)) of one (h,w,3) uint8 array, permuted: the chain a caller wrote by hand before enhance_u8"""
    import hvi_cidnet_amd as P
    t = m.trans
    old = (t.gated, t.alpha_s, t.gated2, t.alpha)
    modes = [(mod, mod.training) for mod in m.modules()]
    m.eval()
    t.gated, t.alpha_s, t.gated2, t.alpha = gated, alpha_s, gated2, alpha
    dev = torch.device("cuda:0")
    u8 = torch.from_numpy(img)
    with torch.no_grad():
        if gamma == 1.0:
            x = u8.permute(2, 0, 1).float().div(255).unsqueeze(0).to(dev)
        else:
            x = torch.from_numpy(P.gamma_table(gamma))[u8.long()].permute(2, 0, 1).unsqueeze(0).to(dev)
        xp, (h, w) = P.pad_to_multiple(x, 8)
        y = m(xp)
        y = y[0] if isinstance(y, tuple) else y
        q = P.metrics.to_uint8(y, (h, w)).permute(0, 2, 3, 1).contiguous()
    t.gated, t.alpha_s, t.gated2, t.alpha = old
    for mod, mode in modes:
        mod.training = mode
    return q[0].cpu().numpy()


@pytest.mark.parametrize("cfg", CFGS)
def test_enhance_u8_matches_the_hand_written_chain_and_restores_the_model(dev, cfg):
    _in_child(_case_enhance_u8, "CIDNet", cfg)


def test_enhance_u8_tnsm(dev):
    _in_child(_case_enhance_u8, "CIDNet_TNSM", CFGS[1])


def _case_enhance_u8(cls_name, cfg):
    import hvi_cidnet_amd as P
    dev = torch.device("cuda:0")
    m = _model(cls_name)
    imgs = _images(SIZES[:4])
    t = m.trans
    t.gated, t.alpha_s, t.gated2, t.alpha = False, 1.1, False, 0.7
    m.train()
    m.HV_LCA1.eval()                                                        # a mixed-mode module tree comes back as it was
    modes = [mod.training for mod in m.modules()]
    refs = [_reference(m, a, **cfg) for a in imgs]
    k_state = (t._this_k_host, t._this_k_dev)                               # the snapshot the reference runs left behind
    for a, ref in zip(imgs, refs):
        q = P.enhance_u8(m, torch.from_numpy(a).to(dev), **cfg)
        assert q.shape == (1, *a.shape) and q.dtype == torch.uint8
        assert np.array_equal(q[0].cpu().numpy(), ref)
        assert [mod.training for mod in m.modules()] == modes
        assert (t.gated, t.alpha_s, t.gated2, t.alpha) == (False, 1.1, False, 0.7)
        assert t._this_k_host == k_state[0] and t._this_k_dev is k_state[1]
    if cls_name == "CIDNet":           # the two (36,52) images as one batch: bit-equal, as test_batch_sizes_agree pins for this model
        q2 = P.enhance_u8(m, torch.from_numpy(np.stack(imgs[:2])).to(dev), **cfg)
        assert np.array_equal(q2.cpu().numpy(), np.stack(refs[:2]))
    assert m.training and not m.HV_LCA1.training


def _write_inputs(folder, imgs):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    names = [f"im{i}{e}" for i, e in enumerate(EXTS)]
    for a, n in zip(imgs, names):
        Image.fromarray(a).save(os.path.join(folder, n))
    return names


def test_enhance_folder(dev, tmp_path):
    _in_child(_case_folder, str(tmp_path))


def _case_folder(tmp):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd.metrics import _read_rgb
    dev = torch.device("cuda:0")
    m = _model()
    cfg = CFGS[1]
    src, out_a, out_b = (os.path.join(tmp, d) for d in ("in", "out_a", "out_b"))
    names = _write_inputs(src, _images(SIZES))
    rep = P.enhance_folder(m, src, out_a, batch_size=4, threads=4, depth=2, **cfg)
    assert rep.names == sorted(names) == names
    assert rep.sizes == [tuple(s) for s in SIZES]
    assert sorted(i for b in rep.batches for i in b) == list(range(len(names))) and all(len(b) <= 4 for b in rep.batches)
    assert rep.batches[0] == [0, 1]                                          # equal sizes share a batch, a new size starts one
    assert rep.seconds["wall"] > 0 and 0 <= rep.seconds["wait_for_slot"] <= rep.seconds["wall"]
    assert sorted(os.listdir(out_a)) == names
    for n, (h, w) in zip(names, SIZES):
        got = _read_rgb(os.path.join(out_a, n))
        assert got.shape == (h, w, 3)
        if not n.endswith(".jpg"):                                           # lossless: the bytes enhance_u8 gives for the decoded input
            ref = P.enhance_u8(m, torch.from_numpy(_read_rgb(os.path.join(src, n))).to(dev), **cfg)[0].cpu().numpy()
            assert np.array_equal(got, ref), n
    rep_b = P.enhance_folder(m, src, out_b, batch_size=1, threads=1, depth=1, **cfg)   # the serial order
    assert rep_b.names == names and rep_b.batches == [[i] for i in range(len(names))]
    for n in names:
        if not n.endswith(".jpg"):
            with open(os.path.join(out_a, n), "rb") as fa, open(os.path.join(out_b, n), "rb") as fb:
                assert fa.read() == fb.read(), n
    assert m.training and m.trans.alpha == 1.0


def test_enhance_folder_stops_on_a_corrupt_file(dev, tmp_path):
    _in_child(_case_corrupt, str(tmp_path))


def _case_corrupt(tmp):
    import faulthandler
    import hvi_cidnet_amd as P
    faulthandler.dump_traceback_later(60, exit=True)                        # a hang ends the child here, with every thread's stack
    m = _model()
    src = os.path.join(tmp, "in")
    _write_inputs(src, _images(SIZES))
    with open(os.path.join(src, "x.png"), "wb") as f:                       # sorts last: the pipeline is running when it is met
        f.write(b"\x89PNG not an image")
    for kw in (dict(batch_size=2, threads=4, depth=2), dict(batch_size=1, threads=1, depth=1)):
        with pytest.raises(RuntimeError, match="x.png"):
            P.enhance_folder(m, src, os.path.join(tmp, "out"), **kw)
    faulthandler.cancel_dump_traceback_later()
    assert m.training


def test_evaluate_saves_what_it_scores(dev, tmp_path):
    _in_child(_case_save_dir, str(tmp_path))


def _case_save_dir(tmp):
    import hvi_cidnet_amd as P
    from hvi_cidnet_amd.metrics import _read_rgb
    dev = torch.device("cuda:0")
    m = _model()
    pairs, _ = _pairs()
    cfg = dict(gamma=1.2, gated=True, alpha_s=1.2, gated2=True, alpha=0.9)
    plain = P.evaluate(m, pairs, batch_size=4, **cfg)
    saved = P.evaluate(m, pairs, batch_size=4, save_dir=os.path.join(tmp, "saved"), **cfg)
    assert saved == plain
    assert sorted(os.listdir(os.path.join(tmp, "saved"))) == [f"{i:05d}.png" for i in range(len(pairs))]
    t = m.trans
    m.eval()
    t.gated, t.alpha_s, t.gated2, t.alpha = cfg["gated"], cfg["alpha_s"], cfg["gated2"], cfg["alpha"]
    with torch.no_grad():
        for i, (low, _) in enumerate(pairs):
            x, (h, w) = P.pad_to_multiple(low.unsqueeze(0).to(dev), 8)
            q = P.metrics.to_uint8(m(x ** cfg["gamma"]), (h, w))[0].permute(1, 2, 0).cpu().numpy()
            assert np.array_equal(_read_rgb(os.path.join(tmp, "saved", f"{i:05d}.png")), q), i
    with pytest.raises(ValueError, match="sweep"):
        P.evaluate(m, pairs, alpha=[0.9, 1.0], save_dir=os.path.join(tmp, "sweep"))
    assert not os.path.exists(os.path.join(tmp, "sweep"))
