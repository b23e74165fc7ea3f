"""Writes the NIQE fixtures tests/golden/niqe*.npz from the reference implementation (CPU only; run once, by hand):

    python tools/gen_niqe_golden.py --reference /path/to/HVI-CIDNet

The reference's loss/niqe_utils.py is imported with an empty stand-in registered as `cv2` (it uses cv2 only on its `gray`
path) and run, per input, exactly as measure_niqe_bris.py runs it: calculate_niqe(np.array(PIL RGB image)).  Its
intermediate values are captured by wrapping the functions it calls (imresize, compute_feature), not by restating them.
Per input i: the RGB input, the reference's cropped Y plane, its half-size image, both MSCN maps, the (blocks, 36)
feature matrix and the score.  niqe.npz also holds the SHA-256 of the reference's Y over all 2^24 RGB triples and the
figures the tests' bars are derived from (measured here with tests/niqe_ref.py):
  score_perturb   the largest change of the restatement's score when every moment is scaled by 1 +- 1e-12 at random;
  score_ref_diff  |restatement score - reference score| per input.
The generator refuses to write a set on which the restatement moves more than 1 % of an input's fits, or any by more
than one grid step.  Every file stays under 1 MiB: arrays are packed into niqe_img<i>.part<k>.npz greedily."""
import argparse
import hashlib
import io
import os
import shutil
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import niqe_ref as R  # noqa: E402

LIMIT = 1000000


def smooth_noise(seed, h, w):
    """uint8 (3,h,w): low-pass noise plus fine grain, so both tails of every block are populated"""
    rng = np.random.default_rng(seed)
    base = rng.random((3, h // 8 + 2, w // 8 + 2))
    up = np.kron(base, np.ones((8, 8)))[:, :h, :w]
    k = np.ones(9) / 9
    for ax in (1, 2):
        up = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), ax, up)
    img = up * 200 + 20 + rng.normal(0, 6, (3, h, w))
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


def inputs(ref_dir):
    from PIL import Image
    with Image.open(os.path.join(ref_dir, "pic", "000001.png")) as im:
        pic = np.array(im.convert("RGB")).transpose(2, 0, 1)
    H, W = pic.shape[1:]
    a = np.ascontiguousarray(pic[:, :384, :576])
    b = np.ascontiguousarray(pic[:, H - 384:, W - 576:]).copy()
    b[:, :103, :103] = np.array([90, 120, 60], dtype=np.uint8)[:, None, None]   # block (0, 0) and its 7-pixel margin: flat
    return [a, b, smooth_noise(3, 397, 603), smooth_noise(4, 192, 288)]


def load_reference(ref_dir):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, ref_dir)
    import loss.niqe_utils as N
    return N


def run_reference(N, rgb):
    """-> dict(y, half, mscn1, mscn2, feat, score) as the reference computes them for the HWC uint8 image"""
    cap = {"blocks": [], "feat": [], "half": None, "y": None}
    orig_feature, orig_resize, orig_niqe = N.compute_feature, N.imresize, N.niqe

    def feature(block):
        cap["blocks"].append(np.array(block))
        f = orig_feature(block)
        cap["feat"].append(f)
        return f

    def resize(img, *a, **k):
        out = orig_resize(img, *a, **k)
        cap["half"] = np.array(out)
        return out

    def niqe(img, *a, **k):
        cap["y"] = np.array(img)
        return orig_niqe(img, *a, **k)

    N.compute_feature, N.imresize, N.niqe = feature, resize, niqe
    try:
        with np.errstate(all="ignore"):
            s = N.calculate_niqe(np.ascontiguousarray(rgb.transpose(1, 2, 0)))
    finally:
        N.compute_feature, N.imresize, N.niqe = orig_feature, orig_resize, orig_niqe
    h, w = cap["y"].shape
    hc, wc = h // 96 * 96, w // 96 * 96
    nh, nw = hc // 96, wc // 96
    nb = nh * nw
    assert len(cap["blocks"]) == 2 * nb

    def assemble(blocks, bs):
        m = np.zeros((nh * bs, nw * bs), dtype=np.float32)
        i = 0
        for bw in range(nw):
            for bh in range(nh):
                assert blocks[i].dtype == np.float32 and blocks[i].shape == (bs, bs)
                m[bh * bs:(bh + 1) * bs, bw * bs:(bw + 1) * bs] = blocks[i]
                i += 1
        return m

    y = cap["y"][:hc, :wc]
    assert np.array_equal(y, np.round(y)) and y.min() >= 0 and y.max() <= 255
    feat = np.concatenate([np.array(cap["feat"][:nb], dtype=np.float64), np.array(cap["feat"][nb:], dtype=np.float64)], axis=1)
    half = (cap["half"] * 255.).astype(np.float32)
    assert cap["half"].dtype == np.float32
    return dict(y=y.astype(np.uint8), half=half, mscn1=assemble(cap["blocks"][:nb], 96), mscn2=assemble(cap["blocks"][nb:], 48),
                feat=feat, score=np.float64(s))


def reference_luma_hash(N):
    """SHA-256 of the reference's rounded Y (uint8) over all 2^24 triples as a 4096 x 4096 image, R-major"""
    rgb = R.luma_all_triples()
    h = hashlib.sha256()
    ys = []
    for r0 in range(0, 4096, 256):
        img = np.ascontiguousarray(rgb[:, r0:r0 + 256].transpose(1, 2, 0)).astype(np.float32)
        y = np.squeeze(N.to_y_channel(img)).round()
        ys.append(y.astype(np.uint8))
        h.update(ys[-1].tobytes())
    return h.hexdigest(), np.concatenate(ys)


def packed(arrays):
    """greedy split of {key: array} into parts whose compressed size stays under LIMIT"""
    def size(d):
        buf = io.BytesIO()
        np.savez_compressed(buf, **d)
        return buf.tell()
    parts, cur = [], {}
    for k, v in arrays.items():
        trial = dict(cur, **{k: v})
        if cur and size(trial) > LIMIT:
            parts.append(cur)
            cur = {k: v}
        else:
            cur = trial
        assert size(cur) <= LIMIT, (k, size(cur))
    parts.append(cur)
    return parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference repository")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    ref_dir = os.path.abspath(args.reference)
    N = load_reference(ref_dir)
    os.chdir(ref_dir)                                    # the reference opens ./loss/niqe_pris_params.npz
    prm = np.load(os.path.join(ref_dir, "loss", "niqe_pris_params.npz"))
    mu_p, cov_p, win = prm["mu_pris_param"], prm["cov_pris_param"], prm["gaussian_window"]
    assert np.array_equal(win, win[::-1, ::-1]), "the window is not symmetric: correlation != convolution"

    digest, y_all = reference_luma_hash(N)
    mine = R.luma(R.luma_all_triples())
    print(f"luma over 2^24 triples: {int((mine != y_all).sum())} differ from the reference; sha256 {digest}")
    assert np.array_equal(mine, y_all)

    rng = np.random.default_rng(11)
    meta = dict(luma_sha256=np.array(digest), n_inputs=np.array(0))
    ref_diff, perturb, half_ulps, files = [], 0.0, [], {}
    ins = inputs(ref_dir)
    for i, rgb in enumerate(ins):
        g = run_reference(N, rgb)
        st = R.stages(rgb, win)
        nb = g["feat"].shape[0]
        print(f"input {i}: {rgb.shape[1]}x{rgb.shape[2]}, {nb} blocks, reference score {float(g['score']):.9f}")
        print(f"  Y differs on {int((st['y'] != g['y']).sum())} px; MSCN1 on {int((st['mscn1'] != g['mscn1']).sum())} px; "
              f"MSCN(golden half) on {int((R.mscn(g['half'], win) != g['mscn2']).sum())} px")
        dh = np.abs(st["half"].astype(np.float64) - g["half"]).max()
        half_ulps.append(dh / 2.0 ** -16)                          # fp32 ulp at 256: 2^-16... values < 256 have ulp <= 2^-16
        print(f"  half-size image: max |diff| {dh:.3e} ({(st['half'] != g['half']).mean() * 100:.1f} % of pixels differ); "
              f"MSCN2 max |diff| {np.nanmax(np.abs(st['mscn2'] - g['mscn2'])):.3e}")
        cols = [0] + [2 + 4 * k for k in range(4)]
        cols = cols + [18 + c for c in cols]
        da = np.abs(st["feat"][:, cols] - g["feat"][:, cols])
        moved = int((da > 1e-9).sum())
        print(f"  fits moved: {moved} of {da.size}; max alpha step {da.max():.4f}")
        if da.max() > 0.001 + 1e-12 or moved > 0.01 * da.size:
            raise SystemExit("refusing this fixture set: the restatement's fits leave the reference's by more than allowed")
        assert np.array_equal(np.isnan(st["feat"]).any(axis=1), np.isnan(g["feat"]).any(axis=1))
        s = R.score(st["feat"], mu_p, cov_p)
        ref_diff.append(abs(s - float(g["score"])))
        print(f"  restatement score {s:.9f}, |diff| {ref_diff[-1]:.3e}; NaN rows {int(np.isnan(g['feat']).any(axis=1).sum())}")
        for _ in range(8):
            mom = []
            for m, bs in ((st["mom1"], 96), (st["mom2"], 48)):
                e = 1e-12 * rng.choice([-1.0, 1.0], size=m.shape)
                e[..., 0] = e[..., 2] = 0.0                         # the counts are exact
                mom.append(R.features_from_moments(m * (1 + e), bs)[0])
            perturb = max(perturb, abs(R.score(np.concatenate(mom, axis=1), mu_p, cov_p) - s))
        files[f"niqe_img{i}"] = dict(rgb=rgb, y=g["y"], half=g["half"], mscn2=g["mscn2"], feat=g["feat"], score=g["score"],
                                     mscn1=g["mscn1"])
    meta.update(n_inputs=np.array(len(ins)), score_perturb=np.array(perturb), score_ref_diff=np.array(ref_diff),
                half_max_ulps=np.array(half_ulps))
    print(f"score_perturb {perturb:.3e}; max score_ref_diff {max(ref_diff):.3e}; half-size ulps {half_ulps}")

    os.makedirs(args.out, exist_ok=True)
    shutil.copyfile(os.path.join(ref_dir, "loss", "niqe_pris_params.npz"), os.path.join(args.out, "niqe_pris_params.npz"))
    np.savez_compressed(os.path.join(args.out, "niqe.npz"), **meta)
    for name, arrays in files.items():
        for k, part in enumerate(packed(arrays)):
            path = os.path.join(args.out, f"{name}.part{k}.npz")
            np.savez_compressed(path, **part)
            print(f"  {os.path.basename(path)}: {os.path.getsize(path)} bytes ({', '.join(part)})")


if __name__ == "__main__":
    main()
