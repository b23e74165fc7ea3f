"""What tests/test_resize_cpu.py, test_resize_gpu.py and test_evaluate_resize_gpu.py share: the cases of the 8-bit bicubic
resize, their images, PIL's own answer (the oracle: exact, no tolerance) and a numpy restatement of Pillow's two fixed-point
passes driven by metrics.resize_plan's tables (the project's own; it is what csrc/resize.hip computes)."""
import numpy as np

# (H, W) -> (h, w): down and up on both axes, one axis unchanged (twice), an 11 x 11 side, an 83:1 reduction (172 taps),
# sizes one apart, a 1-pixel axis, a 3-pixel axis
CASES = [((24, 40), (17, 29)), ((17, 29), (24, 40)), ((24, 40), (24, 31)), ((24, 40), (13, 40)), ((11, 11), (64, 64)),
         ((64, 64), (11, 11)), ((5, 300), (40, 7)), ((33, 47), (34, 46)), ((1, 9), (12, 12)), ((250, 3), (11, 11))]
# an output width that no block size divides, more than one block per pass
WIDE = ((96, 128), (37, 211))
KINDS = ("random", "extremes", "normal")


def image(kind, h, w, seed=0):
    """uint8 (h,w,3): uniform random bytes; random 0 / 255 (both ends of the clamp: bicubic overshoots); a clipped normal"""
    rng = np.random.default_rng([seed, h, w, KINDS.index(kind)])
    if kind == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "extremes":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    return np.clip(rng.normal(128, 90, (h, w, 3)), 0, 255).astype(np.uint8)


def pil_resize(img, size):
    """uint8 (H,W,3) -> uint8 (h,w,3), (h, w) = size: Image.resize with its defaults"""
    from PIL import Image
    return np.array(Image.fromarray(img).resize((size[1], size[0])))


def _pass(a, bounds, coeffs):
    """one pass along axis 0 of a (n_in, ...) uint8 array"""
    out = np.empty((bounds.shape[0],) + a.shape[1:], dtype=np.uint8)
    src = a.astype(np.int64)
    for o, (first, count) in enumerate(bounds):
        k = coeffs[o, :count].astype(np.int64).reshape((-1,) + (1,) * (a.ndim - 1))
        acc = (1 << 21) + (src[first:first + count] * k).sum(axis=0)
        acc = ((acc + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int64)          # the int32 accumulator
        out[o] = np.clip(acc >> 22, 0, 255)
    return out


def restated(img, size, plan):
    """uint8 (H,W,3) -> uint8 (h,w,3): horizontal pass first, rounded to uint8, then vertical; an unchanged axis is skipped.
    plan: metrics.resize_plan"""
    H, W = img.shape[:2]
    h, w = size
    out = img
    if W != w:
        out = _pass(out.transpose(1, 0, 2), *plan(W, w)).transpose(1, 0, 2)
    if H != h:
        out = _pass(out, *plan(H, h))
    return np.ascontiguousarray(out)
