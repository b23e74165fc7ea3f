"""The oracle of the LOE tests (tests/test_loe_cpu.py, tests/test_loe_gpu.py), numpy only.

Definition: lightness L(p) = max(R, G, B) of a uint8 pixel; the sampler takes step = max(1, min(h, w) //
sample) (1 when sample is None), rows = h // step, cols = w // step, sample (i, j) = pixel (i * step, j * step), m = rows *
cols; with U(a, b) = 1 if a >= b else 0, L from the low image and Le from the enhanced one,
    num = sum_x sum_y U(L(x), L(y)) xor U(Le(x), Le(y))       over all m x m ordered pairs, y = x included
    LOE = num / m.
brute() is that text, pairwise and chunked; by_hist() is the 256 x 256 joint-histogram identity the kernel uses, for the
cases where m^2 pairs are too many -- test_loe_cpu.py holds the two equal where both run."""
import numpy as np


def grid(h, w, sample):
    step = 1 if sample is None else max(1, min(h, w) // sample)
    return step, h // step, w // step


def lightness(img, sample):
    """uint8 (3,h,w) -> int64 (m,): max over the channels at the sampled pixels, row-major"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[0] == 3, (img.dtype, img.shape)
    step, rows, cols = grid(img.shape[1], img.shape[2], sample)
    return img[:, :rows * step:step, :cols * step:step].max(axis=0).reshape(-1).astype(np.int64)


def brute(low, out, sample, chunk=1024):
    """-> (num, m): num a Python int, straight from the definition"""
    L, Le = lightness(low, sample), lightness(out, sample)
    assert L.shape == Le.shape
    m, num = L.size, 0
    for s in range(0, m, chunk):
        a = L[s:s + chunk, None] >= L[None, :]
        b = Le[s:s + chunk, None] >= Le[None, :]
        num += int(np.count_nonzero(a ^ b))
    return num, m


def by_hist(low, out, sample):
    """-> (num, m) through H[a][b] = #{x : L(x) = a, Le(x) = b}: num = sum H (A[a] + B[b] - 2 C[a][b]), A and B the inclusive
    prefixes of the marginals and C the 2-D inclusive prefix of H; Python integers, so nothing can overflow"""
    L, Le = lightness(low, sample), lightness(out, sample)
    H = np.zeros((256, 256), dtype=np.int64)
    np.add.at(H, (L, Le), 1)
    A = np.cumsum(H.sum(axis=1))
    B = np.cumsum(H.sum(axis=0))
    C = np.cumsum(np.cumsum(H, axis=0), axis=1)
    num = 0
    for a, b in zip(*np.nonzero(H)):
        num += int(H[a, b]) * (int(A[a]) + int(B[b]) - 2 * int(C[a, b]))
    return num, int(L.size)
