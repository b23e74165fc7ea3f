"""numpy / scipy restatement of the BRISQUE pipeline of include/cidnet_hip.h (csrc/brisque.hip), stage by stage, each stage
through the scipy routine the contract names: scipy.signal.convolve2d (MSCN), scipy.ndimage.gaussian_filter and zoom (half
size), scipy.optimize.brentq (the shape), scipy.special.gammaln; the support-vector regression in plain numpy.  It restates
the description of imquality.brisque, which is not installed: parity with that package itself is not pinned."""
import numpy as np
from scipy import ndimage, optimize, signal, special

TILE = 32
LO, HI = 0.05, 100.0


def gray(rgb_u8):
    """uint8 (3,h,w) -> fp64 (h,w): skimage's rgb2gray of a uint8 image"""
    r, g, b = (rgb_u8[i].astype(np.float64) for i in range(3))
    return ((0.2125 * r + 0.7154 * g) + 0.0721 * b) / 255.0


def window():
    i = np.arange(7) - 3
    k = np.exp(-(i[:, None] ** 2 + i[None, :] ** 2) / (2.0 * (7.0 / 6.0) ** 2))
    return k / k.sum()


def local_mean(y):
    return signal.convolve2d(y, window(), "same")


def mscn(y):
    mu = local_mean(y)
    s = signal.convolve2d(y * y, window(), "same")
    dev = np.sqrt(np.abs(mu * mu - s))
    return (y - mu) / (dev + 1.0 / 255.0)


def maps(m):
    """the five maps, slices and not rolls: M, H, V, D1, D2"""
    return [m, m[:, :-1] * m[:, 1:], m[:-1, :] * m[1:, :], m[:-1, :-1] * m[1:, 1:], m[1:, :-1] * m[:-1, 1:]]


def sums(x):
    """the six raw sums of a map: n_left, sum of squares left, n_right (zeros included), the same, sum |x|, sum x^2"""
    x = np.asarray(x, dtype=np.float64).ravel()
    left, right = x[x < 0], x[x >= 0]
    return np.array([left.size, (left ** 2).sum(), right.size, (right ** 2).sum(), np.abs(x).sum(), (x ** 2).sum()])


def moments(m):
    """(5,6): the sums of the five maps over the whole plane"""
    return np.stack([sums(x) for x in maps(m)])


def tile_moments(m, tile=TILE):
    """(tiles,5,6), tiles in row-major order: a pair belongs to the tile of its M[r][c], the other element being the right,
    lower, lower-right or lower-left neighbour -- so D2[i][j] = M[i+1][j] M[i][j+1] belongs to the tile of (i, j+1)"""
    h, w = m.shape
    nty, ntx = -(-h // tile), -(-w // tile)
    out = np.zeros((nty * ntx, 5, 6))
    for a, (x, dc) in enumerate(zip(maps(m), (0, 0, 0, 0, 1))):
        rr, cc = np.meshgrid(np.arange(x.shape[0]), np.arange(x.shape[1]) + dc, indexing="ij")
        tid = (rr // tile) * ntx + cc // tile
        for t in range(nty * ntx):
            out[t, a] = sums(x[tid == t])
    return out


def phi(a):
    return np.exp(2.0 * special.gammaln(2.0 / a) - special.gammaln(1.0 / a) - special.gammaln(3.0 / a))


def root(big_r):
    """alpha with phi(alpha) = R on [0.05, 100]; NaN where R is NaN or outside (phi(0.05), phi(100))"""
    if not (big_r > phi(LO) and big_r < phi(HI)):
        return np.nan
    return optimize.brentq(lambda a: phi(a) - big_r, LO, HI, xtol=1e-15, rtol=4 * np.finfo(float).eps, maxiter=500)


def fit(s, first):
    """six sums -> [alpha, (sl^2 + sr^2) / 2] for M (first), else [alpha, mean, sl^2, sr^2]; all NaN without a root"""
    with np.errstate(all="ignore"):
        nl, ql, nr, qr, a1, q = s
        sl, sr = np.sqrt(ql / nl), np.sqrt(qr / nr)
        g = sl / sr
        n = nl + nr
        r = (a1 / n) ** 2 / (q / n)
        big_r = r * (g ** 3 + 1) * (g + 1) / (g ** 2 + 1) ** 2
        alpha = root(big_r)
    if np.isnan(alpha):
        return [np.nan] * (2 if first else 4)
    if first:
        return [alpha, (sl ** 2 + sr ** 2) / 2]
    c = np.sqrt(special.gamma(1 / alpha) / special.gamma(3 / alpha))
    return [alpha, (sr - sl) * c * special.gamma(2 / alpha) / special.gamma(1 / alpha), sl ** 2, sr ** 2]


def features_of_moments(mom):
    """(5,6) -> 18"""
    out = []
    for a in range(5):
        out += fit(mom[a], a == 0)
    return np.array(out)


def half_shape(h, w):
    return int(np.round(h / 2)), int(np.round(w / 2))


def smooth(y):
    return ndimage.gaussian_filter(y, 0.5, mode="mirror")


def half(y):
    """skimage.transform.rescale(y, 1/2) with its defaults, through the scipy routines it calls"""
    h, w = y.shape
    oh, ow = half_shape(h, w)
    return ndimage.zoom(smooth(y), (oh / h, ow / w), order=1, mode="mirror", grid_mode=True)


def features(rgb_u8):
    """uint8 (3,h,w) -> 36"""
    y = gray(rgb_u8)
    return np.concatenate([features_of_moments(moments(mscn(y))), features_of_moments(moments(mscn(half(y))))])


def min_margin(rgb_u8):
    """min |Y - mu| over both scales: below about 1e-9 a pixel's side of zero follows the summation order"""
    y = gray(rgb_u8)
    y2 = half(y)
    return min(np.abs(y - local_mean(y)).min(), np.abs(y2 - local_mean(y2)).min())


def svr(f, sv, coef, rho, gamma, fmin, fmax):
    """36 features -> the epsilon-SVR decision value, the support vectors in order"""
    z = -1.0 + 2.0 * (np.asarray(f, dtype=np.float64) - fmin) / (fmax - fmin)
    acc = 0.0
    for v, c in zip(sv, coef):
        acc += c * np.exp(-gamma * ((v - z) ** 2).sum())
    return acc - rho


def score(rgb_u8, prm):
    return svr(features(rgb_u8), prm.sv, prm.coef, prm.rho, prm.gamma, prm.fmin, prm.fmax)
