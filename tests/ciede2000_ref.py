"""Independent numpy fp64 restatement of the CIEDE2000 metric (include/cidnet_hip.h: CIEDE2000), vectorised: sRGB -> Lab with
scikit-image's constants, dE00 by Sharma, Wu and Dalal (2005) with kL = kC = kH = 1, the mean over an image, the GT-mean
variant, and the 34 published test pairs of that paper.  scikit-image is not a dependency: the formulae below are the
definition's, and the published pairs pin the dE00 core."""
import numpy as np

import metrics_ref as MR

M = ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227))
WHITE = (0.95047, 1.0, 1.08883)

# L1 a1 b1 L2 a2 b2 dE00: Sharma, Wu, Dalal, "The CIEDE2000 color-difference formula: implementation notes, supplementary test
# data, and mathematical observations", Color Research and Application 30 (2005), table 1
SHARMA = np.array([
    [50, 2.6772, -79.7751, 50, 0, -82.7485, 2.0425], [50, 3.1571, -77.2803, 50, 0, -82.7485, 2.8615],
    [50, 2.8361, -74.0200, 50, 0, -82.7485, 3.4412], [50, -1.3802, -84.2814, 50, 0, -82.7485, 1.0000],
    [50, -1.1848, -84.8006, 50, 0, -82.7485, 1.0000], [50, -0.9009, -85.5211, 50, 0, -82.7485, 1.0000],
    [50, 0, 0, 50, -1, 2, 2.3669], [50, -1, 2, 50, 0, 0, 2.3669],
    [50, 2.49, -0.001, 50, -2.49, 0.0009, 7.1792], [50, 2.49, -0.001, 50, -2.49, 0.0010, 7.1792],
    [50, 2.49, -0.001, 50, -2.49, 0.0011, 7.2195], [50, 2.49, -0.001, 50, -2.49, 0.0012, 7.2195],
    [50, -0.001, 2.49, 50, 0.0009, -2.49, 4.8045], [50, -0.001, 2.49, 50, 0.0010, -2.49, 4.8045],
    [50, -0.001, 2.49, 50, 0.0011, -2.49, 4.7461], [50, 2.5, 0, 50, 0, -2.5, 4.3065],
    [50, 2.5, 0, 73, 25, -18, 27.1492], [50, 2.5, 0, 61, -5, 29, 22.8977],
    [50, 2.5, 0, 56, -27, -3, 31.9030], [50, 2.5, 0, 58, 24, 15, 19.4535],
    [50, 2.5, 0, 50, 3.1736, 0.5854, 1.0000], [50, 2.5, 0, 50, 3.2972, 0, 1.0000],
    [50, 2.5, 0, 50, 1.8634, 0.5757, 1.0000], [50, 2.5, 0, 50, 3.2592, 0.3350, 1.0000],
    [60.2574, -34.0099, 36.2677, 60.4626, -34.1751, 39.4387, 1.2644],
    [63.0109, -31.0961, -5.8663, 62.8187, -29.7946, -4.0864, 1.2630],
    [61.2901, 3.7196, -5.3901, 61.4292, 2.2480, -4.9620, 1.8731],
    [35.0831, -44.1164, 3.7933, 35.0232, -40.0716, 1.5901, 1.8645],
    [22.7233, 20.0904, -46.6940, 23.0331, 14.9730, -42.5619, 2.0373],
    [36.4612, 47.8580, 18.3852, 36.2715, 50.5065, 21.2231, 1.4146],
    [90.8027, -2.0831, 1.4410, 91.1528, -1.6435, 0.0447, 1.4441],
    [90.9257, -0.5406, -0.9208, 88.6381, -0.8985, -0.7239, 1.5381],
    [6.7747, -0.2908, -2.4247, 5.8714, -0.0985, -2.2286, 0.6377],
    [2.0776, 0.0795, -1.1350, 0.9033, -0.0636, -0.5514, 0.9082]], dtype=np.float64)
assert SHARMA.shape == (34, 7)
# pairs (1-based) whose hue difference is exactly 180 degrees in real arithmetic, and the neighbour whose value the other
# branch gives
SHARMA_ON_THE_EDGE = {10: 11, 14: 15}


def linearize(v):
    """v = level / 255 (any real numbers in [0, 1]) -> linear sRGB"""
    v = np.asarray(v, dtype=np.float64)
    return np.where(v > 0.04045, np.power((v + 0.055) / 1.055, 2.4), v / 12.92)


def _f(t):
    return np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0)


def rgb2lab(img):
    """(3, ...) levels 0..255 (uint8, or real numbers as the GT-mean image holds them) -> Lab (3, ...) fp64"""
    lin = linearize(np.asarray(img, dtype=np.float64) / 255.0)
    r, g, b = lin[0], lin[1], lin[2]
    xyz = [(M[i][0] * r + M[i][1] * g) + M[i][2] * b for i in range(3)]
    fx, fy, fz = (_f(xyz[i] / WHITE[i]) for i in range(3))
    return np.stack([116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)])


def _primed(lab1, lab2):
    """-> C1', C2', h1', h2' (degrees in [0, 360))"""
    a1, b1, a2, b2 = lab1[1], lab1[2], lab2[1], lab2[2]
    cbar = (np.hypot(a1, b1) + np.hypot(a2, b2)) / 2.0
    c7 = cbar ** 7
    G = 0.5 * (1.0 - np.sqrt(c7 / (c7 + 25.0 ** 7)))
    ap1, ap2 = (1.0 + G) * a1, (1.0 + G) * a2
    h1, h2 = np.degrees(np.arctan2(b1, ap1)), np.degrees(np.arctan2(b2, ap2))
    return np.hypot(ap1, b1), np.hypot(ap2, b2), np.where(h1 < 0, h1 + 360.0, h1), np.where(h2 < 0, h2 + 360.0, h2)


def delta_e(lab1, lab2):
    """Lab (3, ...) pairs, lab1 as colour 1 -> dE00 (...) fp64"""
    lab1, lab2 = np.asarray(lab1, dtype=np.float64), np.asarray(lab2, dtype=np.float64)
    C1, C2, h1, h2 = _primed(lab1, lab2)
    grey = C1 * C2 == 0
    dL, dC = lab2[0] - lab1[0], C2 - C1
    dh = h2 - h1
    dh = np.where(dh > 180.0, dh - 360.0, np.where(dh < -180.0, dh + 360.0, dh))
    dh = np.where(grey, 0.0, dh)
    dH = 2.0 * np.sqrt(C1 * C2) * np.sin(np.radians(dh / 2.0))
    Lb, Cb = (lab1[0] + lab2[0]) / 2.0, (C1 + C2) / 2.0
    hs = h1 + h2
    hb = np.where(grey, hs, np.where(np.abs(h1 - h2) <= 180.0, hs / 2.0, np.where(hs < 360.0, (hs + 360.0) / 2.0, (hs - 360.0) / 2.0)))
    T = (1.0 - 0.17 * np.cos(np.radians(hb - 30.0)) + 0.24 * np.cos(np.radians(2.0 * hb)) + 0.32 * np.cos(np.radians(3.0 * hb + 6.0))
         - 0.20 * np.cos(np.radians(4.0 * hb - 63.0)))
    dtheta = 30.0 * np.exp(-(((hb - 275.0) / 25.0) ** 2))
    c7 = Cb ** 7
    RC = 2.0 * np.sqrt(c7 / (c7 + 25.0 ** 7))
    l50 = (Lb - 50.0) ** 2
    SL = 1.0 + 0.015 * l50 / np.sqrt(20.0 + l50)
    SC = 1.0 + 0.045 * Cb
    SH = 1.0 + 0.015 * Cb * T
    RT = -np.sin(np.radians(2.0 * dtheta)) * RC
    x, y, z = dL / SL, dC / SC, dH / SH
    return np.sqrt(x * x + y * y + z * z + RT * y * z)


def image_map(restored, gt, gt_mean=False):
    """uint8 (3,h,w) pair -> the per-pixel dE00 (h,w); gt_mean: restored enters as metrics_ref.gt_mean_image's real numbers"""
    a = MR.gt_mean_image(restored, gt) if gt_mean else restored
    return delta_e(rgb2lab(a), rgb2lab(gt))


def mean_delta_e(restored, gt, gt_mean=False):
    return float(image_map(restored, gt, gt_mean).mean())


def hue_edge_distance(restored, gt, gt_mean=False):
    """min | |h1' - h2'| - 180 | in degrees over the pixels with C1' C2' != 0 (inf where there is none): how far the pair stays
    from the discontinuity of dh' and the mean hue, across which one rounding changes the value"""
    a = MR.gt_mean_image(restored, gt) if gt_mean else restored
    C1, C2, h1, h2 = _primed(rgb2lab(a), rgb2lab(gt))
    d = np.abs(np.abs(h1 - h2) - 180.0)[C1 * C2 != 0]
    return float(d.min()) if d.size else float("inf")
