"""numpy / scipy restatement of the NIQE the library computes: Mittal, Soundararajan, Bovik 2013 with the choices
pyiqa 0.1.x makes as far as they can be stated without the package. Parity with pyiqa itself has never been run.

`dtype` is the arithmetic of the pixel path (half-size image, MSCN maps, block sums): float64 is the reference, float32 mirrors
the device. Both evaluate the local variance with the window centred on its own pixel c (m = sum w (y - c), var = sum w (y - c)^2
- m^2, n = -m / (sigma + 1); see mscn): the same numbers as G*y^2 - mu^2 in exact arithmetic, without the cancellation that
costs float32 1e-3 in the features of flat regions (`shifted=False` evaluates that form, to show it). The
closed-form fit of a block's sums is float64 in both, as on the device. `alpha` forces the AGGD shape of every (block, map) fit.
"""
import numpy as np
from scipy.special import gamma as _gamma

BLOCK = 96
GAM = 0.2 + 0.001 * np.arange(9801)
_G1, _G2, _G3 = _gamma(1 / GAM), _gamma(2 / GAM), _gamma(3 / GAM)
R_GAM = _G2 * _G2 / (_G1 * _G3)
ROLLS = ((0, 1), (1, 0), (1, 1), (1, -1))


def gauss7():
    g = np.exp(-((np.arange(7) - 3.0) ** 2) / (2 * (7.0 / 6.0) ** 2))
    k = np.outer(g, g)
    return k / k.sum()


def luma(img):
    """float32 exactly as the device: img is uint8 (H, W) / (H, W, 3) RGB or float32 (H, W) / (3, H, W) / (1, H, W) in [0,1]."""
    f = np.float32
    a = np.asarray(img)
    if a.dtype == np.uint8:
        a = a.astype(f) / f(255)
        if a.ndim == 3:
            a = np.moveaxis(a, 2, 0)
    a = a.astype(f)
    if a.ndim == 3 and a.shape[0] == 3:
        y = (f(0.299) * a[0] + f(0.587) * a[1]) + f(0.114) * a[2]
    else:
        y = a.reshape(a.shape[-2:])
    return np.rint(y * f(255))


def crop(y):
    return y[:y.shape[0] // BLOCK * BLOCK, :y.shape[1] // BLOCK * BLOCK]


def keys_cubic(x):
    x = np.abs(x)
    return np.where(x <= 1, 1.5 * x ** 3 - 2.5 * x ** 2 + 1, np.where(x <= 2, -0.5 * x ** 3 + 2.5 * x ** 2 - 4 * x + 2, 0.0))


def resize_taps(n):
    """MATLAB imresize(., 0.5) bicubic with antialiasing along an axis of length n: (idx [ceil(n/2), 10], w [ceil(n/2), 10])."""
    i = np.arange((n + 1) // 2)
    u = 2 * i + 0.5
    j = (np.floor(u - 4).astype(np.int64) + 1)[:, None] + np.arange(10)[None]
    w = 0.5 * keys_cubic(0.5 * (u[:, None] - j))
    w = w / w.sum(1, keepdims=True)
    j = np.where(j < 0, -j - 1, np.where(j >= n, 2 * n - 1 - j, j))
    return j, w


def resize_matrix(n):
    j, w = resize_taps(n)
    m = np.zeros((j.shape[0], n))
    for t in range(10):
        np.add.at(m, (np.arange(j.shape[0]), j[:, t]), w[:, t])
    return m


def half_size(y, dtype=np.float64):
    """imresize(y / 255, 0.5) * 255: the vertical pass first, taps summed in order."""
    x = y.astype(dtype) / dtype(255)
    for axis in (0, 1):
        j, w = resize_taps(x.shape[axis])
        w = w.astype(dtype)
        x = np.moveaxis(x, axis, 0)
        acc = np.zeros((j.shape[0],) + x.shape[1:], dtype)
        for t in range(10):
            acc = acc + w[:, t].reshape((-1,) + (1,) * (x.ndim - 1)) * x[j[:, t]]
        x = np.moveaxis(acc, 0, axis)
    return x * dtype(255)


def gauss_classes():
    """The 7x7 Gaussian has ten distinct weights: class of tap (dy, dx) = hi * (hi + 1) / 2 + lo over (lo, hi) = sorted(|dy-3|, |dx-3|)."""
    k = gauss7()
    cls = np.zeros((7, 7), np.int64)
    w = np.zeros(10)
    for dy in range(7):
        for dx in range(7):
            lo, hi = sorted((abs(dy - 3), abs(dx - 3)))
            cls[dy, dx] = hi * (hi + 1) // 2 + lo
            w[cls[dy, dx]] = k[dy, dx]
    return cls, w


def mscn(y, dtype=np.float64, shifted=True):
    """(n, sigma) of an image, replicate border. shifted: differences d = y - c to the window's own centre pixel are summed per weight
    class first (exact for an integer image in either precision, so a mean that is zero by symmetry is exactly zero and the sign
    of n, which the fit counts, is not left to rounding), then m = sum_c w_c S_c, var = sum_c w_c Q_c - m^2, n = -m / (sigma + 1)."""
    y = y.astype(dtype)
    p = np.pad(y, 3, mode="edge")
    H, W = y.shape
    if shifted:
        cls, w = gauss_classes()
        w = w.astype(dtype)
        S = [np.zeros_like(y) for _ in range(10)]
        Q = [np.zeros_like(y) for _ in range(10)]
        for dy in range(7):
            for dx in range(7):
                d = p[dy:dy + H, dx:dx + W] - y
                S[cls[dy, dx]] = S[cls[dy, dx]] + d
                Q[cls[dy, dx]] = Q[cls[dy, dx]] + d * d
        a = np.zeros_like(y)
        b = np.zeros_like(y)
        for c in range(10):
            a = a + w[c] * S[c]
            b = b + w[c] * Q[c]
        sigma = np.sqrt(np.abs(b - a * a))
        return -a / (sigma + dtype(1)), sigma
    k = gauss7().astype(dtype)                            # the text's form, G*y^2 - (G*y)^2: what float32 cannot afford
    a = np.zeros_like(y)
    b = np.zeros_like(y)
    for dy in range(7):
        for dx in range(7):
            s = p[dy:dy + H, dx:dx + W]
            a = a + k[dy, dx] * s
            b = b + k[dy, dx] * (s * s)
    sigma = np.sqrt(np.abs(b - a * a))
    return (y - a) / (sigma + dtype(1)), sigma


def aggd(x, dtype=np.float64, alpha=None):
    """(alpha, left, right, Gamma(1/a), Gamma(2/a), Gamma(3/a)) of the samples x; sums in dtype, the fit in float64."""
    x = x.astype(dtype).ravel()
    q = x * x
    neg, pos = x < 0, x > 0
    sneg, spos, sabs = np.float64(q[neg].sum(dtype=dtype)), np.float64(q[pos].sum(dtype=dtype)), np.float64(np.abs(x).sum(dtype=dtype))
    N = float(x.size)
    with np.errstate(all="ignore"):
        left, right = np.sqrt(sneg / np.float64(neg.sum())), np.sqrt(spos / np.float64(pos.sum()))
        g = left / right
        ma, ms = sabs / N, (sneg + spos) / N
        r = ma * ma / ms
        g2 = g * g
        rn = r * (g2 * g + 1) * (g + 1) / ((g2 + 1) * (g2 + 1))
        idx = int(np.argmin((R_GAM - rn) ** 2)) if np.isfinite(rn) else 0
    if alpha is not None:
        idx = int(round((alpha - 0.2) / 0.001))
    return GAM[idx], left, right, _G1[idx], _G2[idx], _G3[idx]


def block_features(b, dtype=np.float64, alpha=None):
    """18 features of one block of an MSCN map; alpha: None or the 5 forced shapes."""
    out = []
    with np.errstate(all="ignore"):
        a, l, r, g1, g2, g3 = aggd(b, dtype, None if alpha is None else alpha[0])
        sc = np.sqrt(g1 / g3)
        out += [a, (l * sc + r * sc) / 2]
        for k, s in enumerate(ROLLS):
            a, l, r, g1, g2, g3 = aggd(b * np.roll(b, s, axis=(0, 1)), dtype, None if alpha is None else alpha[1 + k])
            sc = np.sqrt(g1 / g3)
            bl, br = l * sc, r * sc
            out += [a, (br - bl) * (g2 / g1), bl, br]
    return out


def features_from_luma(y, dtype=np.float64, alpha=None, shifted=True):
    """y: the rounded luma (any size >= two blocks). Returns (features [blocks, 36] float64, sharpness [blocks]).
    alpha: None or [blocks, 10] forced shapes in feature order (scale 1: block, 4 products; then scale 2)."""
    y = crop(np.asarray(y))
    by, bx = y.shape[0] // BLOCK, y.shape[1] // BLOCK
    if by * bx < 2:
        raise ValueError("fewer than two 96x96 blocks")
    n1, s1 = mscn(y, dtype, shifted)
    n2, _ = mscn(half_size(y, dtype), dtype, shifted)
    feat = np.zeros((by * bx, 36))
    sharp = np.zeros(by * bx)
    for i in range(by):
        for j in range(bx):
            b = i * bx + j
            for sc, (n, B) in enumerate(((n1, BLOCK), (n2, BLOCK // 2))):
                blk = n[i * B:(i + 1) * B, j * B:(j + 1) * B]
                feat[b, 18 * sc:18 * sc + 18] = block_features(blk, dtype, None if alpha is None else alpha[b, 5 * sc:5 * sc + 5])
            sharp[b] = np.float64(s1[i * BLOCK:(i + 1) * BLOCK, j * BLOCK:(j + 1) * BLOCK].sum(dtype=dtype)) / (BLOCK * BLOCK)
    return feat, sharp


def features(img, dtype=np.float64, alpha=None):
    return features_from_luma(luma(img), dtype, alpha)


def alphas_of(feat):
    """[blocks, 10]: the shape entries of a feature matrix, in the order `alpha` takes them."""
    cols = [0, 2, 6, 10, 14]
    return np.asarray(feat)[:, cols + [18 + c for c in cols]]


def score(feat, mu, cov):
    feat = np.asarray(feat, np.float64)
    m = np.nanmean(feat, axis=0)
    ok = ~np.isnan(feat).any(axis=1)
    C = np.cov(feat[ok], rowvar=False)
    d = np.asarray(mu, np.float64).ravel() - m
    P = np.linalg.pinv((np.asarray(cov, np.float64) + C) / 2, rcond=36 * 2.2e-16)
    return float(np.sqrt(d @ P @ d))


def fit(feats_and_sharps, sharpness_threshold=0.75):
    """The paper's training step over [(features, sharpness), ...] of the pristine images -> (mu [36], cov [36, 36])."""
    keep = []
    for f, s in feats_and_sharps:
        f = np.asarray(f, np.float64)[np.asarray(s) > sharpness_threshold * np.max(s)]
        keep.append(f[~np.isnan(f).any(axis=1)])
    X = np.concatenate(keep)
    return X.mean(axis=0), np.cov(X, rowvar=False)
