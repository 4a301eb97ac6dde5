"""The yardstick of the ensemble tests: the mean image, the spread map and the two statistics of the K samples of an image, restated
in numpy with int64 / Python integers LITERALLY from the definition in include/srgd_ensemble.h.  Test infrastructure only: product
code never imports it.

Definition.  K samples, each uint8 [h][w][3], 2 <= K <= 256.  For every one of the 3 h w elements, x_k its K values:
S = sum x_k, Q = sum x_k^2, D = K Q - S^2 (>= 0).
  mean image:  m = (2 S + K) div (2 K)   (integer division: nearest, halves up)
  spread map:  twice the population standard deviation sqrt(D) / K, rounded to nearest with halves up, BY INTEGERS: s = 0 if
               16 D < K^2, else the one s in 1..255 with (2s-1)^2 K^2 <= 16 D < (2s+1)^2 K^2
  mean01:      (float32)m / float32(255), planar [3][h][w]
  mean_std = (sum_e sqrt((double)D_e) / K) / (3 h w) with the sum taken by math.fsum;  max_std = sqrt((double)max_e D_e) / K.

Tolerances of the GPU tests: every comparison is exact but mean_std, whose sum the kernels take in float64 in a fixed order
(math.fsum here is the exactly rounded sum).  The test shapes have N <= 12,288 elements; a term is sqrt(D) <= 127.5 K, so every
partial sum is at most N * 127.5 K and each of the N additions errs by at most 2^-53 of it: N^2 * 2^-53 * 127.5 K in all, which
the divisions by K and by N bring to N * 2^-53 * 127.5 ~ 1.8e-10 in 8-bit units at the very worst, and below 1e-11 for the mostly
pairwise order the kernels use.  The two divisions add 2 ulp of a value <= 127.5 (3e-14).  |mean_std - yardstick| <= 1e-9 absolute."""
import math

import numpy as np

MEAN_STD_TOL = 1e-9
CHUNK = 4096                            # elements per workgroup pass of the kernels (ensemble.hip: EN_CHUNK): shapes straddle it
VEC = 16                                # bytes of a lane per sample


def sums(samples):
    """uint8 [K,h,w,3] -> (K, S, Q, D) as int64 arrays [h,w,3]."""
    x = np.asarray(samples)
    assert x.dtype == np.uint8 and x.ndim == 4 and x.shape[3] == 3 and 2 <= x.shape[0] <= 256
    k = int(x.shape[0])
    x = x.astype(np.int64)
    s, q = x.sum(axis=0), (x * x).sum(axis=0)
    d = k * q - s * s
    assert d.min() >= 0
    return k, s, q, d


def spread_from_d(d, k):
    """The spread map from D by the integer inequalities alone: s = #{t in 1..255 : (2t-1)^2 K^2 <= 16 D}."""
    d16 = 16 * np.asarray(d, dtype=np.int64)
    t = np.arange(1, 256, dtype=np.int64)
    bounds = (2 * t - 1) ** 2 * (k * k)                  # increasing in t: the count is the one s of the definition
    s = (bounds[None, :] <= d16.reshape(-1, 1)).sum(axis=1).reshape(d16.shape)
    ok_lo = np.where(s == 0, d16 < k * k, (2 * s - 1) ** 2 * k * k <= d16)
    assert ok_lo.all() and ((2 * s + 1) ** 2 * k * k > d16).all()
    return s.astype(np.uint8)


def restate(samples):
    """uint8 [K,h,w,3] -> (mean uint8 [h,w,3], spread uint8 [h,w,3], {"mean_std", "max_std"})."""
    k, s, _, d = sums(samples)
    mean = ((2 * s + k) // (2 * k)).astype(np.uint8)
    total = math.fsum(math.sqrt(float(int(v))) for v in d.reshape(-1))
    stats = {"mean_std": (total / k) / d.size, "max_std": math.sqrt(float(int(d.max()))) / k}
    return mean, spread_from_d(d, k), stats


def mean01(mean_u8):
    """uint8 [h,w,3] -> float32 [3,h,w]: (float)m / 255.0f."""
    return (np.asarray(mean_u8).astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1).copy()


def random_samples(k, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (k, h, w, 3), dtype=np.uint8)


def all_means_samples(k, seed=0):
    """[K,16,16,3] samples whose mean image takes all 256 values: channel 0 is the level v = 16 y + x in every sample (spread 0),
    channel 1 alternates v + 1 / v - 1 in pairs around it (flat at 0 and 255, where a neighbour is missing), channel 2 is random."""
    base = np.arange(256, dtype=np.int64).reshape(16, 16)
    inner = (base > 0) & (base < 255)
    out = random_samples(k, 16, 16, seed)
    for j in range(k):
        out[j, :, :, 0] = base
        delta = 0 if j >= 2 * (k // 2) else (1 if j % 2 == 0 else -1)
        out[j, :, :, 1] = base + delta * inner
    return out


def extreme_samples(k, h, w, seed):
    """Every element of every sample is 0 or 255."""
    return (np.random.default_rng(seed).integers(0, 2, (k, h, w, 3)) * 255).astype(np.uint8)
