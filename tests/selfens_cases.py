"""The definitions of include/srgd_selfens.h restated in numpy, and the cases tests/test_selfens_cpu.py and tests/test_selfens_gpu.py
share: ``apply`` (a dihedral operation 0 .. 7 on an ``[h,w,3]`` uint8 image), ``inverse`` and ``merge`` (turn every source back, sum
in int64, divide with halves up)."""
import numpy as np

OPS = {1: (0,), 2: (0, 1), 4: (0, 1, 2, 3), 8: (0, 1, 2, 3, 4, 5, 6, 7)}
MAX_SOURCES = 8
MAX_IMAGES = 32                                           # images of one launch (SRGD_SELFENS_MAX_IMAGES)
TILE = 32
# (h, w): tiles end mid-row and mid-column, rows start at every byte phase modulo 16 (3 * w is odd in most), one side is shorter than
# a tile while the other spans several
SIZES = [(1, 1), (1, 7), (7, 1), (5, 6), (63, 65), (65, 63), (64, 64), (88, 96), (129, 67), (16, 341)]
# source lists of the general entry: the op sets of OPS, odd counts, a repeated op
OP_LISTS = {1: (0,), 2: (0, 1), 3: (5, 0, 6), 4: (0, 1, 2, 3), 5: (7, 4, 4, 1, 2), 8: (0, 1, 2, 3, 4, 5, 6, 7)}
REPEATED = (3, 3, 6, 6, 5, 0)


def apply(x, op):
    """The dihedral operation ``op`` on ``x`` ``[h,w,...]``: bit 2 transposes, then bit 0 reverses the columns, then bit 1 the rows."""
    if not 0 <= op <= 7:
        raise ValueError(op)
    x = x.swapaxes(0, 1) if op & 4 else x
    x = x[:, ::-1] if op & 1 else x
    x = x[::-1] if op & 2 else x
    return x.copy(order="C")                              # a copy of its own: no negative stride is left, also on axes of length 1


def inverse(op):
    """The op that undoes ``op``, found from the definition on a non-square image of distinct values."""
    probe = np.arange(2 * 3).reshape(2, 3)
    found = [k for k in range(8) if apply(apply(probe, op), k).shape == probe.shape and np.array_equal(apply(apply(probe, op), k), probe)]
    assert len(found) == 1
    return found[0]


def compose(first, then):
    """The one op equal to ``first`` followed by ``then``."""
    probe = np.arange(2 * 3).reshape(2, 3)
    want = apply(apply(probe, first), then)
    found = [k for k in range(8) if apply(probe, k).shape == want.shape and np.array_equal(apply(probe, k), want)]
    assert len(found) == 1
    return found[0]


def merge(sources, ops):
    """``sources[j]`` = ``apply(x_j, ops[j])`` of ``[H,W,3]`` images -> uint8 ``[H,W,3]``: (2 S + n) // (2 n) of the sources turned back."""
    n = len(sources)
    assert 1 <= n <= MAX_SOURCES and len(ops) == n
    total = sum(apply(s, inverse(op)).astype(np.int64) for s, op in zip(sources, ops))
    return ((2 * total + n) // (2 * n)).astype(np.uint8)


def mean01(m):
    """fp32 planar ``[3,H,W]`` of a merged uint8 ``[H,W,3]`` image: ``np.float32(m) / np.float32(255)``."""
    return (m.astype(np.float32) / np.float32(255)).transpose(2, 0, 1).copy()


def image(h, w, seed=0):
    return np.random.default_rng([seed, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8)


def sources(h, w, ops, kind="random", seed=0):
    """The source list of an ``[h,w,3]`` image for ``ops``: source j is ``apply(x_j, ops[j])``.
    kind "random": seeded bytes, another image per source; "ones": all 255 (the width of the sums); "halves": n = len(ops) even -
    the sum S of byte e is ``n * base + n / 2`` at even e (S mod n == n / 2: the half goes up) and ``n * base + n / 2 - 1`` at odd e
    (down), base = e % 251."""
    n = len(ops)
    if kind == "random":
        xs = [image(h, w, seed + 17 * j + 1) for j in range(n)]
    elif kind == "ones":
        xs = [np.full((h, w, 3), 255, np.uint8) for _ in range(n)]
    elif kind == "halves":
        assert n % 2 == 0
        e = np.arange(3 * h * w).reshape(h, w, 3)
        base = e % 251
        extra = np.where(e % 2 == 0, n // 2, n // 2 - 1)               # that many sources hold base + 1, the others base
        xs = [(base + (j < extra)).astype(np.uint8) for j in range(n)]
    else:
        raise ValueError(kind)
    return [apply(x, op) for x, op in zip(xs, ops)]


def halves_expected(h, w, n):
    """What ``merge(sources(h, w, ops, "halves"))`` is for any ops of even length n: base + 1 at even bytes, base at odd ones
    (n = 2: S mod 2 == 0 at odd bytes, the mean is exact)."""
    e = np.arange(3 * h * w).reshape(h, w, 3)
    return (e % 251 + (e % 2 == 0)).astype(np.uint8)


def orientation_stub(lr, seed=0):
    """A deterministic, orientation-dependent x4 'super-resolution' of an ``[h,w,3]`` uint8 array for the driver tests: every pixel is
    repeated 4 x 4 and a ramp that is neither symmetric nor transposition-invariant, and the seed, are added modulo 256."""
    up = np.repeat(np.repeat(lr.astype(np.int64), 4, axis=0), 4, axis=1)
    y, x = np.mgrid[0:up.shape[0], 0:up.shape[1]]
    return ((up + (3 * y + 7 * x + 11 * seed)[:, :, None] + np.arange(3)) % 256).astype(np.uint8)
