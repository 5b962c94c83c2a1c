"""The case table of the image-metric tests (test_image_reference_cpu.py, test_gpu_image_metrics.py): sizes x alpha patterns of seeded,
non-negative RGBA32F image pairs.  The compare kernels sweep an image in trips of SWEEP = 256 blocks x 256 threads pixels.

Sizes: one pixel; one block short of / exactly / just over one 256-thread block; one pixel short of / exactly / one pixel over a whole
sweep; three sweeps and a tail of 121 pixels; the ragged-gather test's frame.
Alpha patterns: see ALPHAS.  Pixel values are non-negative, so no sum cancels."""
import functools

import numpy as np

SWEEP = 256 * 256

SIZES = [(1, 1), (255, 1), (256, 1), (257, 1), (65535, 1), (65536, 1), (65537, 1), (481, 409), (200, 96)]
ALPHAS = ["all", "seeded70", "last-only", "none", "cycle", "fireflies"]
CYCLE = np.array([0.0, -0.0, 1e-45, np.nan, -2.0, 1.0], np.float32)      # invalid, invalid, valid (denormal), valid, valid, valid

CASES = [(w, h, a) for (w, h) in SIZES for a in ALPHAS]
CASE_IDS = ["%dx%d-%s" % c for c in CASES]


@functools.lru_cache(maxsize=None)
def images(w, h, alpha):
    """(ref, own): two read-only [h][w][4] float32 images of the case"""
    rng = np.random.default_rng([w, h, ALPHAS.index(alpha)])
    ref = rng.random((h, w, 4), dtype=np.float32)
    own = rng.random((h, w, 4), dtype=np.float32)
    n = w * h
    a = ref.reshape(n, 4)[:, 3]
    if alpha in ("all", "fireflies"):
        a[:] = 1.0
    elif alpha == "seeded70":
        a[:] = (rng.random(n) < 0.7).astype(np.float32)
    elif alpha == "last-only":
        a[:] = 0.0
        a[-1] = 1.0
    elif alpha == "none":
        a[:] = 0.0
    elif alpha == "cycle":
        a[:] = np.resize(CYCLE, n)
    if alpha == "fireflies":      # own_mean and ref_mean apart by orders of magnitude
        own.reshape(n, 4)[::97, :3] *= np.float32(1.0e4)
        ref[..., :3] *= np.float32(0.1)
    ref.setflags(write=False)
    own.setflags(write=False)
    return ref, own


def expected_valid(w, h, alpha):
    """the valid count of a case, worked out from the pattern alone (None: seeded)"""
    n = w * h
    if alpha in ("all", "fireflies"):
        return n
    if alpha == "last-only":
        return 1
    if alpha == "none":
        return 0
    if alpha == "cycle":
        return 4 * (n // 6) + max(0, n % 6 - 2)
    return None


# ---- the multi-rank case: a frame of unequal shards with different means
SHARD_W, SHARD_H = 131, 9


@functools.lru_cache(maxsize=None)
def shards():
    """(ref, own, [pixel index arrays]): a 131 x 9 frame -- the left half bright, the right half dark -- and the flat pixel indices of four
    shards: the left half, the right half without its last two pixels, ONE pixel, and one pixel that is not valid"""
    rng = np.random.default_rng(77)
    w, h = SHARD_W, SHARD_H
    ref = rng.random((h, w, 4), dtype=np.float32)
    own = rng.random((h, w, 4), dtype=np.float32)
    ref[..., 3] = (rng.random((h, w)) < 0.8).astype(np.float32)
    own[:, :w // 2, :3] *= np.float32(40.0)
    own[:, w // 2:, :3] *= np.float32(0.05)
    ref[h - 1, w - 2, 3] = 1.0      # the one-pixel shard: valid
    ref[h - 1, w - 1, 3] = 0.0      # the shard without a valid pixel
    idx = np.arange(w * h).reshape(h, w)
    parts = [idx[:, :w // 2].ravel(), idx[:, w // 2:].ravel()[:-2], idx[h - 1, w - 2:w - 1].ravel(), idx[h - 1, w - 1:].ravel()]
    assert sorted(np.concatenate(parts).tolist()) == list(range(w * h))
    ref.setflags(write=False)
    own.setflags(write=False)
    return ref, own, parts
