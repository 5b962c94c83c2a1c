"""What the tests of sparse volume keys share (test_volume_key_bricks_host.py on the CPU, test_gpu_volume_key_bricks.py on the GPU): the key
sequence of tests/test_gpu_volume_keys.py rebuilt here -- the fixture cloud cropped / padded, a rolled copy, an all-zero key and the synthetic
pair -- its tested times, and the keys as brick lists."""
import numpy as np

# (nz, ny, nx): the smallest shapes at which k_vol_ingest takes another path (ragged, vector, two chunks, two chunks scalar); no dims a
# multiple of 8 except 64^3
SHAPES = {"61x45x70-ragged-no-vec": (70, 45, 61), "64^3-vec": (64, 64, 64), "264x9x10-two-chunks-vec": (10, 9, 264),
          "261x9x10-two-chunks-no-vec": (10, 9, 261)}
N_KEYS = 5      # cloud, rolled cloud, zeros, synthetic A, synthetic B
WEIGHTS = (0, 1, 128, 129, 255, 256)


def _fit(vol, shape):
    """the middle of `vol`, cropped or padded with zeros to `shape`"""
    out = np.zeros(shape, np.uint8)
    src, dst = [], []
    for n, m in zip(vol.shape, shape):
        k = min(n, m)
        src.append(slice((n - k) // 2, (n - k) // 2 + k))
        dst.append(slice((m - k) // 2, (m - k) // 2 + k))
    out[tuple(dst)] = vol[tuple(src)]
    return out


def _synthetic_pair(shape):
    """key A: isolated voxels of value 1 and 255 (alternating) on cell corners, cell edges and the volume's faces, every one alone in
    its 8^3 cell and with empty cells around it where the shape allows; key B: zero there and non-zero everywhere else"""
    nz, ny, nx = shape
    a = np.zeros(shape, np.uint8)
    spots = []
    for cz in range(0, (nz + 7) // 8, 2):
        for cy in range(0, (ny + 7) // 8, 2):
            for cx in range(0, (nx + 7) // 8, 2):
                k = len(spots)
                corner = ((0, 0, 0), (7, 7, 7), (7, 0, 7), (0, 7, 0))[k % 4]
                edge = ((0, 0, 3), (7, 4, 7), (2, 7, 0))[k % 3]
                dz, dy, dx = corner if k % 2 == 0 else edge
                spots.append((min(cz * 8 + dz, nz - 1), min(cy * 8 + dy, ny - 1), min(cx * 8 + dx, nx - 1)))
    spots += [(0, ny // 2, nx // 2), (nz - 1, ny // 2, nx // 3), (nz // 2, 0, nx // 2), (nz // 3, ny - 1, nx // 2), (nz // 2, ny // 2, 0),
              (nz // 2, ny // 3, nx - 1), (nz - 1, ny - 1, nx - 1), (0, 0, 0)]
    for k, p in enumerate(spots):
        a[p] = 1 if (k // 2) % 2 == 0 else 255
    rng = np.random.default_rng(nx * 1000 + ny)
    b = np.where(a != 0, 0, rng.integers(1, 256, shape)).astype(np.uint8)
    return a, b


_KEYS, _BRICKS = {}, {}


def keys_of(cloud16, shape):
    """the dense key sequence of a shape (computed once, never written to)"""
    if shape not in _KEYS:
        cloud = _fit(cloud16, shape)
        rolled = np.ascontiguousarray(np.roll(cloud, (shape[0] // 3, -(shape[1] // 4), shape[2] // 5), axis=(0, 1, 2)))
        a, b = _synthetic_pair(shape)
        keys = np.ascontiguousarray(np.stack([cloud, rolled, np.zeros(shape, np.uint8), a, b]))
        keys.setflags(write=False)
        _KEYS[shape] = keys
    return _KEYS[shape]


def key_bricks_of(sc, cloud16, shape):
    """the same sequence as (counts, origins, bricks) of scene.volumes_to_key_bricks (computed once, never written to)"""
    if shape not in _BRICKS:
        parts = sc.volumes_to_key_bricks(keys_of(cloud16, shape))
        for p in parts:
            p.setflags(write=False)
        _BRICKS[shape] = parts
    return _BRICKS[shape]


def time_of(i, W):
    """a time whose key pair and weight are exactly (i, W), W = 256 included (the last fp32 below i + 1)"""
    return float(np.nextafter(np.float32(i + 1), np.float32(0))) if W == 256 else i + W / 256.0


def times_of(shape):
    """the tested times of a shape's keys: every pair at WEIGHTS and two seeded weights, and the last key itself"""
    rng = np.random.default_rng(shape[2])
    ts = [time_of(i, W) for i in range(N_KEYS - 1) for W in WEIGHTS + tuple(int(w) for w in rng.integers(2, 255, 2))]
    return ts + [float(N_KEYS - 1)]


def cells_of(vol):
    """[gz][gy][gx] bool: the 8^3 cells of a volume that hold a non-zero voxel (= the cells volume_to_bricks makes bricks of)"""
    nz, ny, nx = vol.shape
    p = np.zeros(((nz + 7) // 8 * 8, (ny + 7) // 8 * 8, (nx + 7) // 8 * 8), bool)
    p[:nz, :ny, :nx] = vol != 0
    return p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8, p.shape[2] // 8, 8).any(axis=(1, 3, 5))
