"""The CPU statement of SetVolumeBricks (include/nrc_hpm.h, nrc_renderer_set_volume_bricks): scene.volume_to_bricks / bricks_to_volume
and the VDB reader's brick output (io_vdb.read_vdb_bricks), which must be interchangeable with the dense path it stands beside."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

VDB = os.path.join(GOLDEN, "cloud_sixteenth_excerpt.vdb")
FILE_BBOX = ((-16, -19, -16), (31, -1, 23))
SNAPPED = ((-16, -24, -16), (31, -1, 23))


def random_sparse(shape=(70, 45, 61), seed=5, dtype=np.uint8):
    """[nz][ny][nx] = 70 x 45 x 61 (nx 61: not a multiple of 8 or 4): a few blobs and scattered voxels, most cells empty"""
    rng = np.random.default_rng(seed)
    v = np.zeros(shape, np.uint8)
    idx = rng.integers(0, v.size, 300)
    v.reshape(-1)[idx] = rng.integers(1, 256, idx.size).astype(np.uint8)
    v[10:23, 30:45, 50:61] = rng.integers(0, 256, (13, 15, 11)).astype(np.uint8)      # up to the x and y edges
    v[60:70, 0:9, 0:3] = 77                                                            # up to the z edge
    return v if dtype == np.uint8 else (v.astype(np.float32) / np.float32(255.0))


@pytest.mark.parametrize("name", ["cloud16", "random61x45x70", "random_f32", "zeros"])
def test_round_trip(sc, cloud16, name):
    v = {"cloud16": cloud16, "random61x45x70": random_sparse(), "random_f32": random_sparse(dtype=np.float32),
         "zeros": np.zeros((70, 45, 61), np.uint8)}[name]
    origins, bricks = sc.volume_to_bricks(v)
    assert origins.dtype == np.int32 and origins.shape == (len(bricks), 3) and origins.flags.c_contiguous
    assert bricks.dtype == v.dtype and bricks.shape == (len(origins), 8, 8, 8) and bricks.flags.c_contiguous
    back = sc.bricks_to_volume(origins, bricks, v.shape)
    assert back.dtype == v.dtype and np.array_equal(back, v)
    assert (origins % 8 == 0).all() and (origins >= 0).all()
    if name == "zeros":
        assert len(origins) == 0
        return
    assert (origins < np.array(v.shape[::-1])).all()
    assert bricks.reshape(len(bricks), -1).any(axis=1).all()          # only cells that hold something
    order = (origins[:, 2].astype(np.int64) << 40) | (origins[:, 1].astype(np.int64) << 20) | origins[:, 0]
    assert (np.diff(order) > 0).all()                                  # cell order z, y, x, no cell twice


def test_cloud16_brick_count_and_layout(sc, cloud16):
    origins, bricks = sc.volume_to_bricks(cloud16)
    assert cloud16.shape == (154, 86, 126)
    assert len(origins) == 1233
    # element 64 * dz + 8 * dy + dx of brick i is voxel (x0 + dx, y0 + dy, z0 + dz)
    i = int(np.argmax(bricks.reshape(len(bricks), -1).astype(bool).sum(axis=1)))
    x0, y0, z0 = origins[i]
    flat = bricks.reshape(len(bricks), 512)
    for dx, dy, dz in ((0, 0, 0), (7, 0, 0), (1, 2, 3), (5, 7, 6)):
        if x0 + dx < 126 and y0 + dy < 86 and z0 + dz < 154:
            assert flat[i, 64 * dz + 8 * dy + dx] == cloud16[z0 + dz, y0 + dy, x0 + dx]


def test_highest_index_wins_on_duplicates(sc):
    origins = np.array([[8, 0, 16], [0, 0, 0], [8, 0, 16], [8, 0, 16]], np.int32)
    bricks = np.zeros((4, 8, 8, 8), np.uint8)
    bricks[0] = 10
    bricks[1] = 20
    bricks[2] = 30
    bricks[3, 1, 2, 3] = 40           # the winner is taken whole: its zeros replace the earlier bricks' values too
    v = sc.bricks_to_volume(origins, bricks, (24, 8, 16))
    want = np.zeros((24, 8, 16), np.uint8)
    want[0:8, 0:8, 0:8] = 20
    want[16 + 1, 2, 8 + 3] = 40
    assert np.array_equal(v, want)


def test_edge_bricks_are_cropped_and_invalid_origins_refused(sc):
    origins = np.array([[8, 8, 8]], np.int32)
    bricks = np.arange(512, dtype=np.float32).reshape(1, 8, 8, 8) + 1
    v = sc.bricks_to_volume(origins, bricks, (13, 10, 11))          # nz 13, ny 10, nx 11: 5 x 2 x 3 voxels of the brick remain
    want = np.zeros((13, 10, 11), np.float32)
    want[8:13, 8:10, 8:11] = bricks[0, :5, :2, :3]
    assert np.array_equal(v, want)
    for bad in ([4, 8, 8], [8, 8, 16], [16, 0, 0], [-8, 0, 0]):      # unaligned, z0 >= nz, x0 >= nx, negative
        o = np.array([[0, 0, 0], bad], np.int32)
        b = np.ones((2, 8, 8, 8), np.float32)
        with pytest.raises(ValueError, match="brick 1"):
            sc.bricks_to_volume(o, b, (13, 10, 11))
        skipped = sc.bricks_to_volume(o, b, (13, 10, 11), ignore_invalid=True)
        assert np.array_equal(skipped, sc.bricks_to_volume(o[:1], b[:1], (13, 10, 11)))


def test_aligned_bbox():
    from nrc_hpm_renderer_amd import io_vdb
    assert io_vdb.vdb_bbox(VDB) == FILE_BBOX
    assert io_vdb.aligned_bbox(FILE_BBOX) == SNAPPED
    assert io_vdb.aligned_bbox(((0, 7, 8), (5, 7, 9))) == ((0, 0, 8), (5, 7, 9))
    assert io_vdb.aligned_bbox(((-1, -8, -9), (0, 0, 0))) == ((-8, -8, -16), (0, 0, 0))
    assert io_vdb.aligned_bbox(io_vdb.aligned_bbox(FILE_BBOX)) == SNAPPED


def test_read_vdb_bricks_equals_the_dense_reader(sc):
    from nrc_hpm_renderer_amd import io_vdb
    dense, info = io_vdb.read_vdb_dense(VDB, SNAPPED)              # [x][y][z]
    want = np.ascontiguousarray(dense.transpose(2, 1, 0))          # [nz][ny][nx], the order quantize_density hands to SetVolume
    origins, bricks = io_vdb.read_vdb_bricks(VDB, SNAPPED)
    assert origins.dtype == np.int32 and bricks.dtype == np.float32 and bricks.shape == (len(origins), 8, 8, 8)
    assert len(origins) > 0 and want.any()
    got = sc.bricks_to_volume(origins, bricks, want.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # and quantised, it is the uint8 volume the --vdb path uploads
    assert np.array_equal(sc.quantize_density(dense), (got * np.float32(255.0)).astype(np.uint8))
    # a bbox that cuts through leaves: the crop is the dense reader's
    cut = ((-8, -16, 0), (20, -6, 17))
    want = np.ascontiguousarray(io_vdb.read_vdb_dense(VDB, cut)[0].transpose(2, 1, 0))
    got = sc.bricks_to_volume(*io_vdb.read_vdb_bricks(VDB, cut), want.shape)
    assert want.any() and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_read_vdb_bricks_needs_an_aligned_minimum():
    from nrc_hpm_renderer_amd import io_vdb
    with pytest.raises(ValueError, match="multiple of 8"):
        io_vdb.read_vdb_bricks(VDB, FILE_BBOX)
