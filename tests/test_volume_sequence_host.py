"""VDB sequences for animated media (host side): densifying over a given bbox (crop / zero-pad), the union bbox of a sequence, and the
CLI's refusal to benchmark a moving medium -- no GPU needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

VDB = os.path.join(GOLDEN, "cloud_sixteenth_excerpt.vdb")


@pytest.fixture(scope="module")
def io_vdb():
    from nrc_hpm_renderer_amd import io_vdb as m
    return m


@pytest.fixture(scope="module")
def own(io_vdb):
    vol, info = io_vdb.read_vdb_dense(VDB)
    return vol, info


def test_union_bbox_of_a_file_with_itself_is_its_bbox(io_vdb, own):
    _, info = own
    lo, hi = io_vdb.union_bbox([VDB, VDB])
    assert lo == tuple(int(v) for v in info["bbox_min"]) and hi == tuple(int(v) for v in info["bbox_max"])
    assert io_vdb.vdb_bbox(VDB) == (lo, hi)


def test_densify_over_an_enlarged_bbox_is_the_zero_padded_volume(io_vdb, own):
    vol, info = own
    lo, hi = np.array(info["bbox_min"]), np.array(info["bbox_max"])
    pad_lo, pad_hi = np.array([3, 0, 5]), np.array([2, 7, 1])
    big, binfo = io_vdb.read_vdb_dense(VDB, (tuple(lo - pad_lo), tuple(hi + pad_hi)))
    want = np.pad(vol, [(int(a), int(b)) for a, b in zip(pad_lo, pad_hi)])
    assert big.shape == want.shape
    assert np.array_equal(big, want)
    assert binfo["bbox_min"] == info["bbox_min"]      # (the file's own bbox is still reported)
    # from_vdb keeps the normalisation check and hands back the same grid
    fv, _ = io_vdb.from_vdb(VDB, (tuple(lo - pad_lo), tuple(hi + pad_hi)))
    assert np.array_equal(fv, want)


def test_densify_over_a_smaller_bbox_is_the_crop(io_vdb, own):
    vol, info = own
    lo, hi = np.array(info["bbox_min"]), np.array(info["bbox_max"])
    c_lo = lo + np.array([4, 9, 1])
    c_hi = hi - np.array([6, 2, 11])
    crop, _ = io_vdb.read_vdb_dense(VDB, (tuple(c_lo), tuple(c_hi)))
    a, b = c_lo - lo, c_hi - lo + 1
    assert np.array_equal(crop, vol[a[0]:b[0], a[1]:b[1], a[2]:b[2]])
    # a bbox that straddles the file's: cropped on one side, zero-padded on the other
    s_lo, s_hi = lo + np.array([5, -3, 0]), hi + np.array([4, -8, 2])
    mixed, _ = io_vdb.read_vdb_dense(VDB, (tuple(s_lo), tuple(s_hi)))
    want = np.zeros(tuple(s_hi - s_lo + 1), np.float32)
    src_lo, src_hi = np.maximum(s_lo, lo), np.minimum(s_hi, hi) + 1
    want[tuple(slice(int(x - y), int(z - y)) for x, y, z in zip(src_lo, s_lo, src_hi))] = \
        vol[tuple(slice(int(x - y), int(z - y)) for x, y, z in zip(src_lo, lo, src_hi))]
    assert np.array_equal(mixed, want)


def test_cli_rejects_benchmark_of_a_sequence_without_touching_the_gpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", "import sys; from nrc_hpm_renderer_amd import cli; sys.exit(cli.main(sys.argv[1:]))",
                        "--vdb", VDB, VDB, "--benchmark", "--frames", "1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0
    assert "SkyRenderer ERROR" in p.stderr and "--benchmark" in p.stderr, p.stderr
