"""tests/far_cut_reference.py bites: on the media and views of tests/far_cut_cases.py the stated bound (farthest corner of every touching
box, grown) is never below the distance at which a pixel's ray leaves its last non-empty voxel, and deliberately wrong rules are caught
by the same comparison that tests/test_gpu_far_cut.py applies to the kernels' bounds."""
import numpy as np
import pytest

import far_cut_cases as fc
import far_cut_reference as far
import skip_reference as ref

CASES = [(m, v, f) for m in fc.MEDIA for v in fc.VIEWS for f in (("64x64", "72x40", "two-strips") if m != "cloud16" else ("64x64",))]


def _case(medium, view, frame_name):
    vol = fc.volume(medium)
    size = fc.size_of(vol)
    W, H, tile, lw = fc.frame(frame_name)
    cam = fc.view(view, vol, W / H)
    return vol, size, cam, W, H, tile, lw


@pytest.mark.parametrize("medium,view,frame_name", CASES)
def test_the_stated_bound_is_never_below_the_last_density(medium, view, frame_name):
    vol, size, cam, W, H, tile, lw = _case(medium, view, frame_name)
    last = fc.last_density(medium, view, frame_name)
    bound = far.tile_far(ref.boxes(vol, size), cam, W, H, far.voxel_diagonal(vol, size), tile)
    assert far.violations(bound, last, lw, H) == []
    # the boxes stand a voxel off the density: even without the margin the farthest corner is behind it
    assert far.violations(far.tile_far(ref.boxes(vol, size), cam, W, H, 0.0, tile, margin=False), last, lw, H) == []


@pytest.mark.parametrize("medium", ["sphere", "blobs", "slab", "cloud16"])
def test_the_nearest_corner_rule_is_caught(medium):
    vol, size, cam, W, H, tile, lw = _case(medium, "head-on", "64x64")
    last = fc.last_density(medium, "head-on", "64x64")
    assert np.isfinite(last).sum() > 16                     # (rays meet density)
    wrong = far.tile_far(ref.boxes(vol, size), cam, W, H, far.voxel_diagonal(vol, size), tile, corner="nearest")
    assert len(far.violations(wrong, last, lw, H)) > 0


def test_a_bound_from_the_front_blob_alone_is_caught():
    """two blobs, one behind the other: the far one sets the bound of the tiles both project onto"""
    vol, size, cam, W, H, tile, lw = _case("blobs", "head-on", "64x64")
    last = far.last_density_distance(vol, size, cam, W, H, tile)
    front = np.array(vol)
    front[fc.FAR_BLOB] = 0
    last_front = far.last_density_distance(front, size, cam, W, H, tile)
    both = np.isfinite(last_front) & (last > last_front + 17 * float(size[0]) / fc.N)      # (the gap between the blobs)
    assert both.sum() >= 4
    wrong = far.tile_far(ref.boxes(front, size), cam, W, H, far.voxel_diagonal(vol, size), tile)
    assert len(far.violations(wrong, last, lw, H)) >= both.sum()


def test_an_untouched_tile_keeps_zero_and_a_missed_ray_minus_infinity():
    vol, size, cam, W, H, tile, lw = _case("corner", "head-on", "64x64")
    bound = far.tile_far(ref.boxes(vol, size), cam, W, H, far.voxel_diagonal(vol, size), tile)
    last = far.last_density_distance(vol, size, cam, W, H, tile)
    assert (bound == 0).any() and (bound > 0).any()
    assert np.isneginf(last).any() and np.isfinite(last).any()
    assert not np.isfinite(last[far.per_pixel(bound, lw, H) == 0]).any()      # density only where a box is seen
