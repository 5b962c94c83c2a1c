"""The scenes of tests/trip_edge_cases.py do what tests/test_gpu_trip_edges.py needs them to do -- shown from the oracle and from numpy
alone, without a GPU: camera walks that end on the cap of 128 collisions, camera walks that accept at every place of a trip up to the cap,
and a volume whose sizes are no multiple of anything the addressing could take for granted."""
import numpy as np
import pytest

import trip_edge_cases as te

W, H = te.W, te.H


@pytest.fixture(scope="module")
def frames(orc, sc):
    """per case: (scene, camera, the oracle's gen_rays frame)"""
    out = {}
    for name in te.CASES:
        scene, cam = te.make_case(sc, name)
        out[name] = (scene, cam, orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, te.FRAME_RANDOM[name], threads=8))
    return out


def test_cap_pixels_scatter_only_through_the_cap(frames):
    """an empty medium accepts nothing: a pixel with info == 1 is a camera walk that hit the cap.  At least 90 % of the pixels whose ray enters
    the box are such pixels, and each of them alone drew its 128 look-ups"""
    scene, cam, o = frames["cap"]
    assert int(scene["density"].max()) == 0 and scene["density_factor"] == te.DENSITY_FACTOR
    inside = te.enters_box(scene, cam)
    capped = o["info"] == 1
    print("cap: %d pixels enter the box, %d of them capped, %d capped in all, n_fetch %d" %
          (inside.sum(), (capped & inside).sum(), capped.sum(), o["n_fetch"]))
    assert inside.sum() >= 1024
    assert (capped & inside).sum() >= 0.9 * inside.sum()
    assert o["n_fetch"] >= 128 * int((capped & inside).sum())


def test_late_accept_certificate(orc, frames):
    """camera walks that end by acceptance at the last collisions before the cap and at the first collision of a trip: at least 8 pixels
    accept at collision 127 or 128, at least 8 at an odd collision >= 3.  The restated chain agrees with the oracle wherever it can be
    compared: a scattered pixel's walk drew as many free flights as the chain says, or was capped where the chain accepts nothing"""
    scene, cam, o = frames["late_accept"]
    assert int(scene["density"].min()) == 1 and int(scene["density"].max()) == 1
    acc, first, lengths, info = te.certified_acceptances(orc, scene, cam, te.FRAME_RANDOM["late_accept"])
    assert np.array_equal(info, o["info"])
    scattered = info == 1
    want = np.where(first > 0, first, 128)
    assert np.array_equal(lengths[scattered], want[scattered])
    # a walk that left the box did so before the chain's acceptance
    assert (lengths[~scattered & te.enters_box(scene, cam) & (lengths > 0)] <= want[~scattered & te.enters_box(scene, cam) & (lengths > 0)]).all()
    late = int(((acc == 127) | (acc == 128)).sum())
    odd = int(((acc >= 3) & (acc % 2 == 1)).sum())
    capped = int((scattered & (first == 0)).sum())
    print("late accept: %d scattered, %d accept at 127 / 128 (%d / %d), %d at an odd collision >= 3, %d capped; by collision: %s" %
          (scattered.sum(), late, (acc == 127).sum(), (acc == 128).sum(), odd, capped, np.bincount(acc.ravel(), minlength=129)[1:].tolist()))
    assert late >= 8 and odd >= 8


def test_odd_box_cells(frames):
    """no size is a power of two or a multiple of the cell; occupied, empty and cut cells exist, an occupied and an empty cell are neighbours,
    and the frame scatters"""
    scene, cam, o = frames["odd_box"]
    vol = scene["density"]
    assert vol.shape == te.ODD_DIMS[::-1] and scene["dims"] == te.ODD_DIMS
    for n in te.ODD_DIMS:
        assert n % te.CELL != 0 and n & (n - 1) != 0
    occupied, cut = te.cells(vol)
    assert (occupied & ~cut).any() and (~occupied).any() and (occupied & cut).any() and (~occupied & cut).any()
    neighbours = any((np.diff(occupied.astype(np.int8), axis=a) != 0).any() for a in range(3))
    assert neighbours
    # an occupied cell holds zero voxels too (a set bit does not promise density)
    nz, ny, nx = vol.shape
    occupied_voxels = np.repeat(np.repeat(np.repeat(occupied, te.CELL, axis=0), te.CELL, axis=1), te.CELL, axis=2)[:nz, :ny, :nx]
    assert ((vol == 0) & occupied_voxels).any() and not (vol[~occupied_voxels] != 0).any()
    assert (o["info"] == 1).sum() >= 256, int((o["info"] == 1).sum())
