"""tests/skip_reference.py bites.  The GPU tests of the empty-space skip (test_gpu_empty_skip_geometry.py) bound the kernels' tile mask
between needed_tiles (camera rays against occupied cells) and allowed_tiles (projected boxes, generously grown).  Here, without a GPU, a
numpy restatement of the mask rule -- a box's corners projected in fp32, the rectangle around them grown by a pixel, the tiles it touches --
lies between the bounds on every case the GPU tests use, and broken variants of the rule are rejected: were the bounds so loose that they
passed those, the GPU tests would show nothing."""
import numpy as np
import pytest

import skip_cases as sk
import skip_reference as ref


# ---------------------------------------------------------------------------------------------------------------- the rule
def rule_tiles(boxes, cam, W, H, tile=None, mirror_y=False, outward_strips=False):
    """(bool [tiles_y][tiles_x], off): the mask rule as the tile-mask section of csrc/nrc_integrator.hip states it.  The forward transform is
    the fp64 inverse of inv_proj_view rounded to fp32; the projection runs in fp32."""
    f32 = np.float32
    fwd = np.linalg.inv(np.asarray(cam["inv_proj_view"], np.float64).reshape(4, 4).T).astype(f32)
    cols = ref.local_columns(W, tile)
    block = 1 if tile is None else tile[4]
    ty, tx = ref.tiles_of(cols.size, H)
    mask, off = np.zeros((ty, tx), bool), False
    b = np.asarray(boxes, f32).reshape(-1, 6)
    for lo_x, lo_y, lo_z, hi_x, hi_y, hi_z in b:
        corners = np.array([(x, y, z, 1.0) for z in (lo_z, hi_z) for y in (lo_y, hi_y) for x in (lo_x, hi_x)], f32)
        clip = (corners[:, None, :] * fwd[None, :, :]).sum(axis=2, dtype=f32)
        if not (clip[:, 3] > f32(1.0e-3)).all():
            off = True
            continue
        nx, ny = clip[:, 0] / clip[:, 3], clip[:, 1] / clip[:, 3]
        if mirror_y:
            ny = -ny
        gx0, gx1 = np.floor((nx.min() + f32(1)) * f32(0.5) * f32(W)) - 1, np.ceil((nx.max() + f32(1)) * f32(0.5) * f32(W)) + 1
        gy0, gy1 = np.floor((ny.min() + f32(1)) * f32(0.5) * f32(H)) - 1, np.ceil((ny.max() + f32(1)) * f32(0.5) * f32(H)) + 1
        # local columns: all of every strip the rectangle touches
        strip = cols // block
        s0, s1 = np.floor(gx0 / block), np.floor(gx1 / block)
        if outward_strips:      # the first and last local strip rounded away from the rectangle (what the kernel did before this test existed)
            rank, world = tile[0], tile[1]
            s0, s1 = rank + world * np.floor((s0 - rank) / world), rank + world * np.ceil((s1 - rank) / world)
        lx = np.flatnonzero((strip >= s0) & (strip <= s1))
        y0, y1 = int(max(gy0, 0)), int(min(gy1, H - 1))
        if lx.size == 0 or y0 > y1:
            continue
        mask[y0 // 8:y1 // 8 + 1, lx.min() // 8:lx.max() // 8 + 1] = True
    return mask, off


def _shift(mask):
    out = np.zeros_like(mask)
    out[:, 1:] = mask[:, :-1]
    return out


def _erode(mask):
    p = np.pad(mask, 1)
    return mask & p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]


def _one_cell_short(boxes, vol_name):
    """every x-run ends a cell early (a run of one cell keeps no width)"""
    v = sk.volume(vol_name)
    b = np.array(boxes, np.float32)
    b[:, 3] = np.maximum(b[:, 0], b[:, 3] - np.float32(8.0 * float(sk.size_of(v)[0]) / v.shape[2]))
    return b


MUTANTS = {
    "runs-one-cell-short": lambda r, vol: rule_tiles(_one_cell_short(r.boxes, vol), r.cam, r.W, r.H, r.tile)[0],
    "y-mirrored": lambda r, vol: rule_tiles(r.boxes, r.cam, r.W, r.H, r.tile, mirror_y=True)[0],
    "shifted-one-tile": lambda r, vol: _shift(rule_tiles(r.boxes, r.cam, r.W, r.H, r.tile)[0]),
    "eroded-one-tile": lambda r, vol: _erode(rule_tiles(r.boxes, r.cam, r.W, r.H, r.tile)[0]),
    "second-chunk-dropped": lambda r, vol: rule_tiles(r.boxes[:1024], r.cam, r.W, r.H, r.tile)[0],
    "sharded-strips-rounded-outward": lambda r, vol: rule_tiles(r.boxes, r.cam, r.W, r.H, r.tile, outward_strips=True)[0],
    "all-set": lambda r, vol: np.ones_like(r.needed),
    "all-clear": lambda r, vol: np.zeros_like(r.needed),
}


def _between(mask, r):
    """'' or what is wrong with a mask of a view whose mask is on"""
    if (r.needed & ~mask).any():
        return "%d needed tiles are clear" % int((r.needed & ~mask).sum())
    if r.allowed is not None and (mask & ~r.allowed).any():
        return "%d tiles are set that no box projects onto" % int((mask & ~r.allowed).sum())
    return ""


def _on_cases():
    """(volume, frame, view, reference) of every case whose mask must be on"""
    for vol, fr, views in sk.CASES:
        for vw in views:
            r = sk.reference_of(vol, fr, vw)
            if r.off is False:
                yield vol, fr, vw, r


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("vol,fr,views", sk.CASES, ids=sk.CASE_IDS)
def test_the_rule_lies_between_the_bounds(vol, fr, views):
    for vw in views:
        r = sk.reference_of(vol, fr, vw)
        mask, off = rule_tiles(r.boxes, r.cam, r.W, r.H, r.tile)
        print("%s %s %s: off %s (expected %s), set / needed / allowed = %d / %d / %s of %d" % (
            vol, fr, vw, off, r.off, mask.sum(), r.needed.sum(), "-" if r.allowed is None else r.allowed.sum(), mask.size))
        if r.off is not None:
            assert off == r.off, (vw, off, r.off)
        if not off:
            assert _between(mask, r) == "", (vw, _between(mask, r))
        if r.allowed is not None:
            assert not (r.needed & ~r.allowed).any(), vw      # the bounds themselves are consistent


def test_the_views_are_of_every_kind():
    """the off views are off and the past view is all clear by the reference alone; some view is partly covered in every case of more than
    one tile; the upper bound applies to most views"""
    for vol, fr, views in sk.CASES:
        kinds = set()
        for vw in views:
            r = sk.reference_of(vol, fr, vw)
            if vw in sk.MUST_BE_OFF:
                assert r.off is True, (vol, fr, vw)
            if vw in sk.MUST_BE_CLEAR and vol != "lone":      # ((b) is long in z: the past view catches its end)
                assert r.off is False and not r.allowed.any(), (vol, fr, vw)
            if r.off is False:
                assert r.allowed is not None, (vol, fr, vw)
                kinds.add("part" if r.needed.any() and not r.allowed.all() else "other")
        assert r.needed.size == 1 or "part" in kinds, (vol, fr)


@pytest.mark.parametrize("name", list(MUTANTS))
def test_broken_rules_are_rejected(name):
    rejected = []
    for vol, fr, vw, r in _on_cases():
        if name == "second-chunk-dropped" and r.boxes.shape[0] <= 1024 or name == "sharded-strips-rounded-outward" and r.tile is None:
            continue
        why = _between(MUTANTS[name](r, vol), r)
        if why:
            rejected.append("%s %s %s: %s" % (vol, fr, vw, why))
    print("\n".join(rejected))
    assert rejected, name


def test_the_issue_s_prototype_rejections_hold():
    """cloud16 at 128x80 alone rejects each geometric mutant; dropping the boxes behind the first chunk of the many-box volume is rejected
    from every view that sees it"""
    for name in ("runs-one-cell-short", "y-mirrored", "shifted-one-tile", "eroded-one-tile"):
        by = [vw for vw in sk.ALL_VIEWS if sk.reference_of("cloud16", "128x80", vw).off is False
              and _between(MUTANTS[name](sk.reference_of("cloud16", "128x80", vw), "cloud16"), sk.reference_of("cloud16", "128x80", vw))]
        print(name, "rejected from", by)
        assert by, name
    for vw in ("many-side", "oblique"):
        r = sk.reference_of("many", "96x56", vw)
        assert _between(MUTANTS["second-chunk-dropped"](r, "many"), r) != "", vw


def test_merged_runs_do_not_change_the_ray_test():
    """needed_tiles tests a ray against x-runs of cells; cell by cell it finds the same tiles"""
    for vol, fr, vw in (("cloud16", "ragged100x52", "orbit"), sk.LONE_VIEW, ("lone", "128x80", "oblique")):
        r = sk.reference_of(vol, fr, vw)
        v = sk.volume(vol)
        assert np.array_equal(r.needed, ref.needed_tiles(v, sk.size_of(v), r.cam, r.W, r.H, r.tile, merge_runs=False)), (vol, fr, vw)


def test_every_lone_box_is_needed():
    """non-vacuity of (b): the neighbours of a box in cloud16 cover its tiles, so a mask that drops one box passes there.  Not here: without any
    one group of voxels the lower bound shrinks, and the tiles lost lie outside the upper bound of what remains"""
    vol, fr, vw = sk.LONE_VIEW
    r = sk.reference_of(vol, fr, vw)
    assert r.off is False and r.allowed is not None
    for name in sk.LONE_VOXELS:
        less = sk.Reference(vol, fr, vw, vol=sk.lone_volume(without=name))
        lost = r.needed & ~less.needed
        assert not (less.needed & ~r.needed).any() and lost.any(), name
        assert (lost & ~less.allowed).any(), name      # (a mask built without the group's boxes cannot cover them by its margins)
        print("%-18s %d tiles of its own" % (name, (lost & ~less.allowed).sum()))


def test_the_first_and_the_last_box_of_the_many_box_volume_stand_alone():
    """(c): from the side view the first box (index 0) and the last box (beyond two chunks of 1024) each own needed tiles that the
    rectangles of all the other boxes, generously grown, do not reach; so dropping either is visible to the lower bound"""
    vol, fr, vw = sk.MANY_VIEW
    r = sk.reference_of(vol, fr, vw)
    assert r.boxes.shape[0] > 2048 and r.off is False
    for which, index in (("first", 0), ("last", r.boxes.shape[0] - 1)):
        less = sk.Reference(vol, fr, vw, vol=sk.many_volume(without=which))
        assert less.boxes.shape[0] == r.boxes.shape[0] - 1
        assert np.array_equal(np.delete(r.boxes, index, axis=0), less.boxes), which
        own = r.needed & ~less.allowed
        assert own.any(), which
        mask = rule_tiles(less.boxes, r.cam, r.W, r.H, r.tile)[0]
        assert _between(mask, r) != "", which


def test_bits_and_boxes_on_a_hand_made_volume():
    """a 20 x 9 x 17 volume with two voxels, worked out by hand"""
    v = np.zeros((17, 9, 20), np.uint8)      # cells: 3 x 2 x 3 (cx, cy, cz)
    v[0, 0, 7] = 5       # cell (0, 0, 0); x + 1 = 8 dilates into cell cx = 1
    v[16, 8, 19] = 1     # the last voxel: cell (2, 1, 2); dilates into cy = 0 (y = 7) and cz = 1 (z = 15), not into cx = 1 (x = 18)
    words, edge = ref.occupancy_bits(v)
    assert edge == 8 and words.size == 4
    assert int(words[0]) == (1 << 0) | (1 << ((2 * 2 + 1) * 3 + 2)) and not words[1:].any()
    cells = ref.dilated_cells(v)
    assert cells.shape == (3, 2, 3) and cells.sum() == 2 + 4
    size = np.array([20.0, 9.0, 17.0], np.float32)      # one world unit per voxel
    bx = ref.boxes(v, size)
    want = np.array([[0, 0, 0, 16, 8, 8], [16, 0, 8, 20, 8, 16], [16, 8, 8, 20, 9, 16], [16, 0, 16, 20, 8, 17], [16, 8, 16, 20, 9, 17]], np.float32)
    want -= np.array([10.0, 4.5, 8.5] * 2, np.float32)
    assert np.array_equal(bx, want), bx
    # 16-voxel cells once 8-voxel ones do not fit
    big = np.zeros((8, 8, 1024), np.uint8)
    big[7, 7, 1023] = 1
    words, edge = ref.occupancy_bits(big, max_words=2)      # 128 cells of 8 > 64 bits; 64 cells of 16 fit
    assert edge == 16 and words.size == 4 and int(words[1]) == 1 << 31 and not words[[0, 2, 3]].any()


@pytest.mark.parametrize("vol", ["cloud16", "lone", "many"])
def test_the_reference_s_boxes_cover_the_dilated_medium(vol):
    """covering_errors (run-free: voxel centres against boxes) accepts boxes() and rejects runs that end early, a dropped box, a doubled box
    and a box that leaves the volume"""
    v, bx = sk.volume(vol), sk.boxes_of(vol)
    size = sk.size_of(v)
    assert ref.covering_errors(v, size, bx) == []
    assert ref.covering_errors(v, size, _one_cell_short(bx, vol))
    assert ref.covering_errors(v, size, bx[1:])
    assert ref.covering_errors(v, size, np.concatenate([bx, bx[-1:]]))
    out = np.array(bx)
    out[-1, 5] += np.float32(0.01)
    assert ref.covering_errors(v, size, out)


def test_off_expected_and_the_upper_bound_s_validity():
    cam = sk.sc.make_camera(pos=(10.0, 0.0, 0.0), aspect=1.6)      # looks along -x: clip w = 10 - x
    box = lambda x0, x1: np.array([[x0, -1, -1, x1, 1, 1]], np.float32)      # noqa: E731
    assert ref.off_expected(box(2.0, 10.5), cam) is True
    assert ref.off_expected(box(2.0, 10.0 - 0.005), cam) is None
    assert ref.off_expected(box(2.0, 10.0 - 0.02), cam) is False
    assert ref.off_expected(np.zeros((0, 6), np.float32), cam) is False
    assert ref.allowed_tiles(box(2.0, 9.5), cam, 128, 80) is None
    assert ref.allowed_tiles(box(2.0, 8.5), cam, 128, 80) is not None
