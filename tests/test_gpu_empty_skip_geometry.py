"""The exact empty-space skip against geometry.  Its other tests are equivalences between two product paths (device rebuild == host builder,
tile-parallel mask == box-parallel mask, a frame with the skip == the frame without); here the occupancy bits, the dilated boxes and the
per-camera tile mask are compared with tests/skip_reference.py, a plain fp64 statement of what they must be:

  bits and boxes   bit for bit the reference's, at creation and after a device rebuild from uint8 and from float32, on both renderers
  tile mask        needed (camera rays against occupied cells) <= mask <= allowed (projected boxes, grown by two pixels), the off word as
                   the eye plane demands, both builds (k_tile_mask; k_tile_rects + k_tile_mask_words) word for word the same -- on volumes
                   with more than two chunks of boxes, frames wider than 32 tiles and sharded frames (tests/skip_cases.py)

tests/test_skip_reference_cpu.py shows that these bounds reject a mask rule that is subtly wrong."""
import numpy as np
import pytest

import skip_cases as sk
import skip_reference as ref
from volume_common import _to_f32

pytestmark = pytest.mark.gpu

CFG = dict(train_batch_count=1, log2_train_batch_size=10, log2_infer_batch_size=14)


def _make(api, kind, vol, W, H, cam, tile=None):
    scene = sk.sc.make_scene(vol, scene_id=4)
    if kind == "mc":
        return api.McHpmRenderer(W, H, 8, False, cam, scene, tile=tile), None
    cfg = api.AppConfig(**CFG)
    nrc = api.NeuralRadianceCache(cfg)
    return api.NrcHpmRenderer(W, H, False, cam, cfg, scene, nrc, tile=tile), nrc


def _destroy(*pairs):
    for ren, nrc in pairs:
        ren.Destroy()
        if nrc is not None:
            nrc.Destroy()


# ---------------------------------------------------------------------------------------------------------------- bits and boxes
@pytest.mark.parametrize("kind", ["nrc", "mc"])
@pytest.mark.parametrize("vol_name", ["cloud16", "lone", "many", "sparse512"])
def test_occupancy_bits_and_boxes_are_the_reference_s(api, torch_gpu, kind, vol_name):
    """VolumeBuffer("occ_bits") and ("boxes") == occupancy_bits() and boxes(), bitwise: the creation build, then device rebuilds from
    uint8 and float32 tensors (the renderer is created with another medium of the same size, so a rebuild that did nothing would show).
    (Brick and keyframe sources are bitwise the dense rebuild -- test_gpu_volume_bricks.py, test_gpu_volume_keys.py.)"""
    import torch
    vol = sk.volume(vol_name)
    want_bits, edge = ref.occupancy_bits(vol)
    want_boxes = sk.boxes_of(vol_name)
    assert edge == (16 if vol_name == "sparse512" else 8)
    assert (want_boxes.shape[0] > 2048) == (vol_name in ("many", "sparse512"))      # (more than two chunks of the tile-parallel build)
    cam = sk.sc.make_camera(aspect=2.0)

    def check(ren, what):
        bits = ren.VolumeBuffer("occ_bits").cpu().numpy().view(np.uint32)
        bx = ren.VolumeBuffer("boxes").cpu().numpy()
        assert np.array_equal(ren.VolumeBuffer("density").cpu().numpy(), vol), what
        assert bits.shape == want_bits.shape and np.array_equal(bits, want_bits), (what, bits.shape, want_bits.shape)
        assert bx.shape == want_boxes.shape, (what, bx.shape, want_boxes.shape)
        assert np.array_equal(bx.view(np.uint32), want_boxes.view(np.uint32)), what
        return bx

    fresh = _make(api, kind, vol, 32, 16, cam)
    bx = check(fresh[0], "creation")
    _destroy(fresh)
    # the covering property, on what the device holds, without building runs
    assert ref.covering_errors(vol, sk.size_of(vol), bx) == []
    other = np.ascontiguousarray(np.flip(vol, axis=0) // 2 + 1)
    live = _make(api, kind, other, 32, 16, cam)
    for what, src in (("uint8 tensor", torch.from_numpy(np.array(vol)).cuda()), ("float32 tensor", torch.from_numpy(_to_f32(vol)).cuda())):
        live[0].SetVolume(src)
        check(live[0], what)
        live[0].SetVolume(torch.from_numpy(other).cuda())
    _destroy(live)


# ---------------------------------------------------------------------------------------------------------------- tile mask
def _render(ren, kind):
    if kind == "mc":
        ren.Render()
    else:
        ren.Render(None, False)


@pytest.mark.parametrize("kind", ["nrc", "mc"])
@pytest.mark.parametrize("vol_name,frame_name,views", sk.CASES, ids=sk.CASE_IDS)
def test_tile_mask_lies_between_the_geometric_bounds(api, torch_gpu, kind, vol_name, frame_name, views):
    """per view, with the box count on the host (creation) and in device memory (after a device rebuild of the same medium):
    TileMask() after SetCamera + Render == TileMask() after a one-view RenderPath; the off word is what off_expected demands; when the mask
    is on, no needed tile is clear and (views with every corner at w >= 1) no tile is set outside the allowed ones; the bits behind the last
    tile are clear.  No margin of the reference is to be widened for a case: a needed tile that is clear is a wrong frame."""
    import torch
    vol = sk.volume(vol_name)
    W, H, tile, lw = sk.frame(frame_name)
    cams = [sk.view(v, vol_name, W / H) for v in views]
    old, new = _make(api, kind, vol, lw, H, cams[-1], tile=tile), _make(api, kind, vol, lw, H, cams[-1], tile=tile)
    fr = sk.sc.frame_randoms(1, seed=3)
    for medium in ("creation", "device rebuild"):
        if medium == "device rebuild":
            for ren, _ in (old, new):
                ren.SetVolume(torch.from_numpy(np.array(vol)).cuda())
        for name, cam in zip(views, cams):
            r = sk.reference_of(vol_name, frame_name, name)
            old[0].SetCamera(None, cam)
            old[0].SetFrameRandom(fr[0])
            _render(old[0], kind)
            want = old[0].TileMask()
            new[0].RenderPath([cam], 1, fr, out=False)
            got = new[0].TileMask()
            mask, tail, off = ref.unpack_mask(want, lw, H)
            print("%s %s %s %s, %s: off %d (expected %s), set / needed / allowed = %d / %d / %s of %d tiles" % (
                kind, vol_name, frame_name, name, medium, off, r.off, mask.sum(), r.needed.sum(),
                "-" if r.allowed is None else r.allowed.sum(), mask.size))
            where = (medium, name)
            assert np.array_equal(got, want), (where, [hex(int(x)) for x in got[:4]], [hex(int(x)) for x in want[:4]])
            assert off in (0, 1) and not tail.any(), (where, off, tail)
            if r.off is not None:
                assert bool(off) == r.off, (where, off, r.off)
            if off:
                continue
            assert not (r.needed & ~mask).any(), (where, "needed tiles are clear (ty, tx)", np.argwhere(r.needed & ~mask).tolist())
            if r.allowed is not None:
                assert not (mask & ~r.allowed).any(), (where, "tiles set that no box projects onto (ty, tx)", np.argwhere(mask & ~r.allowed).tolist())
    _destroy(old, new)
