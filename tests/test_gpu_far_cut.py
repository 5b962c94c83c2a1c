"""The far cut of the camera walk ("Far cut"): the first delta walk of a camera path ends behind the last occupancy
box its tile's rays can pass through.  No stored bit may change -- every frame here is the oracle's, which walks every ray whole --, the
bound the mask builds hand to the kernels is never below the distance at which a pixel's ray leaves its last non-empty voxel
(tests/far_cut_reference.py), both builds give the same bound, and the counting kernels, which keep the whole walk, find no density at
or behind any lane's cut (CutFetches()[1] == 0) while the cut does remove collisions where there is empty space behind the medium
(CutFetches()[0] > 0).  Media, views and frames: tests/far_cut_cases.py."""
import numpy as np
import pytest

import far_cut_cases as fc
import far_cut_reference as far
import rng_search
import skip_reference as ref
from nrc_hpm_renderer_amd import parallel

pytestmark = pytest.mark.gpu

CFG = dict(train_batch_count=1, log2_train_batch_size=10, log2_infer_batch_size=14)
CASES = [(m, v, f) for m in fc.MEDIA for v in fc.VIEWS for f in ("64x64", "72x40")] + \
        [("sphere", "head-on", "two-strips"), ("blobs", "head-on", "two-strips"), ("cloud16", "grazing", "two-strips")]


def same_bits(a, b):
    """bit-identical (a NaN matches a NaN)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _columns(W, tile):
    return slice(None) if tile is None else parallel.rank_columns(tile[0], tile[1], W, tile[4])


def _nrc_renderer(api, scene, cam, lw, H, tile):
    cfg = api.AppConfig(**CFG)
    nrc = api.NeuralRadianceCache(cfg)
    return nrc, api.NrcHpmRenderer(lw, H, False, cam, cfg, scene, nrc, tile=tile)


def _frame_is_the_oracles(ren, o, W, H, lw, sel, what):
    """primary, info, infer_input and the live-query list of the frame just rendered, on every pixel"""
    prim = ren.Buffer("primary").cpu().numpy().reshape(H, lw, 4)
    info = ren.Buffer("info").cpu().numpy().reshape(H, lw)
    want_info = o["info"][:, sel]
    assert np.array_equal(info, want_info), what
    assert np.array_equal(prim.view(np.uint32), np.ascontiguousarray(o["primary"][:, sel]).view(np.uint32)), what
    q = ren.Buffer("infer_input").cpu().numpy().reshape(lw, H, 5)
    assert same_bits(q, o["infer_input"].reshape(W, H, 5)[sel]), what
    lst = ren.Buffer("live").cpu().numpy().view(np.uint32)
    ys, xs = np.nonzero(want_info == 1)
    want = ((ys >> 3) * ((lw + 7) >> 3) + (xs >> 3)) * 64 + (ys & 7) * 8 + (xs & 7)
    assert sorted(lst[1:1 + len(want)].tolist()) == sorted(want.tolist()), what      # (the count word is cleared by the frame's compositing)


def _render_counted(ren, frame_random):
    """one frame of the counting kernels: (CutFetches(), CountFetches())"""
    ren.CountFetches(True)
    ren.SetFrameRandom(frame_random)
    ren.Render(None, False)
    cut = ren.CutFetches()
    return cut, ren.CountFetches(False)


@pytest.mark.parametrize("medium,view,frame_name", CASES)
def test_frames_bounds_and_counters(api, orc, torch_gpu, medium, view, frame_name):
    vol = fc.volume(medium)
    size = fc.size_of(vol)
    W, H, tile, lw = fc.frame(frame_name)
    sel = _columns(W, tile)
    cam = fc.view(view, vol, W / H)
    scene = fc.make_scene(vol)
    fr = fc.FRAME_RANDOM
    o = orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, fr, threads=8)
    ref_mc, _, _ = orc.mc_render(scene, cam, W, H, 3, fr, threads=8)

    # ---- the product kernels (they cut), then the counting kernels (they walk whole and count): the same frame, the oracle's
    nrc, ren = _nrc_renderer(api, scene, cam, lw, H, tile)
    ren.SetFrameRandom(fr)
    ren.Render(None, False)
    _frame_is_the_oracles(ren, o, W, H, lw, sel, "product kernel")
    cut, _ = _render_counted(ren, fr)
    _frame_is_the_oracles(ren, o, W, H, lw, sel, "counting kernel")
    mask_words = ren.TileMask()
    far_a = ren.TileFar()
    print("%s %s %s: cut fetches %d, of them with density %d" % (medium, view, frame_name, cut[0], cut[1]))
    assert cut[1] == 0

    # ---- the bound, from both builds
    nrc_b, ren_b = _nrc_renderer(api, scene, cam, lw, H, tile)
    ren_b.RenderPath([cam], 1, np.asarray([fr], np.float32), out=False)
    assert np.array_equal(ren_b.TileMask(), mask_words)
    far_b = ren_b.TileFar()
    assert far_a.size == far_b.size and np.array_equal(far_a.view(np.uint32), far_b.view(np.uint32))
    _frame_is_the_oracles(ren_b, o, W, H, lw, sel, "tile-parallel build")
    if view == "head-on":
        assert mask_words.size > 0 and mask_words[-1] == 0        # the mask is in force: the case means something
    if mask_words.size > 0 and mask_words[-1] == 0:
        ty, tx = ref.tiles_of(lw, H)
        assert far_a.size == ty * tx
        last = fc.last_density(medium, view, frame_name)
        bad = far.violations(far_a.reshape(ty, tx), last, lw, H)
        assert bad == [], (bad[:8], len(bad))
        mask, _, _ = ref.unpack_mask(mask_words, lw, H)
        assert not ((far_a.reshape(ty, tx) > 0) & ~mask).any()    # a bound only where a box is seen (not everywhere: a box is bounded piece by piece)
    else:
        assert cut[0] == 0
    if medium in ("sphere", "blobs") and view == "head-on":
        assert cut[0] > 0                                         # empty space behind the medium: the cut is not vacuous
    if medium == "slab" and view == "head-on":
        assert cut[0] == 0                                        # the medium touches the far face: the cut is the exit point

    # ---- without the skip: the same frames, no cut, and the algorithm's look-ups
    ren.SetEmptySkip(False)
    ren.SetFrameRandom(fr)
    ren.Render(None, False)
    _frame_is_the_oracles(ren, o, W, H, lw, sel, "no skip")
    cut_off, n_fetch = _render_counted(ren, fr)
    assert cut_off == (0, 0)
    if tile is None:
        assert n_fetch == o["n_fetch"]

    # ---- the Monte-Carlo renderer, PATH_LENGTH 3
    mc = api.McHpmRenderer(lw, H, 3, False, cam, scene, tile=tile)
    mc.SetFrameRandom(fr)
    mc.Render()
    assert same_bits(mc.GetImage().cpu().numpy(), ref_mc[:, sel])
    far_mc = mc.TileFar()
    assert np.array_equal(far_mc.view(np.uint32), far_a.view(np.uint32))
    mc.SetEmptySkip(False)                                        # no mask, no capped-state selection, no cut
    mc.SetFrameRandom(fr)
    mc.Render()
    assert same_bits(mc.GetImage().cpu().numpy(), ref_mc[:, sel]) and mc.TileFar().size == 0
    mc.Destroy()
    for r, n in ((ren, nrc), (ren_b, nrc_b)):
        r.Destroy()
        n.Destroy()


@pytest.mark.parametrize("medium", ["sphere", "blobs"])
def test_a_pixel_in_a_capped_state_in_a_tile_the_cut_applies_to(api, orc, torch_gpu, medium):
    """pixel (31, 33) of the 64x64 head-on frame looks at the medium; pinned into the RNG's fixed point its walk never moves and ends at
    the 128-collision cap: its tile's wave must walk whole (a cut walk would leave instead)"""
    W = H = 64
    px, py = 31, 33
    vol = fc.volume(medium)
    cam = fc.view("head-on", vol, 1.0)
    scene = fc.make_scene(vol)
    fr = rng_search.frame_random_for_state0(px, py, W, H)
    assert fr is not None and float(rng_search.init_random(px, py, W, H, fr)) == 0.0
    o = orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, fr, threads=8)
    assert o["info"][py, px] == 1.0
    nrc, ren = _nrc_renderer(api, scene, cam, W, H, None)
    ren.SetFrameRandom(fr)
    ren.Render(None, False)
    _frame_is_the_oracles(ren, o, W, H, W, slice(None), "product kernel")
    ty, tx = ref.tiles_of(W, H)
    assert ren.TileFar().reshape(ty, tx)[py >> 3, px >> 3] > 0       # a tile the cut would apply to
    cut, _ = _render_counted(ren, fr)
    assert cut[0] > 0 and cut[1] == 0                                # ... and it still applies to the other tiles
    mc = api.McHpmRenderer(W, H, 3, False, cam, scene)
    mc.SetFrameRandom(fr)
    mc.Render()
    ref_mc, _, _ = orc.mc_render(scene, cam, W, H, 3, fr, threads=8)
    assert same_bits(mc.GetImage().cpu().numpy(), ref_mc)
    mc.Destroy()
    ren.Destroy()
    nrc.Destroy()
