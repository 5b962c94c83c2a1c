"""Hot tiles from the host (csrc/nrc_hot_tiles.hpp): the list of tiles with a pixel in a capped RNG state is computed when the frame is
enqueued and travels in the camera kernel's arguments -- no pre-pass on the render stream, whichever way the frame's random numbers
arrive.  Every case renders the pinned state-0 frame of a 256x144 view of the cloud (pixel (2, 3) starts in the RNG's fixed point) and
checks three things: the frame's outputs are bit-identical with the feature off, the affected tile rows are the oracle's bit for bit, and
HotTiles() is what a scan of every pixel with the numpy restatement of the RNG (tests/rng_search.py) finds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rng_search  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 256, 144
ROWS = (0, 8)             # the tile row of pixel (2, 3)
FRAME_RANDOM = [0.25, 0.5, 0.75, 1.0]
STATE0_FRAME_RANDOM = [0.7795426845550537, 0.04615384712815285, 0.75, 0.125]      # tests/rng_search.py 256 144 2 3
CFG = dict(train_batch_count=1, log2_train_batch_size=8, log2_infer_batch_size=14, seed=77)
KEYS = ("primary", "info", "infer_input")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def global_columns(lw, tile):
    """global column of every local column (nrc_tile: strips of x_block columns, every x_stride-th strip)"""
    lx = np.arange(lw)
    if tile is None:
        return lx
    off, stride, _, _, block = tile
    return (off + (lx // block) * stride) * block + lx % block


def scan(frame_random, lw=W, tile=None):
    """(tiles [(tx, ty), ...] one per pixel in state 0 in pixel order, the first eight; their count): every pixel of the frame visited"""
    gx, y = np.meshgrid(global_columns(lw, tile), np.arange(H))
    state = rng_search.init_random(gx.astype(np.float32), y.astype(np.float32), W, H, frame_random)
    ys, xs = np.nonzero(state == 0.0)      # row-major: ascending y * lw + lx
    return [(int(x) // 8, int(yy) // 8) for x, yy in zip(xs, ys)][:8], int(xs.size)


@pytest.fixture(scope="module")
def world(sc, cloud16):
    scene = sc.make_scene(cloud16, scene_id=4, env=sc.procedural_sky(32, 16))
    # (from both eyes the ray of pixel (2, 3) crosses the box through empty space: the tile is one the mask rejects)
    cams = [sc.make_camera(aspect=W / H), sc.make_camera(pos=(60.0, 5.0, 3.0), aspect=W / H)]
    return scene, cams


@pytest.fixture(scope="module")
def oracle_rows(orc, world):
    """the oracle's gen_rays outputs of the state-0 frame's first tile row, per view (computed once)"""
    scene, cams = world
    return [orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, STATE0_FRAME_RANDOM, rows=ROWS, threads=8) for cam in cams]


def test_the_scan_finds_the_pinned_pixel():
    assert scan(STATE0_FRAME_RANDOM) == ([(0, 0)], 1)
    assert scan(FRAME_RANDOM) == ([], 0)


def check_against_oracle(bufs, o, lw=W, tile=None):
    cols = global_columns(lw, tile)
    prim, info = bufs[0].reshape(H, lw, 4), bufs[1].reshape(H, lw)
    assert same_bits(prim[ROWS[0]:ROWS[1]], o["primary"][ROWS[0]:ROWS[1], cols])
    assert same_bits(info[ROWS[0]:ROWS[1]], o["info"][ROWS[0]:ROWS[1], cols])
    assert info[3, 2] == 1.0 and info[:8, :8].sum() == 1.0      # the capped pixel "scatters" at its entry point, alone in its tile


def run_nrc(api, world, drive, tile=None, lw=W):
    """drive(renderer) with the feature on and off -> the two (buffers, image, HotTiles()) of the last frame"""
    scene, cams = world
    out = {}
    for on in (True, False):
        cfg = api.AppConfig(**CFG)
        nrc = api.NeuralRadianceCache(cfg)
        ren = api.NrcHpmRenderer(lw, H, True, cams[0], cfg, scene, nrc, tile=tile)
        ren.SetHotTiles(on)
        drive(ren)
        out[on] = ([ren.Buffer(k).cpu().numpy().copy() for k in KEYS], ren.GetImage().cpu().numpy().copy(), ren.HotTiles())
        ren.Destroy()
        nrc.Destroy()
    for a, b in zip(out[True][0], out[False][0]):
        assert same_bits(a, b)
    assert same_bits(out[True][1], out[False][1])
    assert out[False][2] is None
    return out[True]


def test_a_pinned_frame_rendered_alone(api, world, oracle_rows, torch_gpu):
    def drive(ren):
        ren.SetFrameRandom(STATE0_FRAME_RANDOM)
        ren.Render(None, True)
    bufs, _, hot = run_nrc(api, world, drive)
    check_against_oracle(bufs, oracle_rows[0])
    assert hot == (*scan(STATE0_FRAME_RANDOM), False)


def test_the_first_frame_of_a_call_whose_predecessor_ended_on_other_numbers(api, sc, world, oracle_rows, torch_gpu):
    """the benchmark's pattern: the last frame of a RenderFrames call has no successor announced and draws numbers ahead; the next call
    pins others"""
    def drive(ren):
        ren.RenderFrames(np.asarray(sc.frame_randoms(4, seed=5), np.float32), True)
        ren.RenderFrames(np.array([STATE0_FRAME_RANDOM], np.float32), True)
    bufs, _, hot = run_nrc(api, world, drive)
    check_against_oracle(bufs, oracle_rows[0])
    assert hot == (*scan(STATE0_FRAME_RANDOM), False)


def test_the_first_frame_of_a_view_of_a_camera_path(api, world, oracle_rows, torch_gpu):
    scene, cams = world

    def drive(ren):
        ren.RenderPath(cams, 1, np.array([FRAME_RANDOM, STATE0_FRAME_RANDOM], np.float32), train=False, out=False)
    bufs, _, hot = run_nrc(api, world, drive)
    check_against_oracle(bufs, oracle_rows[1])
    assert hot == (*scan(STATE0_FRAME_RANDOM), False)


def test_the_monte_carlo_renderer(api, orc, world, torch_gpu):
    """McHpmRenderer has no switch for the list and no accessor: the frames without it are those with the empty-space mask off (no mask,
    nothing promoted; the mask is exact, so this changes no pixel either).  Two blended frames, the second the state-0 frame: a tile traced
    twice would be blended twice, a tile never traced would keep the first frame.  NOT covered: the list's content -- a wrong tile in it
    that is still traced exactly once passes; the list comes from the function the NRC renderer uses, whose list the other cases check."""
    scene, cams = world
    img = {}
    for skip in (True, False):
        mc = api.McHpmRenderer(W, H, 8, True, cams[0], scene)
        mc.SetEmptySkip(skip)
        for fr in (FRAME_RANDOM, STATE0_FRAME_RANDOM):
            mc.SetFrameRandom(fr)
            mc.Render()
        img[skip] = mc.GetImage().cpu().numpy().copy()
        mc.Destroy()
    assert same_bits(img[True], img[False])
    ref = np.zeros((H, W, 4), np.float32)
    for k, fr in enumerate((FRAME_RANDOM, STATE0_FRAME_RANDOM)):
        orc.mc_render(scene, cams[0], W, H, 8, fr, blend=1.0 / (k + 1), out=ref, rows=ROWS, threads=8)
    assert same_bits(img[True][ROWS[0]:ROWS[1]], ref[ROWS[0]:ROWS[1]])


def test_a_column_tiled_renderer(api, world, oracle_rows, torch_gpu):
    """rank 0 of a world of 2 (strips of 8 columns) owns global column 2; rank 1 has no capped pixel in this frame"""
    from nrc_hpm_renderer_amd import parallel
    for rank, want in ((0, ([(0, 0)], 1)), (1, ([], 0))):
        tile = (rank, 2, W, H, 8)
        lw = parallel.local_width(rank, 2, W, 8)

        def drive(ren):
            ren.SetFrameRandom(STATE0_FRAME_RANDOM)
            ren.Render(None, False)
        bufs, _, hot = run_nrc(api, world, drive, tile=tile, lw=lw)
        assert scan(STATE0_FRAME_RANDOM, lw, tile) == want
        assert hot == (*want, False)
        cols = global_columns(lw, tile)
        o = oracle_rows[0]
        assert same_bits(bufs[0].reshape(H, lw, 4)[ROWS[0]:ROWS[1]], o["primary"][ROWS[0]:ROWS[1], cols])
        assert same_bits(bufs[1].reshape(H, lw)[ROWS[0]:ROWS[1]], o["info"][ROWS[0]:ROWS[1], cols])
        if rank == 0:
            assert bufs[1].reshape(H, lw)[3, 2] == 1.0
