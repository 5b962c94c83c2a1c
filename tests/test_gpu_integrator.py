"""Parity of the HIP path integrator and of whole NRC frames against the oracle, through the C ABI.
Tolerance: >= 99.5 % of pixels within 1e-5 abs and frame relative-L2 <= 1e-3 (the math spec is shared
bit-for-bit, so in practice the frames are identical)."""
import os

import numpy as np
import pytest

import image_reference as ir
from conftest import FRAME_RANDOM, GOLDEN, nrc_debug

pytestmark = pytest.mark.gpu


def frac_close(a, b, atol=1e-5):
    ok = np.isclose(a, b, atol=atol, rtol=1e-5, equal_nan=True)
    return ok.reshape(ok.shape[0], -1).all(axis=1).mean() if a.ndim > 1 else ok.mean()


def same_bits(a, b):
    """bit-identical (a NaN matches a NaN): the integrator's results are a pure function of the specified fp32 arithmetic"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def lin(img_hw, W, H):
    """[H][W][c] image -> the NRC buffers' x*H+y order"""
    return np.ascontiguousarray(img_hw.transpose(1, 0, 2)).reshape(W * H, -1)


@pytest.mark.parametrize("case", ["sphere64", "cloud16_scene0", "cloud16_scene4_sky", "cloud16_scene1_point"])
def test_mc_frame_matches_oracle(api, orc, sc, cloud16, sphere_scene, torch_gpu, case):
    if case == "sphere64":
        scene, W, H, cam = sphere_scene, 64, 64, sc.make_camera(aspect=1.0)
    else:
        sid = {"cloud16_scene0": 0, "cloud16_scene4_sky": 4, "cloud16_scene1_point": 1}[case]
        env = sc.procedural_sky(64, 32) if "sky" in case else None
        scene, W, H, cam = sc.make_scene(cloud16, scene_id=sid, env=env), 96, 54, sc.make_camera(aspect=96 / 54)
    mc = api.McHpmRenderer(W, H, 32, False, cam, scene)
    mc.SetFrameRandom(FRAME_RANDOM)
    mc.Render()
    img = mc.GetImage().cpu().numpy()
    ref, _, _ = orc.mc_render(scene, cam, W, H, 32, FRAME_RANDOM, threads=8)
    assert np.isfinite(img).all()
    assert same_bits(img, ref)                      # stated bar: >= 99.5 % of pixels within 1e-5, rel-L2 <= 1e-3
    assert mc.GetFrameTimeMS() > 0
    mc.Destroy()


def test_scene_parameter_update_matches_oracle(api, orc, sc, cloud16, torch_gpu):
    """HpmScene::Update / the light editors: new light + medium constants take effect with the next Render (textures stay) --
    MC and NRC renderers against the oracle rendered with the updated scene"""
    W, H = 96, 54
    cam = sc.make_camera(aspect=W / H)
    hs = sc.HpmScene(cloud16, scene_id=3, dynamic=True)
    mc = api.McHpmRenderer(W, H, 32, False, cam, hs.scene)
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=10, log2_infer_batch_size=14, scene_id=3)
    nrc = api.NeuralRadianceCache(cfg)
    ren = api.NrcHpmRenderer(W, H, False, cam, cfg, hs.scene, nrc)
    for step in range(2):
        if step == 1:
            assert hs.Update(1.5)                      # azimuth 0.75 rad
            hs.scene["density_factor"] = 0.5           # VolumeData editor
            hs.scene["point_light_strength"] = 2.0     # PointLight editor
            mc.SetSceneParams(hs)
            ren.SetSceneParams(hs)
        mc.SetFrameRandom(FRAME_RANDOM)
        mc.Render()
        ref, _, _ = orc.mc_render(hs.scene, cam, W, H, 32, FRAME_RANDOM, threads=8)
        img = mc.GetImage().cpu().numpy()
        assert same_bits(img, ref)
        ren.SetFrameRandom(FRAME_RANDOM)
        ren.Render(None, False)
        o = orc.nrc_gen_rays(hs.scene, cam, W, H, 1, 0.0, FRAME_RANDOM, threads=8)
        prim = ren.Buffer("primary").cpu().numpy().reshape(H, W, 4)
        assert same_bits(prim, o["primary"])
        if step == 0:
            first = img.copy()
    assert rel(img, first) > 0.05                      # the update changed the picture
    mc.Destroy()
    ren.Destroy()
    nrc.Destroy()


CASES = {
    "camera-inside-volume": dict(cam=dict(pos=(5.0, 2.0, -3.0), view_dir=(-0.7, 0.1, 0.7)), scene_id=4),
    "camera-looking-away": dict(cam=dict(pos=(64.0, 0.0, 0.0), view_dir=(1.0, 0.0, 0.0)), scene_id=4),
    "oblique-camera": dict(cam=dict(pos=(40.0, 35.0, -50.0), view_dir=(-0.6, -0.5, 0.7)), scene_id=0),
    "empty-volume": dict(volume="zeros", scene_id=4),
    "solid-volume": dict(volume="full", scene_id=4),
    "point-light-scene2": dict(scene_id=2),
    "env-only-scene5-sky": dict(scene_id=5, sky=True),
    "thin-medium": dict(scene_id=4, density_factor=0.01),
    "anisotropy-0": dict(scene_id=4, g=0.0),          # NewRayDir's isotropic branch (|g| < 0.001)
    "back-scatter": dict(scene_id=0, g=-0.6),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_unusual_scenes_and_cameras_match_oracle_bitwise(api, orc, sc, cloud16, torch_gpu, case):
    """both renderers on scenes off the beaten path -- camera inside / beside / facing away from the volume, empty and solid
    volumes, every light type alone, isotropic and back-scattering phase functions, a very thin medium"""
    k = CASES[case]
    W, H = 72, 48
    vol = cloud16
    if k.get("volume") == "zeros":
        vol = np.zeros((12, 10, 14), np.uint8)
    elif k.get("volume") == "full":
        vol = np.full((12, 10, 14), 255, np.uint8)
    env = sc.procedural_sky(32, 16) if k.get("sky") else None
    scene = sc.make_scene(vol, scene_id=k["scene_id"], env=env, g=k.get("g", 0.8))
    if "density_factor" in k:
        scene["density_factor"] = k["density_factor"]
    cam = sc.make_camera(aspect=W / H, **k.get("cam", {}))
    mc = api.McHpmRenderer(W, H, 16, False, cam, scene)
    mc.SetFrameRandom(FRAME_RANDOM)
    mc.Render()
    ref, ref_info, _ = orc.mc_render(scene, cam, W, H, 16, FRAME_RANDOM, threads=8)
    img = mc.GetImage().cpu().numpy()
    assert same_bits(img, ref)
    mc.Destroy()
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=8, log2_infer_batch_size=12, scene_id=k["scene_id"])
    nrc = api.NeuralRadianceCache(cfg)
    ren = api.NrcHpmRenderer(W, H, False, cam, cfg, scene, nrc)
    ren.SetFrameRandom(FRAME_RANDOM)
    ren.Render(None, True)
    o = orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, FRAME_RANDOM, threads=8)
    assert same_bits(ren.Buffer("primary").cpu().numpy().reshape(H, W, 4), o["primary"])
    assert same_bits(ren.Buffer("info").cpu().numpy().reshape(H, W), o["info"])
    assert same_bits(ren.Buffer("infer_input").cpu().numpy(), o["infer_input"])
    assert np.isfinite(ren.GetImage().cpu().numpy()).all() and np.isfinite(nrc.GetLoss())
    if case == "empty-volume":
        assert o["info"].sum() == 0
    if case == "solid-volume":
        assert o["info"].mean() > 0.2
    ren.Destroy()
    nrc.Destroy()


# pixel (2, 3) of a 256x144 frame starts in RNG state 0 with this frame random (tests/rng_search.py): all its draws are 0, its delta
# walk never moves and ends in DeltaTrack's 128-collision cap -- it "scatters" at the entry point although its tile sees no density
STATE0_FRAME_RANDOM = [0.7795426845550537, 0.04615384712815285, 0.75, 0.125]


@pytest.mark.parametrize("view", ["default", "oblique", "inside", "tile-3-of-8", "state0-pixel", "density-0.9", "density-1.6-scene5", "empty-volume-1.6"])
def test_empty_space_early_out_is_exact(api, orc, sc, cloud16, torch_gpu, view):
    """the tile mask that lets camera rays skip a walk through provably empty space: frames with and without it are bit-identical
    (NRC primary pass, query buffer, MC image), the oracle -- which walks every ray -- agrees with both, and the mask really
    removes work (fewer density look-ups executed) wherever part of the view is empty.  A walk through empty space can also end
    in DeltaTrack's cap of 128 collisions (path_trace.glsl:161-173) and scatter there: a pixel forced into the RNG's fixed point
    does so on any scene, and with a dense medium (optical depth of the box diagonal 97 / 172) ordinary pixels do"""
    from nrc_hpm_renderer_amd import parallel
    W, H = 256, 144
    cam_kw = {"oblique": dict(pos=(40.0, 35.0, -50.0), view_dir=(-0.6, -0.5, 0.7)),
              "inside": dict(pos=(5.0, 2.0, -3.0), view_dir=(-0.7, 0.1, 0.7))}.get(view, {})
    vol = np.zeros_like(cloud16) if view == "empty-volume-1.6" else cloud16
    scene = sc.make_scene(vol, scene_id=5 if "1.6" in view else 4, env=sc.procedural_sky(32, 16))
    if view == "density-0.9":
        scene["density_factor"] = 0.9
    frame_random = STATE0_FRAME_RANDOM if view == "state0-pixel" else FRAME_RANDOM
    cam = sc.make_camera(aspect=W / H, **cam_kw)
    tile, lw = None, W
    if view == "tile-3-of-8":
        tile, lw = parallel.column_tile(3, 8, W, H), parallel.local_width(3, 8, W)
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=8, log2_infer_batch_size=14)
    out = {}
    for skip in (True, False):
        nrc = api.NeuralRadianceCache(cfg)
        ren = api.NrcHpmRenderer(lw, H, False, cam, cfg, scene, nrc, tile=tile)
        ren.SetEmptySkip(skip)
        ren.CountFetches(True)
        ren.SetFrameRandom(frame_random)
        ren.Render(None, False)
        n_fetch = ren.CountFetches(False)
        mc = api.McHpmRenderer(lw, H, 8, False, cam, scene, tile=tile)
        mc.SetEmptySkip(skip)
        mc.SetFrameRandom(frame_random)
        mc.Render()
        out[skip] = (ren.Buffer("primary").cpu().numpy().copy(), ren.Buffer("info").cpu().numpy().copy(),
                     ren.Buffer("infer_input").cpu().numpy().copy(), mc.GetImage().cpu().numpy().copy(), n_fetch)
        mc.Destroy()
        ren.Destroy()
        nrc.Destroy()
    for k in range(4):
        assert same_bits(out[True][k], out[False][k])
    o = orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, frame_random, threads=8)
    sel = parallel.rank_columns(3, 8, W) if tile else slice(None)
    assert same_bits(out[True][0].reshape(H, lw, 4), o["primary"][:, sel]) and same_bits(out[True][1].reshape(H, lw), o["info"][:, sel])
    assert same_bits(out[True][2].reshape(lw, H, 5), o["infer_input"].reshape(W, H, 5)[sel])
    ref_mc, _, _ = orc.mc_render(scene, cam, W, H, 8, frame_random, threads=8)
    assert same_bits(out[True][3], ref_mc[:, sel])
    if tile is None:
        assert out[False][4] == o["n_fetch"]                      # without the mask the device executes the algorithm's look-ups
    assert out[True][4] <= out[False][4]
    if view in ("default", "tile-3-of-8", "oblique", "state0-pixel", "density-0.9"):
        assert out[True][4] < out[False][4]                        # part of these views is provably empty space
    if view == "state0-pixel":                                     # the case bites: the pixel scatters where no density is
        assert o["info"][3, 2] == 1.0 and o["info"][3, 3] == 0.0 and o["info"][2, 2] == 0.0
    if "1.6" in view:                                              # nearly every RNG state can reach the cap: the mask is not applied
        assert out[True][4] == out[False][4]
    if view == "empty-volume-1.6":                                 # ... and some walks through the empty box do (71 of this frame's)
        assert o["info"].sum() > 20


def test_renderer_argument_errors(api, sc, sphere_scene, torch_gpu):
    """Log::Error semantics at the boundary: a message starting with "SkyRenderer ERROR", no crash, nothing left half-built"""
    cam = sc.make_camera(aspect=1.0)
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=8, log2_infer_batch_size=12)
    nrc = api.NeuralRadianceCache(cfg)
    with pytest.raises(RuntimeError, match="SkyRenderer ERROR.*multiple of 16"):
        api.NrcHpmRenderer(10, 10, False, cam, cfg, sphere_scene, nrc)
    with pytest.raises(RuntimeError, match="SkyRenderer ERROR"):
        api.NrcHpmRenderer(0, 16, False, cam, cfg, sphere_scene, nrc)
    bad = dict(sphere_scene, density_factor=0.0)
    with pytest.raises(RuntimeError, match="SkyRenderer ERROR.*density"):
        api.McHpmRenderer(16, 16, 4, False, cam, bad)
    ren = api.NrcHpmRenderer(16, 16, False, cam, cfg, sphere_scene, nrc)     # the cache is still usable afterwards
    ren.Render(None, True)
    assert np.isfinite(nrc.GetLoss())
    ren.Destroy()
    nrc.Destroy()


def test_mc_progressive_blend(api, orc, sc, sphere_scene, torch_gpu):
    """blendFactor = 1/blendIndex, index advances only when blending (src/McHpmRenderer.cpp:124-136)"""
    W = H = 48
    cam = sc.make_camera(aspect=1.0)
    mc = api.McHpmRenderer(W, H, 8, True, cam, sphere_scene)
    ref = np.zeros((H, W, 4), np.float32)
    frs = sc.frame_randoms(3, seed=5)
    for i in range(3):
        mc.SetFrameRandom(frs[i])
        mc.Render()
        ref, _, _ = orc.mc_render(sphere_scene, cam, W, H, 8, frs[i], blend=1.0 / (i + 1), out=ref, threads=8)
    assert same_bits(mc.GetImage().cpu().numpy(), ref)
    mc.SetBlend(False)
    mc.SetFrameRandom(frs[0])
    mc.Render()
    one, _, _ = orc.mc_render(sphere_scene, cam, W, H, 8, frs[0], threads=8)
    assert same_bits(mc.GetImage().cpu().numpy(), one)
    mc.Destroy()


def _nrc_setup(api, sc, scene, W, H, **cfg_kw):
    kw = dict(train_batch_count=1, log2_train_batch_size=10, log2_infer_batch_size=14)
    kw.update(cfg_kw)
    cfg = api.AppConfig(**kw)
    nrc = api.NeuralRadianceCache(cfg)
    cam = sc.make_camera(aspect=W / H)
    ren = api.NrcHpmRenderer(W, H, False, cam, cfg, scene, nrc)
    return cfg, nrc, cam, ren


@pytest.mark.parametrize("W,H", [(128, 80), (100, 52), (8, 6)], ids=["128x80", "ragged100x52", "tiny8x6"])
def test_gen_rays_and_query_packing_match_oracle(api, orc, sc, cloud16, torch_gpu, W, H):
    """nrc/gen_rays.comp + prep_infer_rays.comp: primary colour/throughput, didScatter, NRC vertex, packed queries; also on
    frames whose width / height are not multiples of the 8x8 wave tile (partial tiles, odd tile-row counts)"""
    scene = sc.make_scene(cloud16, scene_id=4)
    cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H)
    o = orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, FRAME_RANDOM, threads=8)
    # default: the NRC vertex images are stored at the train grid's pixels only (their one reader, prep_train_rays)
    ren.SetFrameRandom(FRAME_RANDOM)
    ren.Render(None, False)
    tg = ren.TrainGrid()
    assert ren.VertexImageBytes() == tg["tw"] * tg["th"] * 32
    gy, gx = np.meshgrid(np.arange(tg["th"]) * tg["y_dist"], np.arange(tg["tw"]) * tg["x_dist"], indexing="ij")
    ok = (gy < H) & (gx < W)
    gy, gx = gy[ok], gx[ok]
    on = o["info"][gy, gx] == 1
    org_s = ren.Buffer("origin").cpu().numpy().reshape(H, W, 4)
    dir_s = ren.Buffer("dir").cpu().numpy().reshape(H, W, 4)
    assert same_bits(org_s[gy[on], gx[on]], o["origin"][gy[on], gx[on]]) and same_bits(dir_s[gy[on], gx[on]], o["dir"][gy[on], gx[on]])
    off_grid = np.ones((H, W), bool)
    off_grid[gy, gx] = False
    assert (org_s[off_grid] == 0).all() and (dir_s[off_grid] == 0).all()      # nothing stored elsewhere (zero-initialised images)
    ren.Destroy()
    nrc.Destroy()
    cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H)
    ren.SetFullVertexImages(True)                   # the reference's whole images
    assert ren.VertexImageBytes() == W * H * 32
    ren.SetFrameRandom(FRAME_RANDOM)
    ren.Render(None, False)
    prim = ren.Buffer("primary").cpu().numpy().reshape(H, W, 4)
    info = ren.Buffer("info").cpu().numpy().reshape(H, W)
    big = W * H >= 4096
    assert np.array_equal(info, o["info"]) and (not big or 0.1 < info.mean() < 0.9)
    assert np.array_equal(prim.view(np.uint32), o["primary"].view(np.uint32))        # bit-identical, every pixel
    m = info.reshape(-1) == 1
    org = ren.Buffer("origin").cpu().numpy()
    dr = ren.Buffer("dir").cpu().numpy()
    assert same_bits(org[m], o["origin"].reshape(-1, 4)[m]) and same_bits(dr[m], o["dir"].reshape(-1, 4)[m])
    q = ren.Buffer("infer_input").cpu().numpy()
    assert same_bits(q, o["infer_input"])                   # NaN phi (quirk Q5) included
    assert not big or np.isnan(q[:, 4]).any()               # the quirk is reproduced
    assert (q[lin(info[..., None], W, H)[:, 0] == 0] == 0).all()     # unscattered slots are zero (vkCmdFillBuffer)
    # throughput: 0.25 after two vertices, 0.5 if the second segment left the volume
    thr = prim[..., 3][info == 1]
    assert set(np.unique(thr)).issubset({0.25, 0.5})
    ren.Destroy()
    nrc.Destroy()


@pytest.mark.parametrize("length,prob", [(3, 0.6), (0, 0.0), (2, 1.0)], ids=["len3-p0.6", "len0", "len2-p1(128-vertex cap)"])
def test_gen_rays_primary_path_length_and_probability(api, orc, sc, cloud16, torch_gpu, length, prob):
    """PRIMARY_RAY_LENGTH / PRIMARY_RAY_PROB (arguments 15/16 of the command line; gen_rays.comp:39-42): longer primary paths with
    Russian-roulette-like continuation, down to the 128-vertex cap when the probability is 1"""
    W, H = 96, 64
    scene = sc.make_scene(cloud16, scene_id=4)
    cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H, primary_ray_length=length, primary_ray_prob=prob)
    ren.SetFrameRandom(FRAME_RANDOM)
    ren.Render(None, False)
    o = orc.nrc_gen_rays(scene, cam, W, H, length, prob, FRAME_RANDOM, threads=8)
    assert same_bits(ren.Buffer("primary").cpu().numpy().reshape(H, W, 4), o["primary"])
    assert same_bits(ren.Buffer("info").cpu().numpy().reshape(H, W), o["info"])
    assert same_bits(ren.Buffer("infer_input").cpu().numpy(), o["infer_input"])
    thr = o["primary"][..., 3][o["info"] == 1]
    assert thr.min() < (0.5 if length == 0 else 0.25) or prob == 0.0
    ren.Destroy()
    nrc.Destroy()


@pytest.mark.parametrize("fix_q1", [0, 1])
def test_prep_train_and_ring_buffer_match_oracle(api, orc, sc, cloud16, torch_gpu, fix_q1):
    """nrc/clear.comp + prep_train_rays.comp over two frames: train inputs/targets and the ring buffer state"""
    W, H = 128, 80
    scene = sc.make_scene(cloud16, scene_id=0)
    cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H, compat_fix=fix_q1)
    tg = ren.TrainGrid()
    assert tg["tw"] * tg["th"] == 1024 and tg["tw"] >= tg["th"]         # CalcTrainSubset: bigger factor on the wide axis
    assert tg["x_dist"] == W // tg["tw"]
    assert tg["y_dist"] == (H // tg["th"] if fix_q1 else tg["x_dist"])   # quirk Q1
    T = tg["tw"] * tg["th"]
    head_tail = np.zeros(2, np.uint32)
    ring = np.zeros((T, 6), np.float32)
    ring[:, 5] = 1.0                                                     # CreateNrcTrainRingBuffer init
    frs = sc.frame_randoms(2, seed=3)
    for f in range(2):
        ren.SetFrameRandom(frs[f])
        ren.Render(None, False)
        o = orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, frs[f], threads=8)
        tin, tgt = orc.nrc_prep_train(scene, W, H, tg["tw"], tg["th"], tg["x_dist"], tg["y_dist"], 1, 1, tg["ring_size"],
                                      frs[f], o["info"], o["origin"], o["dir"], head_tail, ring, threads=8)
        g_in = ren.Buffer("train_input").cpu().numpy()
        g_t = ren.Buffer("train_target").cpu().numpy()
        assert same_bits(g_in, tin) and same_bits(g_t, tgt)
        assert (g_t <= 8.0).all()
        rb = ren.Buffer("ring").cpu().numpy()
        assert rb[0].view(np.uint32) == head_tail[0] and rb[1].view(np.uint32) == head_tail[1]
        assert same_bits(rb[2:].view(np.float32).reshape(-1, 6)[:T], ring)
    assert head_tail[0] > 0 and head_tail[1] > 0
    ren.Destroy()
    nrc.Destroy()


def test_prep_train_spp_ray_length_and_small_ring(api, orc, sc, cloud16, torch_gpu):
    """TRAIN_SPP 3, TRAIN_RAY_LENGTH 4 (reachable with the quirk-Q2 fix), a ring buffer a quarter of the train grid (wraps within
    a frame) over three frames: train rays and ring state bit-identical to the oracle"""
    W, H = 128, 80
    scene = sc.make_scene(cloud16, scene_id=4, env=sc.procedural_sky(64, 32))
    cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H, compat_fix=3, train_spp=3, train_ray_length=4, train_ring_buf_size=0.25)
    tg = ren.TrainGrid()
    T = tg["tw"] * tg["th"]
    assert tg["ring_size"] == T // 4
    head_tail = np.zeros(2, np.uint32)
    ring = np.zeros((T, 6), np.float32)
    ring[:, 5] = 1.0
    frs = sc.frame_randoms(3, seed=8)
    for f in range(3):
        ren.SetFrameRandom(frs[f])
        ren.Render(None, False)
        o = orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, frs[f], threads=8)
        head_before = int(head_tail[0]) % tg["ring_size"]
        tin, tgt = orc.nrc_prep_train(scene, W, H, tg["tw"], tg["th"], tg["x_dist"], tg["y_dist"], 3, 4, tg["ring_size"],
                                      frs[f], o["info"], o["origin"], o["dir"], head_tail, ring, threads=8)
        assert int(head_tail[0]) - head_before > tg["ring_size"]      # the frame pushes more than the ring holds: slots are written twice
        assert same_bits(ren.Buffer("train_input").cpu().numpy(), tin)
        assert same_bits(ren.Buffer("train_target").cpu().numpy(), tgt)
        rb = ren.Buffer("ring").cpu().numpy()
        assert rb[0].view(np.uint32) == head_tail[0] and rb[1].view(np.uint32) == head_tail[1]
        assert same_bits(rb[2:].view(np.float32).reshape(-1, 6)[:tg["ring_size"]], ring[:tg["ring_size"]])
    assert tgt.max() > 0
    ren.Destroy()
    nrc.Destroy()


@pytest.mark.parametrize("model", [(3, 0, 64, 6), (3, 0, 128, 8), (2, 0, 64, 3), (0, 0, 64, 6)])
def test_full_nrc_frame_matches_oracle_pipeline(api, orc, sc, cloud16, torch_gpu, model):
    """NrcHpmRenderer::Render(queue, true): gen_rays -> prep_train -> InferAndTrain -> render.comp, two frames with
    blending; inference always sees the previous frame's EMA weights (quirk Q13).  Models: the north-star 6x64 (fused
    kernels), BASELINE configs[4]'s 8x128, a TriangleWave/3x64 net and the reference-default HashGrid model (generic kernels)."""
    W, H = 128, 80
    scene = sc.make_scene(cloud16, scene_id=4)
    pos_id, dir_id, width, depth = model
    hg = 12 if pos_id == 0 else 0          # HashGrid (the reference's default encoding) with a small table for the oracle
    cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H, pos_id=pos_id, dir_id=dir_id, nn_width=width, nn_depth=depth,
                                    hashgrid_log2_size=hg)
    ren.SetBlend(True)
    onn = orc.nn_create(pos_id=pos_id, dir_id=dir_id, width=width, depth=depth, hashgrid_log2_size=hg)
    tg = ren.TrainGrid()
    T = tg["tw"] * tg["th"]
    head_tail = np.zeros(2, np.uint32)
    ring = np.zeros((T, 6), np.float32)
    ring[:, 5] = 1.0
    ref = np.zeros((H, W, 4), np.float32)
    frs = sc.frame_randoms(2, seed=9)
    for f in range(2):
        ren.SetFrameRandom(frs[f])
        ren.Render(None, True)
        o = orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, frs[f], threads=8)
        tin, tgt = orc.nrc_prep_train(scene, W, H, tg["tw"], tg["th"], tg["x_dist"], tg["y_dist"], 1, 1, tg["ring_size"],
                                      frs[f], o["info"], o["origin"], o["dir"], head_tail, ring, threads=8)
        y = onn.forward(o["infer_input"], use_ema=True, mode=1)
        loss_ref = onn.backward(tin, tgt)
        onn.optimizer_step()
        ref = orc.nrc_composite(W, H, 1, 1.0 / (f + 1), o["primary"], o["info"], y, ref)
        assert abs(nrc.GetLoss() - loss_ref) < 5e-3 * abs(loss_ref)
    img = ren.GetImage().cpu().numpy()
    assert np.isfinite(img).all() and (img[..., 3] == 1.0).all()
    assert rel(img[..., :3], ref[..., :3]) < 2e-3
    assert frac_close(img.reshape(-1, 4), ref.reshape(-1, 4), atol=5e-3) >= 0.995
    # Adam normalises every element to +-lr: elements whose gradient is ~0 +- fp16 noise may flip sign, hence the slack
    assert rel(nrc.GetParams(1), onn.buffer(1)) < 3e-3
    st = ren.EvaluateTimestampQueries()
    assert st["total"] > 0 and st["gen_rays"] > 0 and st["infer"] > 0 and st["train"] > 0
    # showNrc = 0 -> primary radiance only
    ren.SetBlend(False)
    ren.SetShowNrc(False)
    ren.SetFrameRandom(frs[0])
    ren.Render(None, False)
    o = orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, frs[0], threads=8)
    assert same_bits(ren.GetImage().cpu().numpy()[..., :3], o["primary"][..., :3])
    ren.Destroy()
    nrc.Destroy()


@pytest.mark.parametrize("model", [(3, 0, 64, 6, 1), (2, 2, 64, 3, 1), (3, 0, 64, 6, 4), (3, 0, 64, 6, 1, 2), (2, 2, 64, 3, 2, 3)],
                         ids=["fused", "generic", "fused-4-train-batches", "q2-fixed-long-train-paths", "generic-q1q2-fixed"])
def test_pipelined_streams_equal_single_stream_bitwise(api, sc, cloud16, torch_gpu, model, monkeypatch):
    """the four-stream frame graph (train rays, training and inference of frame N beside gen_rays of frame N+1; triple-buffered
    gen_rays outputs, double-buffered train rays and inference weights) is pure scheduling: after 8 trained, blended frames the
    framebuffer, the loss and every parameter equal the single-stream order (NRC_DEBUG=single_stream) bit for bit.  With quirk Q2 fixed
    (train paths of up to 32 vertices) the graph has six streams: the train rays' start vertices and the ring on D, the TRACES of even and
    odd frames on two streams of their own, overlapping each other (k_prep_train<1> / <2>) -- against the one-launch kernel of the
    single-stream order"""
    fix = dict(compat_fix=model[5], train_ray_length=32, train_spp=1) if len(model) > 5 else {}
    W, H = 256, 160
    scene = sc.make_scene(cloud16, scene_id=4)
    frs = sc.frame_randoms(8, seed=21)
    results = []
    for mode in ("single_stream", None, None, None, None):     # the full graph several times: races are rare
        nrc_debug(monkeypatch, single_stream=mode is not None)
        cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H, pos_id=model[0], dir_id=model[1], nn_width=model[2], nn_depth=model[3],
                                        train_batch_count=model[4], log2_train_batch_size=10 if model[4] == 1 else 8, **fix)
        ren.SetBlend(True)
        for f in range(8):
            ren.SetFrameRandom(frs[f])
            ren.Render(None, f != 5)      # no host synchronisation between frames (one frame without training: the graph's other branch)
        results.append((ren.GetImage().cpu().numpy().copy(), nrc.GetLoss(), nrc.GetParams(0).copy(), nrc.GetParams(1).copy(),
                        ren.Buffer("train_input").cpu().numpy().copy(), ren.Buffer("train_target").cpu().numpy().copy(),
                        ren.Buffer("ring").cpu().numpy().copy()))
        ren.Destroy()
        nrc.Destroy()
    base = results[0]
    for other in results[1:]:
        assert np.array_equal(base[0].view(np.uint32), other[0].view(np.uint32))
        assert base[1] == other[1]
        assert np.array_equal(base[2].view(np.uint32), other[2].view(np.uint32))
        assert np.array_equal(base[3].view(np.uint32), other[3].view(np.uint32))
        assert np.array_equal(base[4].view(np.uint32), other[4].view(np.uint32))
        assert np.array_equal(base[5].view(np.uint32), other[5].view(np.uint32)) and np.array_equal(base[6].view(np.uint32), other[6].view(np.uint32))


def test_no_value_of_the_schedule_changes_a_pixel(api, sc, cloud16, torch_gpu, monkeypatch):
    """nrc_schedule is scheduling only: camera kernels at the default wave priority under the library's other kernels or at the common one,
    two or three frames between a cost sample and the launch order made of it, the XCD-aware finish of that order off / narrow / wide,
    round 3's or round 4's training kernels (NRC_DEBUG=train_gen_old / wgrad_old) -- after 10 trained, blended frames the framebuffer, the loss
    and the parameters are the same bit for bit whichever way they are set (the weight-gradient kernels differ in their chunk sums: not
    toggled here), and a renderer left to itself reports the neutral start values"""
    W, H = 256, 160
    scene = sc.make_scene(cloud16, scene_id=4)
    frs = sc.frame_randoms(10, seed=33)
    results = []
    for sched, env in ((None, {}), (dict(camera_priority_low=1), {}), (dict(cost_order_lag=3), {}), (dict(xcd_window=0), {}),
                       (dict(xcd_window=16), {}), (dict(camera_priority_low=1, cost_order_lag=3, xcd_window=16), {}), (None, {"train_gen_old": 1})):
        nrc_debug(monkeypatch, **env)
        cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H, pos_id=3, dir_id=0, nn_width=128, nn_depth=3, train_batch_count=1,
                                        log2_train_batch_size=10)
        if sched is None:
            got = ren.GetSchedule()
            assert {k: got[k] for k in ("camera_priority_low", "cost_order_lag", "xcd_window", "composite_defer", "tuning_done", "source")} == \
                dict(camera_priority_low=0, cost_order_lag=2, xcd_window=2, composite_defer=0, tuning_done=False, source="default")
        else:
            ren.SetSchedule(**sched)
            got = ren.GetSchedule()
            assert all(got[k] == v for k, v in sched.items())
        ren.SetBlend(True)
        for f in range(10):               # the cost order is sampled at frame 0, 4, 8 and in use from frame 2 / 3 on
            ren.SetFrameRandom(frs[f])
            ren.Render(None, True)
        results.append((ren.GetImage().cpu().numpy().copy(), nrc.GetLoss(), nrc.GetParams(0).copy()))
        ren.Destroy()
        nrc.Destroy()
    nrc_debug(monkeypatch)
    base = results[0]
    assert np.isfinite(base[0]).all() and base[0].max() > 0.0
    for other in results[1:]:
        assert np.array_equal(base[0].view(np.uint32), other[0].view(np.uint32))
        assert base[1] == other[1]
        assert np.array_equal(base[2].view(np.uint32), other[2].view(np.uint32))


def test_the_renderer_chooses_its_schedule_on_live_frames_without_changing_them(api, sc, cloud16, torch_gpu):
    """the Tuner (nrc_schedule.hpp): with the pipeline kept full (render_frames, no host synchronisation) the renderer tries the alternatives of
    each knob on the caller's own frames and settles -- tuning_done -- within 370 to 900 frames (128 to warm up, ten trials of 24, replayed up to
    three times where a result is inside the noise); the frames are those of a renderer whose
    schedule is pinned, bit for bit; pinned knobs keep their values; a host that synchronises after every frame never tunes.  (1080p: the
    GPU, not the host's enqueue, must bound the frame -- a renderer whose host cannot keep the pipeline full has nothing to measure)"""
    W, H = 1920, 1080
    scene = sc.make_scene(sc.cached_volume("cloud", 256, seed=1337), scene_id=4, env=sc.procedural_sky())      # the bench scene: 0.25 ms per frame
    n_frames = 1280      # 128 to warm up + at most three rounds of 3 + 3 + 4 trials of 24 frames + the waits for their time stamps
    n_spare = 2560       # (a sequence during which the host stalled is played again: frames beyond n_frames only count for "settles")
    frs = sc.frame_randoms(n_frames + n_spare, seed=5)

    def run(pin, feed):
        cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H, log2_train_batch_size=10)
        if pin:
            ren.SetSchedule(**pin)
        ren.SetBlend(True)
        if feed == "batches":
            for k in range(0, n_frames, 32):
                ren.RenderFrames(frs[k:k + 32], True)
        else:
            for f in range(96):
                ren.SetFrameRandom(frs[f])
                ren.Render(None, True)
                torch_gpu.cuda.synchronize()
        out = [ren.GetImage().cpu().numpy().copy(), nrc.GetParams(0).copy(), ren.GetSchedule()]
        k = n_frames
        while feed == "batches" and not out[2]["tuning_done"] and k < n_frames + n_spare:
            ren.RenderFrames(frs[k:k + 32], True)
            k += 32
            out[2] = ren.GetSchedule()
        ren.Destroy()
        nrc.Destroy()
        return out

    knobs = lambda s_: (s_["camera_priority_low"], s_["cost_order_lag"], s_["xcd_window"])
    api.clear_schedule_cache()      # (what earlier tuners of this process settled on, and the package's table: this test starts from the defaults)
    pinned = run(dict(camera_priority_low=0, cost_order_lag=2, xcd_window=2), "batches")
    assert pinned[2]["source"] == "pinned"
    free = run(None, "batches")
    assert free[2]["source"] == "tuner" and free[2]["key"].startswith("gfx950:256cu:8xcd|pos3.dir0.w64.d6.hg0|vol2^24|1920x1080.of1920x1080|train1x1024")
    # what the tuner settled on is remembered under the renderer's key: the next renderer of this kind STARTS on it and skips the trials --
    # a run shorter than the tuner's ~400 frames is a tuned run (nrc_schedule_cache_save / _load carry the table to the next process)
    cached = run(None, "sync")
    assert cached[2]["source"] == "cache" and cached[2]["tuning_done"] and knobs(cached[2]) == knobs(free[2])
    api.clear_schedule_cache()
    part = run(dict(cost_order_lag=3), "batches")
    assert pinned[2]["tuning_done"] and free[2]["tuning_done"] and part[2]["tuning_done"]
    assert part[2]["cost_order_lag"] == 3
    assert free[2]["camera_priority_low"] in (0, 1) and free[2]["cost_order_lag"] in (2, 3) and free[2]["xcd_window"] in (0, 2, 16)
    for other in (free, part):
        assert np.array_equal(pinned[0].view(np.uint32), other[0].view(np.uint32))
        assert np.array_equal(pinned[1].view(np.uint32), other[1].view(np.uint32))
    api.clear_schedule_cache()
    starved = run(None, "sync")
    assert not starved[2]["tuning_done"] or knobs(starved[2]) == (0, 2, 2)
    assert starved[2]["source"] in ("default", "tuner")
    assert (starved[2]["camera_priority_low"], starved[2]["cost_order_lag"], starved[2]["xcd_window"]) == (0, 2, 2)


@pytest.mark.parametrize("model", [(2, 2, 64, 3), (3, 0, 128, 2), (3, 0, 64, 6)], ids=["generic-64", "generic-128", "fused"])
def test_deferred_compositing_inside_render_frames_changes_no_pixel(api, sc, cloud16, torch_gpu, model, monkeypatch):
    """nrc_renderer_render_frames composites every frame but its last on the train-ray stream, one frame late (round 4: stream C --
    inference, then compositing -- bounds the frame of a heavy model; nrc_schedule.composite_defer): pure scheduling -- after 3 calls of 4
    trained, blended frames the framebuffer, the loss, the parameters and the frame timeline's shape equal the undeferred order and the
    frame-by-frame Render loop bit for bit"""
    W, H = 256, 160
    scene = sc.make_scene(cloud16, scene_id=4)
    frs = sc.frame_randoms(12, seed=27)
    results = []
    for mode in ("0", "1", "1", "1", "loop"):
        cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H, pos_id=model[0], dir_id=model[1], nn_width=model[2], nn_depth=model[3],
                                        log2_train_batch_size=10)
        ren.SetSchedule(composite_defer=0 if mode == "0" else 1)
        ren.SetBlend(True)
        if mode == "loop":
            for f in range(12):
                ren.SetFrameRandom(frs[f])
                ren.Render(None, True)
        else:
            for k in range(3):
                ren.RenderFrames(frs[4 * k:4 * k + 4], True)      # no host synchronisation between the calls
        img = ren.GetImage().cpu().numpy().copy()
        tl = ren.FrameTimeline()
        assert tl.shape == (12, 6) and np.isfinite(tl).all() and (tl[:, 4] >= tl[:, 3]).all()      # every frame's compositing was timed
        results.append((img, nrc.GetLoss(), nrc.GetParams(0).copy()))
        ren.Destroy()
        nrc.Destroy()
    base = results[0]
    assert np.abs(base[0]).max() > 0.0
    for other in results[1:]:
        assert np.array_equal(base[0].view(np.uint32), other[0].view(np.uint32))
        assert base[1] == other[1]
        assert np.array_equal(base[2].view(np.uint32), other[2].view(np.uint32))


@pytest.mark.parametrize("model", [(2, 0, 64, 3, 0), (3, 0, 128, 2, 0), (1, 0, 32, 2, 0), (0, 0, 64, 2, 11), (3, 0, 64, 6, 0), (2, 2, 64, 3, 0)],
                         ids=["triwave-64", "enc80-128", "identity-32", "hashgrid-64", "fused", "triwave-dir-64"])
def test_live_query_list_changes_no_pixel(api, sc, cloud16, torch_gpu, model, monkeypatch):
    """renderer inference builds its 32-query tiles from the frame's live-query list (k_gen_rays appends the query index of every
    pixel that scattered; k_infer, k_infer_gen, k_encode_hash_list) instead of computing every tile of four pixel rows that holds a
    live query: results are per query, so framebuffer, loss and parameters after 6 trained frames equal the list-free path
    (NRC_DEBUG=no_live_list) bit for bit, and so does the radiance of every scattered pixel of the last frame.
    (256x160 is at most 40 960 queries: one round of every inference kernel and less than one stride of the list encoder.  Frames past a
    round, against the dense kernel per live pixel: test_gpu_renderer_inference_rounds.py)"""
    W, H = 256, 160
    scene = sc.make_scene(cloud16, scene_id=4)
    frs = sc.frame_randoms(6, seed=29)
    results = []
    for no_list in ("1", None, None, "zero-dead"):      # ("zero-dead": the list, with gen_rays writing the zero queries of unscattered pixels)
        nrc_debug(monkeypatch, no_live_list=no_list == "1", zero_dead_queries=no_list == "zero-dead")
        cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H, pos_id=model[0], dir_id=model[1], nn_width=model[2], nn_depth=model[3],
                                        hashgrid_log2_size=model[4], log2_infer_batch_size=21)      # ONE inference batch: the list is used
        ren.SetBlend(True)
        # (a HashGrid model's table gradient is summed with fp16 atomics in no fixed order -- its training is not bitwise repeatable: untrained)
        ren.RenderFrames(frs, model[0] != 0)
        img = ren.GetImage().cpu().numpy().copy()
        info = ren.Buffer("info").cpu().numpy().reshape(-1).copy()
        rad = ren.Buffer("infer_output").cpu().numpy().reshape(-1, 3).copy()
        qry = ren.Buffer("infer_input").cpu().numpy().reshape(-1, 5).copy()
        results.append((img, nrc.GetLoss(), nrc.GetParams(0).copy(), info, rad, qry))
        ren.Destroy()
        nrc.Destroy()
    base = results[0]
    live = base[3].reshape(H, W).T.reshape(-1) == 1.0      # the radiance buffer is handed out in the reference's x * H + y order
    assert live.sum() > 1000 and np.isfinite(base[4][live]).all()
    if model[1] == 0:      # (only the OneBlob direction encoding absorbs the NaN angle of quirk Q5: the other models' training batches carry it into
        assert np.abs(base[4][live]).max() > 0.0      # the weights, and their radiance is 0 with and without the list)
    for other in results[1:]:
        assert np.array_equal(base[0].view(np.uint32), other[0].view(np.uint32))
        assert base[1] == other[1]
        assert np.array_equal(base[2].view(np.uint32), other[2].view(np.uint32))
        assert np.array_equal(base[3], other[3])
        assert np.array_equal(base[4][live].view(np.uint32), other[4][live].view(np.uint32))
        # the query buffer as it is handed out: bit-identical, zeros where the pixel did not scatter (the reference's zero-filled slots)
        assert np.array_equal(base[5].view(np.uint32), other[5].view(np.uint32)) and not base[5][~live].any() and not other[4][~live].any()


def test_wave_priority_switch_changes_no_pixel(api, sc, cloud16, torch_gpu):
    """nrc_set_wave_priority_raise(0) leaves every kernel of the library at the hardware's default issue priority instead of s_setprio 3
    (for a process whose foreign kernels -- RCCL's all-reduce -- run beside the renderer; nrc_cache_comm_init selects it for world > 1):
    one priority for the whole library either way, so 8 trained, blended frames agree bit for bit"""
    W, H = 256, 160
    scene = sc.make_scene(cloud16, scene_id=4)
    frs = sc.frame_randoms(8, seed=31)
    results = []
    try:
        for raise_ in (True, False, False, True):
            api.set_wave_priority_raise(raise_)
            cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H)
            ren.SetBlend(True)
            ren.RenderFrames(frs, True)
            results.append((ren.GetImage().cpu().numpy().copy(), nrc.GetLoss(), nrc.GetParams(0).copy()))
            ren.Destroy()
            nrc.Destroy()
    finally:
        api.set_wave_priority_raise(True)
    for other in results[1:]:
        assert np.array_equal(results[0][0].view(np.uint32), other[0].view(np.uint32))
        assert results[0][1] == other[1]
        assert np.array_equal(results[0][2].view(np.uint32), other[2].view(np.uint32))


@pytest.mark.parametrize("model", [(3, 0, 64, 6, 0), (3, 0, 128, 2, 0), (0, 0, 64, 2, 11), (2, 1, 64, 2, 0)], ids=["fused", "enc80-128", "hashgrid", "generic"])
def test_a_view_without_a_scattering_pixel_renders_the_environment(api, orc, sc, cloud16, torch_gpu, model):
    """the camera looks away from the medium: no pixel scatters, the frame's live-query list stays empty (a list-driven inference launch
    with nothing to do, a training step on a ring buffer without a hit) -- four trained frames equal the oracle's gen_rays primary colour"""
    W, H = 128, 80
    scene = sc.make_scene(cloud16, scene_id=4, env=sc.procedural_sky(32, 16))
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=10, log2_infer_batch_size=21, pos_id=model[0], dir_id=model[1], nn_width=model[2],
                        nn_depth=model[3], hashgrid_log2_size=model[4])
    nrc = api.NeuralRadianceCache(cfg)
    cam = sc.make_camera(pos=(64.0, 0.0, 0.0), view_dir=(1.0, 0.0, 0.0), aspect=W / H)      # the medium is behind the camera
    ren = api.NrcHpmRenderer(W, H, False, cam, cfg, scene, nrc)
    frs = sc.frame_randoms(4, seed=5)
    ren.RenderFrames(frs, True)
    img = ren.GetImage().cpu().numpy().reshape(H, W, 4)
    info = ren.Buffer("info").cpu().numpy()
    assert not info.any()
    assert not ren.Buffer("infer_input").cpu().numpy().any() and not ren.Buffer("infer_output").cpu().numpy().any()
    o = orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, frs[3], threads=8)
    assert not o["info"].any()
    assert same_bits(img[..., :3], o["primary"][..., :3]) and (img[..., 3] == 1.0).all() and img[..., :3].std() > 0.0
    ren.Destroy()
    nrc.Destroy()


def test_framebuffer_on_a_consumer_stream(api, sc, cloud16, torch_gpu):
    """GetImage(stream): a read-back stream of the caller is ordered behind each frame's compositing while the render stream runs
    ahead; the copies it makes equal the frames of a renderer that is read synchronously"""
    W, H = 256, 160
    scene = sc.make_scene(cloud16, scene_id=4)
    frs = sc.frame_randoms(6, seed=33)
    side = torch_gpu.cuda.Stream()
    copies = []
    cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H)
    for f in range(6):
        ren.SetFrameRandom(frs[f])
        ren.Render(None, True)
        img = ren.GetImage(side)
        with torch_gpu.cuda.stream(side):
            copies.append(img.clone())          # the framebuffer is overwritten by the next frame's compositing
        side.synchronize()                      # (a real consumer would double-buffer instead of blocking the host)
    got = [c.cpu().numpy() for c in copies]
    ren.Destroy()
    nrc.Destroy()
    cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H)
    for f in range(6):
        ren.SetFrameRandom(frs[f])
        ren.Render(None, True)
        ref = ren.GetImage().cpu().numpy()
        assert np.array_equal(ref.view(np.uint32), got[f].view(np.uint32))
    ren.Destroy()
    nrc.Destroy()


@pytest.mark.parametrize("block", [1, 8])
def test_column_tiles_reproduce_the_whole_frame(api, sc, cloud16, torch_gpu, block):
    """pixel-tile sharding: N interleaved column tiles (single columns / strips of 8) == the single-GPU frame, bit
    for bit (integrator)"""
    from nrc_hpm_renderer_amd import parallel
    W, H, world = 96, 48, 3
    scene = sc.make_scene(cloud16, scene_id=4)
    cam = sc.make_camera(aspect=W / H)
    full = api.McHpmRenderer(W, H, 16, False, cam, scene)
    full.SetFrameRandom(FRAME_RANDOM)
    full.Render()
    whole = full.GetImage().cpu().numpy()
    parts = []
    for r in range(world):
        lw = parallel.local_width(r, world, W, block)
        t = api.McHpmRenderer(lw, H, 16, False, cam, scene, tile=parallel.column_tile(r, world, W, H, block))
        t.SetFrameRandom(FRAME_RANDOM)
        t.Render()
        parts.append(t.GetImage().cpu().numpy())
        t.Destroy()
    assert np.array_equal(parallel.gather_columns(parts, W, block), whole)
    full.Destroy()
    # the NRC renderer's primary pass shards the same way
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=8, log2_infer_batch_size=12)
    prim = []
    for r in range(2):
        lw = parallel.local_width(r, 2, W, block)
        nrc = api.NeuralRadianceCache(cfg)
        ren = api.NrcHpmRenderer(lw, H, False, cam, cfg, scene, nrc, tile=parallel.column_tile(r, 2, W, H, block))
        ren.SetFrameRandom(FRAME_RANDOM)
        ren.Render(None, False)
        prim.append(ren.Buffer("primary").cpu().numpy().reshape(H, lw, 4))
        ren.Destroy()
        nrc.Destroy()
    nrc = api.NeuralRadianceCache(cfg)
    ren = api.NrcHpmRenderer(W, H, False, cam, cfg, scene, nrc)
    ren.SetFrameRandom(FRAME_RANDOM)
    ren.Render(None, False)
    assert np.array_equal(parallel.gather_columns(prim, W, block), ren.Buffer("primary").cpu().numpy().reshape(H, W, 4))
    ren.Destroy()
    nrc.Destroy()
    with pytest.raises(RuntimeError, match="tile"):
        api.McHpmRenderer(W, H, 16, False, cam, scene, tile=(1, 1, W, H))          # columns would exceed the frame
    with pytest.raises(RuntimeError, match="power of two"):
        api.McHpmRenderer(W // 3, H, 16, False, cam, scene, tile=(0, 3, W, H, 3))


def test_compare_images_and_exr_export(api, orc, sc, sphere_scene, torch_gpu, tmp_path):
    from nrc_hpm_renderer_amd import io_exr
    W = H = 64
    cam = sc.make_camera(aspect=1.0)
    a = api.McHpmRenderer(W, H, 8, False, cam, sphere_scene)
    b = api.McHpmRenderer(W, H, 8, False, cam, sphere_scene)
    a.SetFrameRandom(FRAME_RANDOM)
    b.SetFrameRandom([0.9, 0.1, 0.4, 0.6])
    a.Render()
    b.Render()
    ia, ib = a.GetImage(), b.GetImage()
    res = api.CompareImages(ia, ib)
    # all five numbers against the exact-sum reference: each metric within one fp32 ulp, valid equal (tests/image_reference.py) -- the
    # kernels and the oracle alike
    want = ir.metrics_exact(ia.cpu().numpy(), ib.cpu().numpy())
    assert ir.metric_violations(res, want) == []
    assert ir.metric_violations(orc.compare(ia.cpu().numpy(), ib.cpu().numpy()), want) == []
    assert 0 < res["valid"] <= W * H and res["mse"] > 0
    p = str(tmp_path / "out.exr")
    a.ExportOutputImageToFile(None, p)
    assert np.array_equal(io_exr.read_exr(p), ia.cpu().numpy())
    a.Destroy()
    b.Destroy()


def test_set_camera_resets_accumulation(api, sc, sphere_scene, torch_gpu):
    W = H = 32
    cam = sc.make_camera(aspect=1.0)
    mc = api.McHpmRenderer(W, H, 4, True, cam, sphere_scene)
    for _ in range(3):
        mc.Render()
    cam2 = sc.make_camera(pos=(0.0, 0.0, 64.0), view_dir=(0.0, 0.0, -1.0), aspect=1.0)
    mc.SetCamera(None, cam2)
    mc.SetFrameRandom(FRAME_RANDOM)
    mc.Render()
    fresh = api.McHpmRenderer(W, H, 4, False, cam2, sphere_scene)
    fresh.SetFrameRandom(FRAME_RANDOM)
    fresh.Render()
    assert np.array_equal(mc.GetImage().cpu().numpy(), fresh.GetImage().cpu().numpy())
    mc.Destroy()
    fresh.Destroy()


def _gpu_pair(api, sc, cloud16, name, frames, seed=7):
    import exr_pin
    cam = sc.make_camera(aspect=1920 / 1080)
    out = []
    for scene in exr_pin.perturbed(sc, cloud16, name):
        mc = api.McHpmRenderer(1920, 1080, 32, True, cam, scene)
        frs = sc.frame_randoms(frames, seed=seed)
        for f in range(frames):
            mc.SetFrameRandom(frs[f])
            mc.Render()
        out.append(mc.GetImage().cpu().numpy())
        mc.Destroy()
    return out


def test_reference_exr_pin_per_pixel_and_it_bites(api, sc, cloud16, exr_stats, torch_gpu):
    """The reference-held pin at full size (tests/exr_pin.py): McHpmRenderer at 1920x1080, PATH_LENGTH 32, 2048 blended frames of
    the reference's cloud, scenes 0 and 4, down-sampled 8x8 like the fixtures and compared with reference/0/0.exr and
    reference/4/0.exr per pixel: directional term within -2.5 %...+2.5 % (measured -1.95 %: the sixteenth-resolution cloud
    transmits less than the quarter-resolution one the EXRs were rendered with), env term within 1.5 % (measured -0.1 %),
    interior pattern correlation >= 0.98 and per-pixel L2 <= 13 %, silhouette, centre block, maximum, background, relBias.
    The same bounds REJECT renders with one term of the estimator changed (a biting pin): directional light x1.05 / x0.98,
    env x1.1 / x0.8, g 0.75 / 0.85 / -0.8, density x1.1 / x0.9, the light from the opposite side / from above."""
    import exr_pin
    b = exr_pin.bounds()
    own0, own4 = _gpu_pair(api, sc, cloud16, "none", 2048)
    assert np.isfinite(own0).all() and np.isfinite(own4).all()
    st = exr_pin.pin_statistics(exr_pin.downsample8(own0), exr_pin.downsample8(own4))
    assert exr_pin.violations(st, b) == [], st
    # full-resolution facts of SURVEY App. E that need no down-sampling
    assert abs(own4[..., :3].mean() / exr_stats["4"]["mean_rgb_all"] - 1.0) < 0.02
    assert abs(own0[..., :3].mean() / exr_stats["0"]["mean_rgb_all"] - 1.0) < 0.025
    assert abs(own0[..., 3].mean() - exr_stats["0"]["mean_alpha"]) < 0.006
    assert np.allclose(own4[own4[..., 3] == 0][:, :3], exr_stats["4"]["background"], atol=2e-4)
    assert (own0[own0[..., 3] == 0][:, :3] == 0).all()
    # Reference::Result through the product's own metric kernels (nrc_compare_images) on the down-sampled pair
    ref0, ref4 = exr_pin.load_refs()
    for ref, own in ((ref0, exr_pin.downsample8(own0)), (ref4, exr_pin.downsample8(own4))):
        r = api.CompareImages(torch_gpu.from_numpy(ref).cuda(), torch_gpu.from_numpy(own).cuda())
        m = exr_pin.result_metrics(ref, own)
        assert abs(r["mse"] - m["mse"]) < 1e-5 * max(1.0, m["mse"]) and r["valid"] == m["valid"]
        # all five numbers, each metric within one fp32 ulp of the exact sums (the EXRs' alpha is 0 around the cloud: holes in the valid set)
        assert ir.metric_violations(r, ir.metrics_exact(ref, own)) == []
        assert 0 < r["valid"] < ref.shape[0] * ref.shape[1]
        assert abs((r["own_mean"] - r["ref_mean"]) / r["ref_mean"]) < 0.03            # GetRelBias
        assert r["mse"] < 0.01                                                         # measured 0.0048 / 0.0012
    flagged = {}
    for name, must_flag in (("dir_x1.05", "dir_ratio"), ("dir_x0.98", "dir_ratio"), ("env_x1.1", "env_ratio"), ("env_x0.8", "env_ratio"),
                            ("g=0.75", "dir_ratio"), ("g=0.85", "dir_ratio"), ("g=-0.8", "corr0"), ("density_x1.1", "dir_ratio"),
                            ("density_x0.9", "centre0"), ("light_from_opposite_side", "corr0"), ("light_from_above", "corr0")):
        p0, p4 = _gpu_pair(api, sc, cloud16, name, 768)
        bad = exr_pin.violations(exr_pin.pin_statistics(exr_pin.downsample8(p0), exr_pin.downsample8(p4)), b)
        flagged[name] = bad
        assert any(v.startswith(must_flag) for v in bad), (name, bad)


def test_full_size_nrc_frame_rows_bitwise_against_oracle(api, orc, sc, cloud16, torch_gpu):
    """BASELINE size (1920x1080, configs[1]): three bands of rows of the gen_rays outputs -- top edge, image centre through the
    cloud, bottom edge -- are bit-identical to the oracle (same hash RNG, same specified fp32 math), query buffer included"""
    W, H = 1920, 1080
    scene = sc.make_scene(cloud16, scene_id=4, env=sc.procedural_sky(64, 32))
    cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H, log2_train_batch_size=14, log2_infer_batch_size=21)
    ren.SetFrameRandom(FRAME_RANDOM)
    ren.Render(None, False)
    prim = ren.Buffer("primary").cpu().numpy().reshape(H, W, 4)
    info = ren.Buffer("info").cpu().numpy().reshape(H, W)
    q = ren.Buffer("infer_input").cpu().numpy().reshape(W, H, 5)
    scattered = 0
    for y0, y1 in ((0, 8), (536, 548), (1072, 1080)):
        o = orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, FRAME_RANDOM, rows=(y0, y1), threads=8)
        assert np.array_equal(info[y0:y1], o["info"][y0:y1])
        assert np.array_equal(prim[y0:y1].view(np.uint32), o["primary"][y0:y1].view(np.uint32))
        oq = o["infer_input"].reshape(W, H, 5)[:, y0:y1]
        gq = q[:, y0:y1]
        same = (gq.view(np.uint32) == oq.view(np.uint32)) | (np.isnan(gq) & np.isnan(oq))      # quirk Q5: NaN phi
        assert same.all()
        scattered += int(o["info"][y0:y1].sum())
    assert scattered > 2000
    ren.Destroy()
    nrc.Destroy()
    # the ground-truth renderer (mc/render.comp, PATH_LENGTH 32) at the same size: one band through the cloud
    mc = api.McHpmRenderer(W, H, 32, False, cam, scene)
    mc.SetFrameRandom(FRAME_RANDOM)
    mc.Render()
    img = mc.GetImage().cpu().numpy()
    ref, _, _ = orc.mc_render(scene, cam, W, H, 32, FRAME_RANDOM, rows=(540, 546), threads=8)
    assert np.array_equal(img[540:546].view(np.uint32), ref[540:546].view(np.uint32))
    mc.Destroy()


def test_cli_main_loop_and_benchmark_log(torch_gpu, tmp_path):
    """headless main loop (src/main.cu:248-391): 17 positional args, Render(queue, true) per frame, per-frame
    `frame mse relBias CV` log in `output/ <config name>/log.txt`, EXR export"""
    from nrc_hpm_renderer_amd import cli, io_exr
    out = str(tmp_path / "output")
    exr = str(tmp_path / "final.exr")
    argv = ["RelativeL2Luminance", "Adam", "0.01", "0.99", "3", "0", "64", "6", "14", "10", "1", "4", "1.0", "1", "1", "0.0", "32",
            "--frames", "12", "--width", "128", "--height", "80", "--volume", "32", "--benchmark", "--ref-frames", "64",
            "--output", out, "--export", exr]
    assert cli.main(argv) == 0
    name = " RelativeL2Luminance_Adam_0.010000_0.990000_3_0_64_6_14_10_1_4_1.000000_1_1_0.000000_32"
    lines = open(os.path.join(out, name, "log.txt")).read().strip().splitlines()
    assert len(lines) == 12
    rows = np.array([[float(x) for x in ln.split()] for ln in lines])
    assert rows.shape == (12, 4) and np.isfinite(rows).all()
    assert (rows[:, 0] == np.arange(12)).all() and (rows[:, 1] > 0).all()
    img = io_exr.read_exr(exr)
    assert img.shape == (80, 128, 4) and np.isfinite(img).all()
    with pytest.raises(SystemExit):
        cli.main(argv[:5])


def test_hot_tiles_are_started_first_and_change_no_pixel(api, orc, sc, cloud16, torch_gpu):
    """a pixel in the RNG's fixed point inside a tile the empty-space mask rejects walks for the whole launch: gen_rays starts its
    tile first.  The list is computed one frame ahead when the next frame's random numbers are known (RenderFrames) or drawn early
    (unpinned frames: same sequence as without), in front of gen_rays otherwise; frames are bit-identical with the feature off, and
    the oracle agrees"""
    W, H = 256, 144
    scene = sc.make_scene(cloud16, scene_id=4, env=sc.procedural_sky(32, 16))
    cam = sc.make_camera(aspect=W / H)
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=8, log2_infer_batch_size=14, seed=77)
    keys = ("primary", "info", "infer_input", "train_input", "train_target")
    out = {}
    for on in (True, False):
        nrc = api.NeuralRadianceCache(cfg)
        ren = api.NrcHpmRenderer(W, H, True, cam, cfg, scene, nrc)
        ren.SetHotTiles(on)
        got = []
        # pinned, one at a time: the list is computed in front of gen_rays
        ren.SetFrameRandom(STATE0_FRAME_RANDOM)
        ren.Render(None, True)
        got.append(([ren.Buffer(k).cpu().numpy().copy() for k in keys], ren.HotTiles()))
        # announced ahead: frame 1 of these two is the state-0 frame, its list comes from the end of frame 0's work
        ren.RenderFrames(np.array([FRAME_RANDOM, STATE0_FRAME_RANDOM], np.float32), True)
        got.append(([ren.Buffer(k).cpu().numpy().copy() for k in keys], ren.HotTiles()))
        # unpinned: drawn one frame early with the feature on, at the frame with it off -- the same numbers
        for _ in range(5):
            ren.Render(None, True)
        got.append(([ren.Buffer(k).cpu().numpy().copy() for k in keys], ren.HotTiles()))
        out[on] = (got, ren.GetImage().cpu().numpy().copy(), nrc.GetLoss())
        ren.Destroy()
        nrc.Destroy()
    for (fa, _), (fb, _) in zip(out[True][0], out[False][0]):
        for a, b in zip(fa, fb):
            assert same_bits(a, b)
    assert same_bits(out[True][1], out[False][1]) and out[True][2] == out[False][2]
    assert [h for _, h in out[False][0]] == [None, None, None]
    hot = [h for _, h in out[True][0]]
    assert hot[0] == ([(0, 0)], 1, False)            # pixel (2, 3): tile (0, 0), found in front of gen_rays
    assert hot[1] == ([(0, 0)], 1, True)             # ... and one frame ahead
    assert hot[2] == ([], 0, True)
    o = orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, STATE0_FRAME_RANDOM, threads=8)
    for fa, _ in out[True][0][:2]:
        assert same_bits(fa[0].reshape(H, W, 4), o["primary"]) and same_bits(fa[1].reshape(H, W), o["info"])
    assert o["info"][3, 2] == 1.0 and o["info"][:8, :8].sum() == 1.0


# pixels (1080, 90) and (1083, 90) of a 1920x1080 frame -- the same 8x8 tile -- both start in RNG state 0 with this frame random
# (tests/rng_search.py pair 1920 1080): k_hot_tiles, which appends one entry per capped PIXEL, lists tile (135, 11) twice
PAIR_STATE0_FRAME_RANDOM = [0.6137924194335938, 0.015384615398943424, 0.75, 0.125]


def test_a_tile_listed_twice_in_the_hot_list_is_still_traced_once(api, orc, sc, cloud16, torch_gpu):
    """two capped pixels in one tile gave two hot waves on that tile; k_mc_render blends in place (out = b * col + (1 - b) *
    prev), so the tile could be blended twice.  The later duplicate now leaves (camera_wave_tile): the blended Monte-Carlo frame and
    the gen_rays outputs of that tile row are the oracle's, bit for bit"""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import rng_search
    W, H = 1920, 1080
    for px in ((1080, 90), (1083, 90)):
        assert float(rng_search.init_random(px[0], px[1], W, H, PAIR_STATE0_FRAME_RANDOM)) == 0.0
    scene = sc.make_scene(cloud16, scene_id=4, env=sc.procedural_sky(32, 16))
    cam = sc.make_camera(aspect=W / H)
    rows = (88, 96)
    mc = api.McHpmRenderer(W, H, 8, True, cam, scene)
    ref = np.zeros((H, W, 4), np.float32)
    for k, fr in enumerate((FRAME_RANDOM, PAIR_STATE0_FRAME_RANDOM)):      # blend factors 1, 1/2: the second frame reads the first
        mc.SetFrameRandom(fr)
        mc.Render()
        orc.mc_render(scene, cam, W, H, 8, fr, blend=1.0 / (k + 1), out=ref, rows=rows, threads=8)
    img = mc.GetImage().cpu().numpy()
    mc.Destroy()
    assert same_bits(img[rows[0]:rows[1]], ref[rows[0]:rows[1]])
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=8, log2_infer_batch_size=21)
    nrc = api.NeuralRadianceCache(cfg)
    ren = api.NrcHpmRenderer(W, H, False, cam, cfg, scene, nrc)
    ren.SetFrameRandom(PAIR_STATE0_FRAME_RANDOM)
    ren.Render(None, False)
    tiles, n, ahead = ren.HotTiles()
    assert n == 2 and tiles == [(135, 11), (135, 11)] and not ahead      # listed twice (one entry per capped pixel) ...
    o = orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, PAIR_STATE0_FRAME_RANDOM, rows=rows, threads=8)
    prim = ren.Buffer("primary").cpu().numpy().reshape(H, W, 4)
    info = ren.Buffer("info").cpu().numpy().reshape(H, W)
    assert same_bits(prim[rows[0]:rows[1]], o["primary"][rows[0]:rows[1]]) and same_bits(info[rows[0]:rows[1]], o["info"][rows[0]:rows[1]])
    assert info[90, 1080] == 1.0 and info[90, 1083] == 1.0               # ... both pixels scattered at their entry points
    ren.Destroy()
    nrc.Destroy()


def test_cost_ordered_tile_launch_is_a_permutation_and_changes_no_pixel(api, sc, cloud16, torch_gpu):
    """the costliest-first launch order of gen_rays' tiles: after the first sort the order is no longer the identity, it is a
    permutation of all tile slots with the provably empty tiles behind the cloud's, and every frame -- primary pass, queries,
    train rays, loss, composited image -- is bit-identical to the renderer that launches in the fixed centre-out order"""
    W, H = 328, 200                       # ragged: 41 x 25 tiles, an odd row of 11 + 1 padding workgroups
    scene = sc.make_scene(cloud16, scene_id=4, env=sc.procedural_sky(32, 16))
    cam = sc.make_camera(aspect=W / H)
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=8, log2_infer_batch_size=14)
    frs = sc.frame_randoms(20, seed=5)
    out = {}
    for on in (True, False):
        nrc = api.NeuralRadianceCache(cfg)
        ren = api.NrcHpmRenderer(W, H, True, cam, cfg, scene, nrc)
        ren.SetCostOrder(on)
        ren.SetBlend(True)
        frames = []
        for f in range(20):               # sorts after frames 0 and 16, in use from frames 2 and 18
            ren.SetFrameRandom(frs[f])
            ren.Render(None, True)
            if f in (0, 1, 2, 17, 19):
                frames.append([ren.Buffer(k).cpu().numpy().copy() for k in ("primary", "info", "infer_input", "train_input", "train_target")])
        order = ren.TileOrder()
        out[on] = (frames, ren.GetImage().cpu().numpy().copy(), nrc.GetLoss(), order, ren.Buffer("info").cpu().numpy().reshape(H, W))
        ren.Destroy()
        nrc.Destroy()
    for fa, fb in zip(out[True][0], out[False][0]):
        for a, b in zip(fa, fb):
            assert same_bits(a, b)
    assert same_bits(out[True][1], out[False][1]) and out[True][2] == out[False][2]
    assert out[True][1][..., :3].std() > 0.01 and (out[True][1][..., 3] == 1.0).all()      # not flat; alpha is 1 everywhere after blended frames
    n = len(out[False][3])
    assert np.array_equal(out[False][3], np.arange(n, dtype=np.uint32))       # off: never sorted
    order = out[True][3]
    assert np.array_equal(np.sort(order), np.arange(n, dtype=np.uint32)) and not np.array_equal(order, np.arange(n, dtype=np.uint32))
    # slot -> tile (centre-out rows of 4-tile workgroups, rows padded to an odd count); scattering tiles come before empty ones
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    row_blocks = ((tiles_x + 3) // 4) | 1
    assert n == row_blocks * 4 * tiles_y
    info = out[True][4]
    scat = np.zeros(n, bool)
    for d in range(n):
        k, j = divmod(d // 4, row_blocks)
        tx = j * 4 + d % 4
        mid = tiles_y // 2
        ty = mid - (k + 1) // 2 if k & 1 else mid + k // 2
        if tx < tiles_x:
            scat[d] = info[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8].mean() > 0.5
    assert scat.sum() > 20
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    assert rank[scat].mean() < 0.5 * rank[~scat].mean()
    # XCD-aware finish (k_tile_order_xcd, round 4): behind the two workgroups of the hot tiles, every whole window of 64 ranks (a 16^3
    # volume: M = 2, sixteen workgroups, two per XCD) hands its tiles to the XCDs by screen row -- XCD x (workgroups x and x + 8 of the
    # window) holds positions 8 x .. 8 x + 7 of the window's tiles sorted by (row, slot in the row)
    k_of = order // (row_blocks * 4)
    ty_of = np.where(k_of & 1, tiles_y // 2 - (k_of + 1) // 2, tiles_y // 2 + k_of // 2)
    key = ty_of.astype(np.int64) * 65536 + order % (row_blocks * 4)
    whole = 0
    for r0 in range(64 - 8, n - 64 + 1, 64):
        win = key[r0:r0 + 64].reshape(16, 4)                       # [workgroup of the window][wave]
        by_xcd = np.concatenate([np.concatenate([win[x], win[x + 8]]) for x in range(8)])
        assert np.all(np.diff(by_xcd) > 0), r0
        whole += 1
    assert whole >= (n - 64) // 64 - 1
    # the MC renderer orders its launch the same way (one stream: the sort follows the sampled frame)
    imgs = {}
    for on in (True, False):
        mc = api.McHpmRenderer(W, H, 8, True, cam, scene)
        mc.SetCostOrder(on)
        for f in range(3):
            mc.SetFrameRandom(frs[f])
            mc.Render()
        imgs[on] = mc.GetImage().cpu().numpy().copy()
        mc.Destroy()
    assert same_bits(imgs[True], imgs[False]) and imgs[True][..., :3].std() > 0.01


def test_schedule_cache_file_roundtrip(api, sc, cloud16, torch_gpu, tmp_path):
    """nrc_schedule_cache_save / _load / _clear: an entry under a renderer's key makes the next renderer of that kind start on it (source
    "cache", no trials); entries of other keys never match; damaged lines are skipped; and -- like every value of every knob -- the cached
    schedule changes no pixel"""
    W, H = 256, 128
    scene = sc.make_scene(cloud16, scene_id=4)
    api.clear_schedule_cache()
    cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H)
    s0 = ren.GetSchedule()
    assert s0["source"] == "default" and not s0["tuning_done"] and s0["key"]
    frs = sc.frame_randoms(6, seed=3)
    ren.RenderFrames(frs, True)
    img0, w0 = ren.GetImage().cpu().numpy().copy(), nrc.GetParams(0).copy()
    ren.Destroy()
    nrc.Destroy()
    path = str(tmp_path / "schedules.txt")
    with open(path, "w") as f:
        f.write("# a comment\n%s 1 3 16\nsome-other-device|model 0 2 0\n%s 1 99 16\nnot a line\n" % (s0["key"], s0["key"] + "x"))
    assert api.load_schedule_cache(path) == 2          # (the lag of 99 is outside nrc_schedule's range: skipped, like the free text)
    cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H)
    s1 = ren.GetSchedule()
    assert s1["source"] == "cache" and s1["tuning_done"] and (s1["camera_priority_low"], s1["cost_order_lag"], s1["xcd_window"]) == (1, 3, 16)
    ren.RenderFrames(frs, True)
    assert np.array_equal(img0.view(np.uint32), ren.GetImage().cpu().numpy().view(np.uint32)) and np.array_equal(w0, nrc.GetParams(0))
    ren.SetSchedule(cost_order_lag=2)                   # a caller that knows better still pins
    assert ren.GetSchedule()["cost_order_lag"] == 2 and ren.GetSchedule()["source"] == "pinned in part"
    ren.Destroy()
    nrc.Destroy()
    out = str(tmp_path / "saved.txt")
    assert api.save_schedule_cache(out) == 2
    api.clear_schedule_cache()
    assert api.load_schedule_cache(out) == 2
    api.clear_schedule_cache()
    with pytest.raises(RuntimeError, match="cannot read schedule cache"):
        api.load_schedule_cache(str(tmp_path / "missing.txt"))


def _raw_buffer(api, ren, which):
    """nrc_renderer_buffer(which) through raw ctypes: (pointer, bytes, host copy as uint32 words), or the error text when it fails"""
    import ctypes as C
    import torch
    n = C.c_size_t(0)
    p = ren.L.nrc_renderer_buffer(ren.h, C.c_int(which), C.byref(n))
    if not p:
        return ren.L.nrc_last_error().decode()
    return p, n.value, api._wrap_device(p, n.value, torch.int32, (n.value // 4,)).cpu().numpy().view(np.uint32).copy()


def test_per_set_buffer_ids_name_the_last_frames_set(api, sc, cloud16, torch_gpu):
    """nrc_renderer_buffer ids 0-4 mean "the last rendered frame's gen_rays set", and that set is (frames - 1) % n_sets: after every one
    of n_sets + 2 trained frames (the sets wrap once) ids 0-3 are the very buffers of ids 16 * (set + 1) + 0..3, id 4 holds what the set's
    id holds, and every id has the size its element type and count give.  Before the first frame the ids mean set 0."""
    W, H = 128, 80
    px = W * H
    scene = sc.make_scene(cloud16, scene_id=4)
    cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H)
    n_sets = 0
    while n_sets < 64 and not isinstance(_raw_buffer(api, ren, 16 * (n_sets + 1)), str):
        n_sets += 1
    assert 2 <= n_sets < 64 and "bad buffer id" in _raw_buffer(api, ren, 16 * (n_sets + 1))
    tg = ren.TrainGrid()
    T = tg["tw"] * tg["th"]
    sizes = [px * 16, px * 4, px * 16, px * 16, px * 20, px * 12, T * 20, T * 12, 8 + max(T, tg["ring_size"]) * 24]

    def check(cur):
        for i in range(4):
            p, n, _ = _raw_buffer(api, ren, i)
            ps, ns, _ = _raw_buffer(api, ren, 16 * (cur + 1) + i)
            assert (p, n) == (ps, ns), (cur, i)
        _, n, q = _raw_buffer(api, ren, 4)
        _, ns, qs = _raw_buffer(api, ren, 16 * (cur + 1) + 4)
        assert n == ns and np.array_equal(q, qs), cur
        assert [_raw_buffer(api, ren, i)[1] for i in range(9)] == sizes

    check(0)                                            # before the first frame: set 0
    frs = sc.frame_randoms(n_sets + 2, seed=11)
    seen = []
    for N in range(1, n_sets + 3):
        ren.SetFrameRandom(frs[N - 1])
        ren.Render(None, True)
        check((N - 1) % n_sets)
        seen.append(_raw_buffer(api, ren, 0)[0])
    assert len(set(seen[:n_sets])) == n_sets and seen[n_sets:] == seen[:2]      # every set once, then round again
    assert "buffers 9-11 belong to a self-training renderer" in _raw_buffer(api, ren, 9)
    ren.Destroy()
    nrc.Destroy()
    cfg, nrc, cam, ren = _nrc_setup(api, sc, scene, W, H, self_train=1)
    ren.SetFrameRandom(frs[0])
    ren.Render(None, True)
    spp = cfg.c.train_spp
    assert [_raw_buffer(api, ren, i)[1] for i in (9, 10, 11)] == [T * spp * 20, T * spp * 16, T * spp * 12]
    ren.Destroy()
    nrc.Destroy()
