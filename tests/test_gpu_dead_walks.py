"""Ratio tracking stops fetching density once a walk's transmittance is exactly 0 (dead lanes' look-ups get the
border offset).  Only the look-ups change: every stored bit of
k_gen_rays, k_mc_render and k_prep_train stays the oracle's, which keeps multiplying, on media that kill most walks after a few
collisions (tests/dead_walk_cases.py), and the counters say that the rule fired there and nowhere else."""
import numpy as np
import pytest

import dead_walk_cases as dw

pytestmark = pytest.mark.gpu

W, H = dw.W, dw.H


def same_bits(a, b):
    """bit-identical (a NaN matches a NaN)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# CountFetches of the frame below with every ray walked (SetEmptySkip(False)), measured with the commit before the rule: the algorithm's
# collisions, which the rule must not change (they are also what the oracle counts)
PARENT_FETCHES = {"all255": 157384, "all254": 157402, "split": 433369, "cloud": 222100, "thin": 188800}


@pytest.fixture(scope="module")
def cases(orc, sc, cloud16):
    """per scene: (scene, camera, the oracle's gen_rays frame) -- computed once, read by every test"""
    out = {}
    for name in dw.SCENES + ("thin",):
        scene, cam = dw.make_case(sc, name, cloud16)
        out[name] = (scene, cam, orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, dw.FRAME_RANDOM, threads=8))
    return out


def _renderer(api, scene, cam, **cfg_kw):
    kw = dict(train_batch_count=1, log2_train_batch_size=10, log2_infer_batch_size=14)
    kw.update(cfg_kw)
    cfg = api.AppConfig(**kw)
    nrc = api.NeuralRadianceCache(cfg)
    return nrc, api.NrcHpmRenderer(W, H, False, cam, cfg, scene, nrc)


def test_the_saturated_scene_is_dark_in_the_oracle(cases):
    """not vacuous: from the oracle alone, at least half of the scattered pixels of the all-255 scene carry a primary RGB of exactly 0
    (their shadow walks died), and the 254 scene has such pixels too"""
    for name, least in (("all255", 0.5), ("all254", 0.1)):
        o = cases[name][2]
        scattered = o["info"] == 1
        dark = (o["primary"][..., :3] == 0.0).all(axis=2) & scattered
        assert scattered.sum() >= 1024 and dark.sum() >= least * scattered.sum(), (name, int(dark.sum()), int(scattered.sum()))


@pytest.mark.parametrize("name", dw.SCENES)
def test_gen_rays_outputs_are_the_oracles_bits(api, cases, torch_gpu, name):
    scene, cam, o = cases[name]
    nrc, ren = _renderer(api, scene, cam)
    ren.SetFrameRandom(dw.FRAME_RANDOM)
    ren.Render(None, False)
    prim = ren.Buffer("primary").cpu().numpy().reshape(H, W, 4)
    info = ren.Buffer("info").cpu().numpy().reshape(H, W)
    assert np.array_equal(info, o["info"])
    assert np.array_equal(prim.view(np.uint32), o["primary"].view(np.uint32))          # every bit, the sign of a zero included
    live = o["info"].T.reshape(-1) == 1                                                # queries are in x * H + y order
    q = ren.Buffer("infer_input").cpu().numpy()
    assert live.sum() > 1000 and same_bits(q[live], o["infer_input"][live])
    lst = ren.Buffer("live").cpu().numpy().view(np.uint32)
    ys, xs = np.nonzero(o["info"] == 1)
    want = ((ys >> 3) * ((W + 7) >> 3) + (xs >> 3)) * 64 + (ys & 7) * 8 + (xs & 7)
    assert sorted(lst[1:1 + len(want)].tolist()) == sorted(want.tolist())        # (the count word is cleared by the frame's compositing)
    ren.Destroy()
    nrc.Destroy()


@pytest.mark.parametrize("name", dw.SCENES)
def test_mc_frame_is_the_oracles_bits(api, orc, cases, torch_gpu, name):
    scene, cam, _ = cases[name]
    mc = api.McHpmRenderer(W, H, 4, False, cam, scene)
    mc.SetFrameRandom(dw.FRAME_RANDOM)
    mc.Render()
    img = mc.GetImage().cpu().numpy()
    ref, _, _ = orc.mc_render(scene, cam, W, H, 4, dw.FRAME_RANDOM, threads=8)
    assert np.array_equal(np.ascontiguousarray(img, np.float32).view(np.uint32), np.ascontiguousarray(ref, np.float32).view(np.uint32))
    mc.Destroy()


@pytest.mark.parametrize("name", dw.SCENES)
def test_train_rays_and_ring_are_the_oracles_bits(api, orc, sc, cases, torch_gpu, name):
    """k_prep_train over two frames: the light sums, fminf(8, .) and the ring see dead walks' zeros"""
    scene, cam, _ = cases[name]
    nrc, ren = _renderer(api, scene, cam, compat_fix=3, train_spp=2, train_ray_length=3)
    tg = ren.TrainGrid()
    T = tg["tw"] * tg["th"]
    head_tail = np.zeros(2, np.uint32)
    ring = np.zeros((T, 6), np.float32)
    ring[:, 5] = 1.0
    frs = sc.frame_randoms(2, seed=3)
    for f in range(2):
        ren.SetFrameRandom(frs[f])
        ren.Render(None, False)
        o = orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, frs[f], threads=8)
        tin, tgt = orc.nrc_prep_train(scene, W, H, tg["tw"], tg["th"], tg["x_dist"], tg["y_dist"], 2, 3, tg["ring_size"],
                                      frs[f], o["info"], o["origin"], o["dir"], head_tail, ring, threads=8)
        assert same_bits(ren.Buffer("train_input").cpu().numpy(), tin)
        assert same_bits(ren.Buffer("train_target").cpu().numpy(), tgt)
        rb = ren.Buffer("ring").cpu().numpy()
        assert rb[0].view(np.uint32) == head_tail[0] and rb[1].view(np.uint32) == head_tail[1]
        assert same_bits(rb[2:].view(np.float32).reshape(-1, 6)[:tg["ring_size"]], ring[:tg["ring_size"]])
    assert head_tail[0] > 0
    ren.Destroy()
    nrc.Destroy()


@pytest.mark.parametrize("name", dw.SCENES + ("thin",))
def test_counters(api, cases, torch_gpu, name):
    """CountFetches keeps counting the algorithm's collisions (the parent's and the oracle's number); MaskedFetches, the look-ups of
    them that a dead walk kept from memory, is 0 on a medium that cannot take a product to 0 and positive on the saturated ones"""
    scene, cam, o = cases[name]
    nrc, ren = _renderer(api, scene, cam)
    ren.SetEmptySkip(False)
    ren.CountFetches(True)
    ren.SetFrameRandom(dw.FRAME_RANDOM)
    ren.Render(None, False)
    masked = ren.MaskedFetches()
    n_fetch = ren.CountFetches(False)
    print("%s: fetches %d, masked %d" % (name, n_fetch, masked))
    assert n_fetch == o["n_fetch"]
    if PARENT_FETCHES[name] is not None:
        assert n_fetch == PARENT_FETCHES[name]
    assert masked <= n_fetch
    if name == "thin":
        assert int(scene["density"].max()) <= 64 and masked == 0
    if name in ("all255", "all254", "split"):
        assert masked > 0
    if name == "all255":          # a walk dies after six collisions and has some twenty: most look-ups are masked
        assert masked > n_fetch // 4
    ren.Destroy()
    nrc.Destroy()
