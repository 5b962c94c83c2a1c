"""The tracking loops' per-trip bookkeeping ("Trip overhead": the cap of 128 collisions as a lane mask, both voxel
indices and both cell indices of a trip behind one wait-state pad each, the located trip's predicates as lane masks) changes no stored bit:
k_gen_rays, k_mc_render and k_prep_train against the oracle on the media of tests/trip_edge_cases.py -- walks that end on the cap, walks
that accept at every place of a trip up to the cap, a volume of 20 x 12 x 36 voxels -- with the empty-space skip on and off.
(tests/test_trip_edge_cases_cpu.py shows from the oracle alone that the media do that.)"""
import numpy as np
import pytest

import trip_edge_cases as te

pytestmark = pytest.mark.gpu

W, H = te.W, te.H
SKIP = (False, True)


def same_bits(a, b):
    """bit-identical (a NaN matches a NaN)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def cases(orc, sc):
    """per case: (scene, camera, the oracle's gen_rays frame) -- computed once, read by every test"""
    out = {}
    for name in te.CASES:
        scene, cam = te.make_case(sc, name)
        out[name] = (scene, cam, orc.nrc_gen_rays(scene, cam, W, H, 1, 0.0, te.FRAME_RANDOM[name], threads=8))
    return out


@pytest.fixture(scope="module")
def mc_frames(orc, cases):
    return {name: orc.mc_render(cases[name][0], cases[name][1], W, H, 4, te.FRAME_RANDOM[name], threads=8)[0] for name in te.CASES}


@pytest.fixture(scope="module")
def train_frames(orc, sc, cases):
    """per case: the frame randoms of two frames and the oracle's gen_rays frames for them (the ring is replayed by the test)"""
    frs = sc.frame_randoms(2, seed=3)
    return frs, {name: [orc.nrc_gen_rays(cases[name][0], cases[name][1], W, H, 1, 0.0, frs[f], threads=8) for f in range(2)] for name in te.CASES}


def _renderer(api, scene, cam, **cfg_kw):
    kw = dict(train_batch_count=1, log2_train_batch_size=10, log2_infer_batch_size=14)
    kw.update(cfg_kw)
    cfg = api.AppConfig(**kw)
    nrc = api.NeuralRadianceCache(cfg)
    return nrc, api.NrcHpmRenderer(W, H, False, cam, cfg, scene, nrc)


@pytest.mark.parametrize("skip", SKIP)
@pytest.mark.parametrize("name", te.CASES)
def test_gen_rays_outputs_are_the_oracles_bits(api, cases, torch_gpu, name, skip):
    scene, cam, o = cases[name]
    nrc, ren = _renderer(api, scene, cam)
    ren.SetEmptySkip(skip)
    ren.SetFrameRandom(te.FRAME_RANDOM[name])
    ren.Render(None, False)
    prim = ren.Buffer("primary").cpu().numpy().reshape(H, W, 4)
    info = ren.Buffer("info").cpu().numpy().reshape(H, W)
    assert np.array_equal(info, o["info"])
    assert np.array_equal(prim.view(np.uint32), o["primary"].view(np.uint32))          # every bit, the sign of a zero included
    live = o["info"].T.reshape(-1) == 1                                                # queries are in x * H + y order
    q = ren.Buffer("infer_input").cpu().numpy()
    assert live.sum() >= 256 and same_bits(q[live], o["infer_input"][live])
    lst = ren.Buffer("live").cpu().numpy().view(np.uint32)
    ys, xs = np.nonzero(o["info"] == 1)
    want = ((ys >> 3) * ((W + 7) >> 3) + (xs >> 3)) * 64 + (ys & 7) * 8 + (xs & 7)
    assert sorted(lst[1:1 + len(want)].tolist()) == sorted(want.tolist())        # (the count word is cleared by the frame's compositing)
    ren.Destroy()
    nrc.Destroy()


@pytest.mark.parametrize("skip", SKIP)
@pytest.mark.parametrize("name", te.CASES)
def test_mc_frame_is_the_oracles_bits(api, cases, mc_frames, torch_gpu, name, skip):
    scene, cam, _ = cases[name]
    mc = api.McHpmRenderer(W, H, 4, False, cam, scene)
    mc.SetEmptySkip(skip)
    mc.SetFrameRandom(te.FRAME_RANDOM[name])
    mc.Render()
    img = mc.GetImage().cpu().numpy()
    ref = mc_frames[name]
    assert np.array_equal(np.ascontiguousarray(img, np.float32).view(np.uint32), np.ascontiguousarray(ref, np.float32).view(np.uint32))
    mc.Destroy()


@pytest.mark.parametrize("skip", SKIP)
@pytest.mark.parametrize("name", te.CASES)
def test_train_rays_and_ring_are_the_oracles_bits(api, orc, cases, train_frames, torch_gpu, name, skip):
    """k_prep_train with compat_fix 3, two samples of three segments per train ray, over two frames"""
    scene, cam, _ = cases[name]
    frs, gen = train_frames
    nrc, ren = _renderer(api, scene, cam, compat_fix=3, train_spp=2, train_ray_length=3)
    ren.SetEmptySkip(skip)
    tg = ren.TrainGrid()
    T = tg["tw"] * tg["th"]
    head_tail = np.zeros(2, np.uint32)
    ring = np.zeros((T, 6), np.float32)
    ring[:, 5] = 1.0
    for f in range(2):
        ren.SetFrameRandom(frs[f])
        ren.Render(None, False)
        o = gen[name][f]
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
