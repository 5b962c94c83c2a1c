"""Reprojection on the GPU (include/nrc_hpm.h "Reproject"; k_reproject): every pixel of the kernel's two outputs equals, bit for bit, the host
restatement nrc_test_reproject_host -- csrc/nrc_reproject.hpp's arithmetic, which tests/test_reproject_cpu.py pins to an fp64 statement --,
a path target equals the per-view loop and leaves the frames and the training alone, a denoise target in the same call filters the
accumulated frames, and the accumulated frames of an orbit of the GPU's Monte-Carlo frames are as much better than the raw ones as the
oracle's."""
import numpy as np
import pytest

import denoise_reference as D
import reproject_reference as R

pytestmark = pytest.mark.gpu

V = R.V
CFG = dict(train_batch_count=1, log2_train_batch_size=8, log2_infer_batch_size=12)
KINDS = ("nrc", "mc")
FRAMES = 4.0
CAPPED = dict(max_history=8.0, sigma_depth=1.5)


def _make(api, kind, scene, cam, w=V.W, h=V.H, tile=None, blend=True, path_length=8):
    if kind == "mc":
        return api.McHpmRenderer(w, h, path_length, blend, cam, scene, tile=tile), None
    cfg = api.AppConfig(**CFG)
    nrc = api.NeuralRadianceCache(cfg)
    return api.NrcHpmRenderer(w, h, blend, cam, cfg, scene, nrc, tile=tile), nrc


def _destroy(*pairs):
    for ren, nrc in pairs:
        ren.Destroy()
        if nrc is not None:
            nrc.Destroy()


def _render(ren, kind, fr, train=False):
    ren.SetFrameRandom(fr)
    if kind == "mc":
        ren.Render()
    else:
        ren.Render(None, train)


def _np(t):
    return t.cpu().numpy().copy()


def _gpu(torch, a):
    return torch.from_numpy(np.array(a, np.float32)).cuda()      # (a copy: the fixtures are read-only)


def _differ(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def _same_pair(got, want):
    return R.same_bits(_np(got[0]), want[0]) and R.same_bits(_np(got[1]), want[1])


# ---------------------------------------------------------------------------------------------------------------- 1. kernel == host
@pytest.mark.parametrize("w,h", R.SYNTHETIC_SIZES + (R.SMALL,), ids=["48x32", "ragged44x36", "97x41", "9x7"])
def test_kernel_equals_the_host_restatement_on_the_synthetic_images(api, sc, torch_gpu, w, h):
    """holes, ramps, depth steps, a NaN and a +inf pixel in both images, counts in [1, 40]; every camera pair, a max_history that bites, and
    no history; 97 x 41 spans four 32 x 8 tiles across and six down, with ragged tiles on both edges; 9 x 7 is less than a tile"""
    if (w, h) == R.SMALL:
        host = [np.ascontiguousarray(a[10:17, 20:29]) for a in R.synthetic(48, 32)]
    else:
        host = list(R.synthetic(w, h))
    rgba, aov, hr, hn, ha = host
    d_rgba, d_aov, d_hr, d_hn, d_ha = (_gpu(torch_gpu, a) for a in host)
    for name, (hcam, cam) in R.camera_pairs(sc, w, h).items():
        for p in (R.params(), R.params(**CAPPED)):
            got = api.Reproject((d_hr, d_hn, d_ha, hcam), d_rgba, FRAMES, d_aov, cam, p)
            want = api.test_reproject_host((hr, hn, ha, hcam), rgba, FRAMES, aov, cam, p)
            assert _same_pair(got, want), (name, p, _differ(_np(got[0]), want[0]), _differ(_np(got[1]), want[1]))
    cam = R.camera_pairs(sc, w, h)["orbit2"][1]
    got = api.Reproject(None, d_rgba, 3.0, d_aov, cam)
    assert R.same_bits(_np(got[0]), rgba) and (_np(got[1]) == np.float32(3.0)).all()
    for d, a in zip((d_rgba, d_aov, d_hr, d_hn, d_ha), host):      # (the inputs are left alone)
        assert R.same_bits(_np(d), a)
    out, cnt = torch_gpu.empty_like(d_rgba), torch_gpu.empty_like(d_hn)
    got = api.Reproject((d_hr, d_hn, d_ha, cam), d_rgba, FRAMES, d_aov, cam, None, out=out, out_count=cnt)
    assert got[0].data_ptr() == out.data_ptr() and got[1].data_ptr() == cnt.data_ptr()
    assert _same_pair(got, api.test_reproject_host((hr, hn, ha, cam), rgba, FRAMES, aov, cam))


@pytest.mark.parametrize("name", R.RENDERED)
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_equals_the_host_restatement_on_rendered_frames(api, sc, torch_gpu, kind, name):
    """three views of the orbit, four frames each, of either renderer, carried from view to view with the renderer's own view AOVs"""
    scene, cam0 = V.cases(sc)[name]
    cams = R.orbit(sc)[:3]
    ren = _make(api, kind, scene, cam0, path_length=R.PATH_LENGTH)
    frs = sc.frame_randoms(12, seed=3)
    hist, host_hist = None, None
    for i, cam in enumerate(cams):
        ren[0].SetCamera(None, cam)
        for k in range(4):
            _render(ren[0], kind, frs[4 * i + k])
        img, aov = ren[0].GetImage().contiguous().clone(), ren[0].ViewAov().clone()
        got = api.Reproject(hist, img, FRAMES, aov, cam)
        want = api.test_reproject_host(host_hist, _np(img), FRAMES, _np(aov), cam)
        assert _same_pair(got, want), (i, _differ(_np(got[0]), want[0]), _differ(_np(got[1]), want[1]))
        hist, host_hist = (got[0], got[1], aov, cam), (want[0], want[1], _np(aov), cam)
    medium = host_hist[2][..., 0] != 0.0
    assert medium.sum() > 250 and (~medium).sum() > 50
    assert (host_hist[1][medium] > FRAMES).mean() > 0.95 and (host_hist[1][~medium] == np.float32(FRAMES)).all()
    _destroy(ren)


# ---------------------------------------------------------------------------------------------------------------- 2. paths
def _nrc_state(ren, nrc):
    return dict(loss=nrc.GetLoss(), step=nrc.GetStep(), params=[nrc.GetParams(k).copy() for k in range(4)])


@pytest.mark.parametrize("timed", (False, True), ids=["plain", "timed"])
@pytest.mark.parametrize("kind", KINDS)
def test_path_target_equals_the_loop_and_leaves_everything_else_alone(api, sc, torch_gpu, kind, timed):
    """RenderPath over 3 views x 2 frames with accumulated_out == the loop SetCamera, Render x 2, ViewAov, Reproject with the previous result,
    bitwise in colour and count; `out`, aov_out and (NRC, training) loss, step and weights are bitwise those of the same path without the
    target.  With a denoise target in the same call, denoised[i] == Denoise(accum[i], aov_out[i]) bitwise."""
    torch = torch_gpu
    blk = V.blocks_volume()
    scene = sc.make_scene(blk, scene_id=4)
    cams = R.orbit(sc)[:3]
    frs = sc.frame_randoms(6, seed=5)
    train = kind == "nrc"
    keys = np.stack([blk, np.ascontiguousarray(np.roll(blk, (1, 0, -1), axis=(0, 1, 2)))])
    times = [0.25, 0.5, 1.0] if timed else None
    plain, with_rp, loop = (_make(api, kind, scene, cams[0]) for _ in range(3))
    if timed:
        for r in (plain, with_rp, loop):
            r[0].SetVolumeKeys(keys)
    p = R.params(max_history=3.0)
    dp = D.params(passes=2)
    aov_a = torch.full((3, V.H, V.W, 4), float("nan"), device="cuda")
    aov_b, acc, dn = aov_a.clone(), aov_a.clone(), aov_a.clone()
    cnt = torch.full((3, V.H, V.W), float("nan"), device="cuda")
    out_a = plain[0].RenderPath(cams, 2, frs, train, times=times, aov_out=aov_a)
    out_b = with_rp[0].RenderPath(cams, 2, frs, train, times=times, aov_out=aov_b, accumulated_out=acc, accumulated_counts=cnt, reproject_params=p,
                                  denoised_out=dn, denoise_params=dp)
    torch.cuda.synchronize()
    assert R.same_bits(_np(out_a), _np(out_b)) and R.same_bits(_np(aov_a), _np(aov_b))
    assert R.same_bits(_np(plain[0].GetImage()), _np(with_rp[0].GetImage()))
    if train:
        a, b = _nrc_state(*plain), _nrc_state(*with_rp)
        assert a["step"] == b["step"] and np.float32(a["loss"]).view(np.uint32) == np.float32(b["loss"]).view(np.uint32)
        for k in range(4):
            assert np.array_equal(a["params"][k].view(np.uint32), b["params"][k].view(np.uint32)), k
    got, got_n = _np(acc), _np(cnt)
    assert not np.isnan(got[..., :3]).any() and not np.isnan(got_n).any()
    assert R.same_bits(got[0], _np(out_b[0])) and (got_n[0] == np.float32(2.0)).all()      # (view 0 has no history)
    medium = _np(aov_b[2])[..., 0] != 0.0
    assert medium.sum() > 100 and (got_n[2][medium] > 2.0).mean() > 0.5 and got_n.max() <= 5.0      # (max_history 3 bites: 3 + 2 frames)
    hist = None
    for i, cam in enumerate(cams):
        if timed:
            loop[0].SetVolumeTime(times[i])
        loop[0].SetCamera(None, cam)
        for k in range(2):
            _render(loop[0], kind, frs[2 * i + k], train)
        img, aov = loop[0].GetImage().contiguous().clone(), loop[0].ViewAov().clone()
        assert R.same_bits(_np(img), _np(out_b[i])) and R.same_bits(_np(aov), _np(aov_b[i])), i
        step = api.Reproject(hist, img, 2.0, aov, cam, p)
        assert R.same_bits(got[i], _np(step[0])) and R.same_bits(got_n[i], _np(step[1])), (i, _differ(got[i], _np(step[0])))
        hist = (step[0], step[1], aov, cam)
        assert R.same_bits(_np(dn[i]), _np(api.Denoise(acc[i], aov_b[i], dp))), i      # (accumulate, then filter)
    assert not R.same_bits(_np(dn[2]), _np(api.Denoise(out_b[2].contiguous(), aov_b[2], dp)))
    # the target is consumed: the next path writes nothing
    acc.fill_(7.0)
    cnt.fill_(7.0)
    with_rp[0].RenderPath(cams[:2], 1, frs[:2], False, out=False, aov_out=aov_b[:2].contiguous())
    torch.cuda.synchronize()
    assert (_np(acc) == 7.0).all() and (_np(cnt) == 7.0).all()
    _destroy(plain, with_rp, loop)


# ---------------------------------------------------------------------------------------------------------------- 3. refusals, ownership
@pytest.mark.parametrize("kind", KINDS)
def test_the_invalid_combinations_fail_and_leave_nothing_behind(api, sc, torch_gpu, kind):
    torch = torch_gpu
    scene, cam = V.cases(sc)["blocks_v3"]
    cams = R.orbit(sc)[:3]
    frs = sc.frame_randoms(3, seed=2)
    ren = _make(api, kind, scene, cam)
    _render(ren[0], kind, frs[0])
    aovs = torch.full((3, V.H, V.W, 4), 7.0, device="cuda")
    acc = torch.full((3, V.H, V.W, 4), 7.0, device="cuda")
    cnt = torch.full((3, V.H, V.W), 7.0, device="cuda")
    depths = torch.full((3, V.H, V.W), 60.0, device="cuda")
    before = _np(ren[0].GetImage())

    def untouched(what):
        torch.cuda.synchronize()
        assert R.same_bits(before, _np(ren[0].GetImage())), what
        assert (_np(acc) == 7.0).all() and (_np(cnt) == 7.0).all() and (_np(aovs) == 7.0).all(), what

    # a missing AOV target
    ren[0].SetPathReprojectTarget(acc, cnt)
    with pytest.raises(RuntimeError, match="without an AOV target"):
        ren[0].RenderPath(cams, 1, frs, False, out=False)
    untouched("no AOV target")
    # depths present
    ren[0].SetPathAovTarget(aovs)
    ren[0].SetPathAovDepths(depths)
    ren[0].SetPathReprojectTarget(acc, cnt)
    with pytest.raises(RuntimeError, match="with AOV depths"):
        ren[0].RenderPath(cams, 1, frs, False, out=False)
    untouched("depths")
    # another number of views
    ren[0].SetPathAovTarget(aovs)
    ren[0].SetPathReprojectTarget(acc[:2].contiguous(), cnt[:2].contiguous(), views=2)
    with pytest.raises(RuntimeError, match="reproject target holds 2 views"):
        ren[0].RenderPath(cams, 1, frs, False, out=False)
    untouched("views mismatch")
    # no frame per camera
    ren[0].SetPathAovTarget(aovs)
    ren[0].SetPathReprojectTarget(acc, cnt)
    with pytest.raises(RuntimeError, match="at least one frame per camera"):
        ren[0].RenderPath(cams, 0, frs[:0], False, out=False)
    untouched("zero frames")
    # a singular camera among the path's
    flat = dict(inv_proj_view=np.zeros(16, np.float32), pos=cams[0]["pos"])
    ren[0].SetPathAovTarget(aovs)
    ren[0].SetPathReprojectTarget(acc, cnt)
    with pytest.raises(RuntimeError, match="singular"):
        ren[0].RenderPath([cams[0], flat, cams[2]], 1, frs, False, out=False)
    untouched("singular camera")
    # every target went with the failed calls: a plain path writes none of them
    ren[0].RenderPath(cams, 1, frs, False, out=False)
    torch.cuda.synchronize()
    assert (_np(acc) == 7.0).all() and (_np(cnt) == 7.0).all() and (_np(aovs) == 7.0).all()
    # the keyword form checks before it reaches the library, and bad parameters are refused when the target is set
    with pytest.raises(ValueError, match="needs aov_out"):
        ren[0].RenderPath(cams, 1, frs, False, out=False, accumulated_out=acc)
    with pytest.raises(ValueError, match="needs accumulated_out"):
        ren[0].RenderPath(cams, 1, frs, False, out=False, aov_out=aovs, accumulated_counts=cnt)
    with pytest.raises(RuntimeError, match="reproject"):
        ren[0].SetPathReprojectTarget(acc, cnt, R.params(max_history=0.0))
    with pytest.raises(RuntimeError, match="d_counts"):
        ren[0].SetPathReprojectTarget(acc, None)
    aovs.fill_(7.0)
    ren[0].RenderPath(cams, 1, frs, False, out=False)
    torch.cuda.synchronize()
    assert (_np(acc) == 7.0).all() and (_np(cnt) == 7.0).all() and (_np(aovs) == 7.0).all()
    _destroy(ren)


@pytest.mark.parametrize("kind", KINDS)
def test_a_sharded_renderer_refuses(api, sc, torch_gpu, kind):
    scene, _ = V.cases(sc)["blocks_v3"]
    cam = V.orbit_view(sc, 3, 72 / 32)
    ren = _make(api, kind, scene, cam, 24, 32, tile=(1, 3, 72, 32, 8))
    acc, cnt = torch_gpu.empty((1, 32, 24, 4), device="cuda"), torch_gpu.empty((1, 32, 24), device="cuda")
    with pytest.raises(RuntimeError, match="no pixel neighbours"):
        ren[0].SetPathReprojectTarget(acc, cnt)
    ren[0].SetPathReprojectTarget(None, None)      # (cancelling is always allowed)
    _destroy(ren)


def test_aliasing_and_half_a_history_are_refused_before_anything_is_enqueued(api, sc, torch_gpu):
    torch, C = torch_gpu, api.C
    L = api.load_library()
    host = R.synthetic(48, 32)
    d_rgba, d_aov, d_hr, d_hn, d_ha = (_gpu(torch, a) for a in host)
    hcam, cam = R.camera_pairs(sc, 48, 32)["orbit2"]
    ccam, chcam = api.make_c_camera(cam), api.make_c_camera(hcam)
    p = api.make_c_reproject_params()
    out = torch.full((32, 48, 4), 7.0, device="cuda")
    cnt = torch.full((32, 48), 7.0, device="cuda")

    def call(hist, o, n):
        return L.nrc_reproject(hist[0], hist[1], hist[2], hist[3], d_rgba.data_ptr(), C.c_float(FRAMES), d_aov.data_ptr(), C.byref(ccam), 48, 32, C.byref(p),
                               o, n, None)
    whole = (d_hr.data_ptr(), d_hn.data_ptr(), d_ha.data_ptr(), C.byref(chcam))
    for what, o, n in (("the colour", d_rgba.data_ptr(), cnt.data_ptr()), ("the guide", d_aov.data_ptr(), cnt.data_ptr()),
                       ("the history colour", d_hr.data_ptr(), cnt.data_ptr()), ("the history guide", d_ha.data_ptr(), cnt.data_ptr()),
                       ("a shifted history colour", d_hr.data_ptr() + 16, cnt.data_ptr()), ("the history count", out.data_ptr(), d_hn.data_ptr()),
                       ("the count inside the colour", out.data_ptr(), d_rgba.data_ptr() + 64), ("the other output", out.data_ptr(), out.data_ptr() + 32)):
        assert call(whole, o, n) == -1, what
        assert b"overlaps" in L.nrc_last_error(), what
    for half in ((None, whole[1], whole[2], whole[3]), (whole[0], None, whole[2], whole[3]), (whole[0], whole[1], None, whole[3]),
                 (whole[0], whole[1], whole[2], None), (None, None, None, whole[3])):
        assert call(half, out.data_ptr(), cnt.data_ptr()) == -1 and b"all or none" in L.nrc_last_error()
    assert call(whole, out.data_ptr() + 4, cnt.data_ptr()) == -1 and b"aligned" in L.nrc_last_error()
    torch.cuda.synchronize()
    assert (_np(out) == 7.0).all() and (_np(cnt) == 7.0).all()      # (nothing was enqueued)
    for d, a in zip((d_rgba, d_aov, d_hr, d_hn, d_ha), host):
        assert R.same_bits(_np(d), a)
    assert call(whole, out.data_ptr(), cnt.data_ptr()) == 0
    assert _same_pair((out, cnt), api.test_reproject_host((host[2], host[3], host[4], hcam), host[0], FRAMES, host[1], cam))
    with pytest.raises(ValueError):
        api.Reproject((d_hr, d_hn, d_ha, hcam), d_rgba, FRAMES, d_aov, cam, out=d_rgba[:, :24])
    with pytest.raises(RuntimeError, match="reproject"):
        api.Reproject((d_hr, d_hn, d_ha, hcam), d_rgba, FRAMES, d_aov, cam, R.params(sigma_alpha=float("nan")))


@pytest.mark.parametrize("kind", KINDS)
def test_a_renderer_given_a_target_allocates_nothing(api, sc, torch_gpu, kind):
    torch = torch_gpu
    scene, cam = V.cases(sc)["blocks_v3"]
    cams = R.orbit(sc)[:2]
    ren = _make(api, kind, scene, cam)
    aovs, acc = torch.empty((2, V.H, V.W, 4), device="cuda"), torch.empty((2, V.H, V.W, 4), device="cuda")
    cnt = torch.empty((2, V.H, V.W), device="cuda")
    frs = sc.frame_randoms(2, seed=2)
    ren[0].RenderPath(cams, 1, frs, False, out=False, aov_out=aovs)      # (whatever a path with an AOV target allocates, it has now)
    torch.cuda.synchronize()
    before = api.live_allocations()
    ren[0].RenderPath(cams, 1, frs, False, out=False, aov_out=aovs, accumulated_out=acc, accumulated_counts=cnt)
    torch.cuda.synchronize()
    assert api.live_allocations() == before
    assert (_np(cnt)[1] > 1.0).sum() > 100      # (and the target was served)
    _destroy(ren)


# ---------------------------------------------------------------------------------------------------------------- 4. quality
@pytest.mark.parametrize("name", R.RENDERED)
def test_quality_on_an_orbit_of_the_gpus_monte_carlo_frames(api, sc, torch_gpu, name):
    """test_reproject_cpu.py's quality condition on the GPU: the orbit (8 views 2 degrees apart, 4 frames each), the frame randoms (seeds 3
    and 4, the mean of 1024 frames of seed 99 at the last view as the truth), the default parameters, the bound and the cap on pixels
    without history are the CPU test's; the frames are the Monte-Carlo renderer's, the guides its view AOVs, and the accumulation is one
    RenderPath call with a reproject target"""
    torch = torch_gpu
    scene, _ = V.cases(sc)[name]
    cams = R.orbit(sc)
    ren = _make(api, "mc", scene, cams[-1], blend=False, path_length=R.PATH_LENGTH)
    truth = torch.zeros((R.H, R.W, 4), device="cuda", dtype=torch.float64)
    for fr in sc.frame_randoms(R.TRUTH_FRAMES, seed=R.TRUTH_SEED):
        _render(ren[0], "mc", fr)
        truth += ren[0].GetImage()
    truth = (truth / R.TRUTH_FRAMES).cpu().numpy()
    _destroy(ren)
    ren = _make(api, "mc", scene, cams[0], blend=True, path_length=R.PATH_LENGTH)
    ratios, shares = {}, {}
    for seed in R.QUALITY_SEEDS:
        aovs = torch.empty((R.ORBIT_VIEWS, R.H, R.W, 4), device="cuda")
        acc, cnt = torch.empty_like(aovs), torch.empty((R.ORBIT_VIEWS, R.H, R.W), device="cuda")
        raw = ren[0].RenderPath(cams, R.ORBIT_FRAMES, sc.frame_randoms(R.ORBIT_VIEWS * R.ORBIT_FRAMES, seed=seed), False, aov_out=aovs,
                                accumulated_out=acc, accumulated_counts=cnt)
        torch.cuda.synchronize()
        medium = _np(aovs[-1])[..., 0] != 0.0
        ratios[seed] = R.mse(_np(acc[-1]), truth) / R.mse(_np(raw[-1]), truth)
        shares[seed] = float((_np(cnt[-1])[medium] == np.float32(R.ORBIT_FRAMES)).mean())
    print("%s: MSE ratios by seed %s; medium pixels without history %s" % (name, {k: round(v, 3) for k, v in ratios.items()}, shares))
    assert max(ratios.values()) <= R.QUALITY_BOUND
    assert max(shares.values()) <= R.NO_HISTORY_CAP
    _destroy(ren)
