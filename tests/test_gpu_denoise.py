"""The denoise filter on the GPU (include/nrc_hpm.h "Denoise"; k_denoise_pass): every pixel and channel of the kernel's result equals, bit
for bit, the host restatement nrc_test_denoise_host -- csrc/nrc_denoise.hpp's arithmetic, which tests/test_denoise_cpu.py pins to an fp64
statement --, the renderer calls equal the free function, a path target equals the per-view loop and leaves the frames alone, and the
filter buys on the GPU's Monte-Carlo frames what it buys on the oracle's."""
import numpy as np
import pytest

import denoise_reference as D

pytestmark = pytest.mark.gpu

R = D.V
CFG = dict(train_batch_count=1, log2_train_batch_size=8, log2_infer_batch_size=12)
KINDS = ("nrc", "mc")
COLOUR_ON = dict(sigma_color=1.5, color_decay=0.5)


def _make(api, kind, scene, cam, w=R.W, h=R.H, tile=None, blend=True, path_length=8):
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


# ---------------------------------------------------------------------------------------------------------------- 1. kernel == host
@pytest.mark.parametrize("w,h", D.SYNTHETIC_SIZES, ids=["48x32", "ragged44x36", "97x41"])
def test_kernel_equals_the_host_restatement_on_the_synthetic_images(api, torch_gpu, w, h):
    """holes, ramps, depth steps, a NaN and a +inf pixel; 1 .. 6 passes (strides 1 .. 32) and the colour term on; 97 x 41 spans four 32 x 8
    tiles across and six down, with ragged tiles on both edges"""
    rgba, aov = D.synthetic(w, h)
    d_rgba, d_aov = _gpu(torch_gpu, rgba), _gpu(torch_gpu, aov)
    for p in [D.params(passes=n) for n in range(1, 7)] + [D.params(passes=3, **COLOUR_ON), D.params(passes=6, sigma_color=0.75, color_decay=0.8)]:
        got, want = _np(api.Denoise(d_rgba, d_aov, p)), api.test_denoise_host(rgba, aov, p)
        assert D.same_bits(got, want), (p, _differ(got, want))
    assert D.same_bits(_np(d_rgba), rgba) and D.same_bits(_np(d_aov), aov)      # (the inputs are left alone)
    out = torch_gpu.empty_like(d_rgba)
    assert api.Denoise(d_rgba, d_aov, None, out=out).data_ptr() == out.data_ptr()
    assert D.same_bits(_np(out), api.test_denoise_host(rgba, aov))


@pytest.mark.parametrize("name", D.RENDERED)
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_equals_the_host_restatement_on_rendered_frames(api, sc, torch_gpu, kind, name):
    """a blend of four frames of either renderer, filtered with the renderer's own view AOV"""
    scene, cam = R.cases(sc)[name]
    ren = _make(api, kind, scene, cam, path_length=D.PATH_LENGTH)
    for fr in sc.frame_randoms(4, seed=3):
        _render(ren[0], kind, fr)
    img, aov = ren[0].GetImage().contiguous(), ren[0].ViewAov()
    h_img, h_aov = _np(img), _np(aov)
    assert (h_aov[..., 0] > 0).sum() > 250 and (h_aov[..., 0] == 0).sum() > 50
    for p in (D.params(), D.params(passes=5, **COLOUR_ON)):
        got, want = _np(api.Denoise(img, aov, p)), api.test_denoise_host(h_img, h_aov, p)
        assert D.same_bits(got, want), (p, _differ(got, want))
    _destroy(ren)


# ---------------------------------------------------------------------------------------------------------------- 2. DenoisedFrame
@pytest.mark.parametrize("kind", KINDS)
def test_denoised_frame_is_the_free_function_and_follows_every_change(api, sc, torch_gpu, kind):
    """DenoisedFrame() == Denoise(framebuffer, ViewAov()) bitwise -- and again after more frames, a camera change and a volume swap"""
    blk = R.blocks_volume()
    scene, cam = R.cases(sc)["blocks_v3"]
    ren = _make(api, kind, scene, cam)
    frs = sc.frame_randoms(8, seed=6)
    seen = []

    def check(what, p=None):
        got = _np(ren[0].DenoisedFrame(p))
        want = _np(api.Denoise(ren[0].GetImage().contiguous(), ren[0].ViewAov(), p))
        assert D.same_bits(got, want), (what, _differ(got, want))
        assert D.same_bits(want, api.test_denoise_host(_np(ren[0].GetImage()), _np(ren[0].ViewAov()), p)), what
        assert not any(D.same_bits(got, s) for s in seen), what
        seen.append(got)

    _render(ren[0], kind, frs[0])
    check("first frame")
    a, b = ren[0].DenoisedFrame(), ren[0].DenoisedFrame()
    assert a.data_ptr() == b.data_ptr() and D.same_bits(_np(a), seen[0])      # (the renderer's buffer; the same inputs, the same bits)
    _render(ren[0], kind, frs[1])
    _render(ren[0], kind, frs[2])
    check("more frames")
    check("other parameters", D.params(passes=5, **COLOUR_ON))
    ren[0].SetCamera(None, R.orbit_view(sc, 1))
    _render(ren[0], kind, frs[3])
    check("camera change")
    ren[0].SetVolume(np.ascontiguousarray(np.roll(blk, (5, 3, -4), axis=(0, 1, 2))))
    _render(ren[0], kind, frs[4])
    check("volume swap")
    # frames rendered behind the call do not reach into its result, nor does the call disturb them
    before = _np(ren[0].DenoisedFrame())
    held = ren[0].DenoisedFrame()
    _render(ren[0], kind, frs[5])
    torch_gpu.cuda.synchronize()
    assert D.same_bits(_np(held), before)
    check("a frame behind a call")
    _destroy(ren)


# ---------------------------------------------------------------------------------------------------------------- 3. paths
def _nrc_state(ren, nrc):
    return dict(loss=nrc.GetLoss(), step=nrc.GetStep(), params=[nrc.GetParams(k).copy() for k in range(4)])


@pytest.mark.parametrize("timed", (False, True), ids=["plain", "timed"])
@pytest.mark.parametrize("kind", KINDS)
def test_path_target_equals_the_loop_and_leaves_everything_else_alone(api, sc, torch_gpu, kind, timed):
    """RenderPath over 3 views x 2 frames with denoised_out == SetCamera + Render x 2 + DenoisedFrame per view, bitwise; `out`, aov_out and
    (NRC, training) loss, step and weights are bitwise those of the same path without the target"""
    torch = torch_gpu
    blk = R.blocks_volume()
    scene = sc.make_scene(blk, scene_id=4)
    cams = [R.orbit_view(sc, k) for k in (3, 1, 6)]
    frs = sc.frame_randoms(6, seed=5)
    train = kind == "nrc"
    keys = np.stack([blk, np.ascontiguousarray(np.roll(blk, (5, 3, -4), axis=(0, 1, 2)))])
    times = [0.25, 0.5, 1.0] if timed else None
    plain, with_dn, loop = (_make(api, kind, scene, cams[0]) for _ in range(3))
    if timed:
        for r in (plain, with_dn, loop):
            r[0].SetVolumeKeys(keys)
    p = D.params(passes=4, **COLOUR_ON)
    aov_a = torch.full((3, R.H, R.W, 4), float("nan"), device="cuda")
    aov_b, dn = aov_a.clone(), aov_a.clone()
    out_a = plain[0].RenderPath(cams, 2, frs, train, times=times, aov_out=aov_a)
    out_b = with_dn[0].RenderPath(cams, 2, frs, train, times=times, aov_out=aov_b, denoised_out=dn, denoise_params=p)
    torch.cuda.synchronize()
    assert D.same_bits(_np(out_a), _np(out_b)) and D.same_bits(_np(aov_a), _np(aov_b))
    assert D.same_bits(_np(plain[0].GetImage()), _np(with_dn[0].GetImage()))
    if train:
        a, b = _nrc_state(*plain), _nrc_state(*with_dn)
        assert a["step"] == b["step"] and np.float32(a["loss"]).view(np.uint32) == np.float32(b["loss"]).view(np.uint32)
        for k in range(4):
            assert np.array_equal(a["params"][k].view(np.uint32), b["params"][k].view(np.uint32)), k
    got = _np(dn)
    assert not np.isnan(got[..., :3]).any()
    for i, cam in enumerate(cams):
        # (view i filtered by the free function from the path's own outputs, and by the loop on a third renderer)
        assert D.same_bits(got[i], _np(api.Denoise(out_b[i], aov_b[i], p))), i
        if timed:
            loop[0].SetVolumeTime(times[i])
        loop[0].SetCamera(None, cam)
        for k in range(2):
            _render(loop[0], kind, frs[2 * i + k], train)
        assert D.same_bits(_np(loop[0].GetImage()), _np(out_b[i])), i
        assert D.same_bits(got[i], _np(loop[0].DenoisedFrame(p))), i
    # the target is consumed: the next path writes nothing
    dn.fill_(7.0)
    with_dn[0].RenderPath(cams[:2], 1, frs[:2], False, out=False, aov_out=aov_b[:2].contiguous())
    torch.cuda.synchronize()
    assert (_np(dn) == 7.0).all()
    _destroy(plain, with_dn, loop)


@pytest.mark.parametrize("kind", KINDS)
def test_the_three_invalid_combinations_fail_and_leave_nothing_behind(api, sc, torch_gpu, kind):
    torch = torch_gpu
    scene, cam = R.cases(sc)["blocks_v3"]
    cams = [R.orbit_view(sc, k) for k in (3, 1, 6)]
    frs = sc.frame_randoms(3, seed=2)
    ren = _make(api, kind, scene, cam)
    _render(ren[0], kind, frs[0])
    aovs = torch.full((3, R.H, R.W, 4), 7.0, device="cuda")
    dn = torch.full((3, R.H, R.W, 4), 7.0, device="cuda")
    depths = torch.full((3, R.H, R.W), 60.0, device="cuda")
    before = _np(ren[0].GetImage())

    def untouched(what):
        torch.cuda.synchronize()
        assert D.same_bits(before, _np(ren[0].GetImage())), what
        assert (_np(dn) == 7.0).all() and (_np(aovs) == 7.0).all(), what

    # a missing AOV target
    ren[0].SetPathDenoiseTarget(dn)
    with pytest.raises(RuntimeError, match="without an AOV target"):
        ren[0].RenderPath(cams, 1, frs, False, out=False)
    untouched("no AOV target")
    # an n_views mismatch
    ren[0].SetPathAovTarget(aovs)
    ren[0].SetPathDenoiseTarget(dn[:2].contiguous(), views=2)
    with pytest.raises(RuntimeError, match="denoise target holds 2 views"):
        ren[0].RenderPath(cams, 1, frs, False, out=False)
    untouched("views mismatch")
    # depths present
    ren[0].SetPathAovTarget(aovs)
    ren[0].SetPathAovDepths(depths)
    ren[0].SetPathDenoiseTarget(dn)
    with pytest.raises(RuntimeError, match="with AOV depths"):
        ren[0].RenderPath(cams, 1, frs, False, out=False)
    untouched("depths")
    # every target went with the failed calls: a plain path writes none of them
    ren[0].RenderPath(cams, 1, frs, False, out=False)
    torch.cuda.synchronize()
    assert (_np(dn) == 7.0).all() and (_np(aovs) == 7.0).all()
    # the keyword form checks before it reaches the library, and bad parameters are refused when the target is set
    with pytest.raises(ValueError, match="needs aov_out"):
        ren[0].RenderPath(cams, 1, frs, False, out=False, denoised_out=dn)
    with pytest.raises(RuntimeError, match="denoise"):
        ren[0].SetPathDenoiseTarget(dn, D.params(passes=9))
    ren[0].RenderPath(cams, 1, frs, False, out=False)
    torch.cuda.synchronize()
    assert (_np(dn) == 7.0).all()
    _destroy(ren)


# ---------------------------------------------------------------------------------------------------------------- 4. refusals, ownership
@pytest.mark.parametrize("kind", KINDS)
def test_a_sharded_renderer_refuses(api, sc, torch_gpu, kind, tmp_path):
    scene, _ = R.cases(sc)["blocks_v3"]
    cam = R.orbit_view(sc, 3, 72 / 32)
    ren = _make(api, kind, scene, cam, 24, 32, tile=(1, 3, 72, 32, 8))
    dn = torch_gpu.empty((1, 32, 24, 4), device="cuda")
    for call in (lambda: ren[0].DenoisedFrame(), lambda: ren[0].SetPathDenoiseTarget(dn),
                 lambda: ren[0].ExportDenoisedImageToFile(str(tmp_path / "no.exr"))):
        with pytest.raises(RuntimeError, match="no pixel neighbours"):
            call()
    assert not (tmp_path / "no.exr").exists()
    ren[0].SetPathDenoiseTarget(None)      # (cancelling is always allowed)
    # an unsharded tile description is an ordinary renderer
    whole = _make(api, kind, scene, cam, 72, 32, tile=(0, 1, 72, 32, 8))
    _render(whole[0], kind, [0.25, 0.5, 0.75, 1.0])
    assert np.isfinite(_np(whole[0].DenoisedFrame())).all()
    _destroy(ren, whole)


def test_aliasing_and_bad_arguments_are_refused(api, torch_gpu):
    torch, C = torch_gpu, api.C
    L = api.load_library()
    rgba, aov = D.synthetic(48, 32)
    d_rgba, d_aov = _gpu(torch, rgba), _gpu(torch, aov)
    p = api.make_c_denoise_params()
    n = L.nrc_denoise_scratch_bytes(48, 32, C.byref(p))
    scratch = torch.zeros(n + 48 * 32 * 16, device="cuda", dtype=torch.uint8)
    out = torch.full((32, 48, 4), 7.0, device="cuda")

    def call(o, s):
        return L.nrc_denoise(d_rgba.data_ptr(), d_aov.data_ptr(), 48, 32, C.byref(p), o, s, None)

    for what, o, s in (("the colour", d_rgba.data_ptr(), scratch.data_ptr()), ("the guide", d_aov.data_ptr(), scratch.data_ptr()),
                       ("the scratch's first image", scratch.data_ptr(), scratch.data_ptr()),
                       ("the scratch's guide pairs", scratch.data_ptr() + n - 16, scratch.data_ptr()),
                       ("a shifted colour", d_rgba.data_ptr() + 16, scratch.data_ptr())):
        assert call(o, s) == -1, what
        assert b"overlaps" in L.nrc_last_error(), what
    assert call(out.data_ptr() + 4, scratch.data_ptr()) == -1 and b"aligned" in L.nrc_last_error()
    torch.cuda.synchronize()
    assert D.same_bits(_np(d_rgba), rgba) and (_np(out) == 7.0).all()      # (nothing was enqueued)
    assert call(out.data_ptr(), scratch.data_ptr()) == 0
    assert D.same_bits(_np(out), api.test_denoise_host(rgba, aov))
    with pytest.raises(ValueError):
        api.Denoise(d_rgba, d_aov, None, out=d_rgba[:, :24])
    with pytest.raises(RuntimeError, match="denoise"):
        api.Denoise(d_rgba, d_aov, D.params(sigma_alpha=float("nan")))


@pytest.mark.parametrize("kind", KINDS)
def test_a_renderer_that_never_asks_allocates_nothing(api, sc, torch_gpu, kind):
    scene, cam = R.cases(sc)["blocks_v3"]
    base = api.live_allocations()
    ren = _make(api, kind, scene, cam)
    for fr in sc.frame_randoms(2, seed=1):
        _render(ren[0], kind, fr)
    ren[0].RenderPath([cam, R.orbit_view(sc, 1)], 1, sc.frame_randoms(2, seed=2), False)
    torch_gpu.cuda.synchronize()
    idle = api.live_allocations()
    ren[0].ViewAov()
    with_aov = api.live_allocations()
    assert with_aov == idle + 1
    ren[0].DenoisedFrame()
    assert api.live_allocations() == with_aov + 2      # (the image and the scratch)
    ren[0].DenoisedFrame(D.params(passes=6))
    ren[0].RenderPath([cam], 1, sc.frame_randoms(1, seed=2), False, aov_out=torch_gpu.empty((1, R.H, R.W, 4), device="cuda"),
                      denoised_out=torch_gpu.empty((1, R.H, R.W, 4), device="cuda"))
    assert api.live_allocations() == with_aov + 2      # (first use only)
    _destroy(ren)
    assert api.live_allocations() == base


# ---------------------------------------------------------------------------------------------------------------- 5. quality
@pytest.mark.parametrize("name", D.RENDERED)
def test_quality_on_the_gpus_monte_carlo_frames(api, sc, torch_gpu, name):
    """test_denoise_cpu.py's quality condition on the GPU: the cases, the frame randoms (blends of 1, 4 and 16 frames of seeds 3 and 4, the
    mean of 1024 frames of seed 99 as the truth), the default parameters and the bound <= 0.5 are the CPU test's; the frames are the
    Monte-Carlo renderer's, the guide its view AOV, the filter the kernel"""
    torch = torch_gpu
    scene, cam = R.cases(sc)[name]
    ren = _make(api, "mc", scene, cam, blend=False, path_length=D.PATH_LENGTH)
    truth = torch.zeros((D.H, D.W, 4), device="cuda", dtype=torch.float64)
    for fr in sc.frame_randoms(D.TRUTH_FRAMES, seed=D.TRUTH_SEED):
        _render(ren[0], "mc", fr)
        truth += ren[0].GetImage()
    truth = (truth / D.TRUTH_FRAMES).cpu().numpy()
    _destroy(ren)
    ren = _make(api, "mc", scene, cam, blend=True, path_length=D.PATH_LENGTH)
    aov = ren[0].ViewAov()
    ratios = {}
    for seed in D.QUALITY_SEEDS:
        ren[0].SetCamera(None, cam)      # (restarts the blend)
        for k, fr in enumerate(sc.frame_randoms(max(D.QUALITY_FRAMES), seed=seed), 1):
            _render(ren[0], "mc", fr)
            if k in D.QUALITY_FRAMES:
                img = ren[0].GetImage().contiguous()
                ratios[seed, k] = D.mse(_np(api.Denoise(img, aov)), truth) / D.mse(_np(img), truth)
    print("%s: MSE ratios (seed, frames) %s" % (name, {k: round(v, 3) for k, v in ratios.items()}))
    assert len(ratios) == 6
    assert max(ratios.values()) <= D.QUALITY_BOUND
    _destroy(ren)


# ---------------------------------------------------------------------------------------------------------------- 6. EXR
@pytest.mark.parametrize("kind", KINDS)
def test_exr_denoised_round_trips(api, sc, torch_gpu, kind, tmp_path):
    from nrc_hpm_renderer_amd import io_exr
    scene, cam = R.cases(sc)["blocks_v3"]
    ren = _make(api, kind, scene, cam)
    for fr in sc.frame_randoms(2, seed=9):
        _render(ren[0], kind, fr)
    p = D.params(passes=2)
    path = str(tmp_path / "dn.exr")
    ren[0].ExportDenoisedImageToFile(path, p)
    img, aov, raw = _np(ren[0].DenoisedFrame(p)), _np(ren[0].ViewAov()), _np(ren[0].GetImage())
    planes = io_exr.read_exr_channels(path)
    assert sorted(planes) == ["A", "B", "G", "R", "Z", "Zhalf", "tau"]
    for name, want in (("R", img[..., 0]), ("G", img[..., 1]), ("B", img[..., 2]), ("A", aov[..., 0]), ("tau", aov[..., 1]), ("Z", aov[..., 2]),
                       ("Zhalf", aov[..., 3])):
        assert D.same_bits(planes[name], want), name
    assert not D.same_bits(planes["R"], raw[..., 0])
    assert D.same_bits(img, api.test_denoise_host(raw, aov, p))
    _destroy(ren)
