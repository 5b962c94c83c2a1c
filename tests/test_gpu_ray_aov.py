"""The ray AOV on the GPU (include/nrc_hpm.h "Ray AOV"; k_ray_aov<RayList | ViewDepth | OrthoView>): every ray's {alpha, tau, z_front,
z_half} equals, bit for bit, the host restatement nrc_test_ray_aov_host -- the plain range walk of csrc/nrc_view_aov.hpp, which
tests/test_ray_aov_cpu.py pins to an fp64 reference of the range -- although the kernel jumps out of empty cells by the occupancy bits
and, for the view's depths, skips tiles by the empty-space mask.  Every ray, all four components, no exclusions."""
import numpy as np
import pytest

import ray_aov_reference as Q
import view_aov_reference as R

pytestmark = pytest.mark.gpu

CFG = dict(train_batch_count=1, log2_train_batch_size=8, log2_infer_batch_size=12)
KINDS = ("nrc", "mc")


def _make(api, kind, scene, cam, w=R.W, h=R.H, tile=None, blend=False, path_length=8):
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


def _dev(torch, a):
    return torch.from_numpy(np.array(a, np.float32, order="C")).cuda()      # (a copy: the shared ray sets are read-only)


def _list(torch, ren, rays):
    """RayAov of records [...][8] as numpy [...][4]"""
    recs = np.ascontiguousarray(rays, np.float32)
    return ren.RayAov(_dev(torch, recs.reshape(-1, 8))).cpu().numpy().reshape(recs.shape[:-1] + (4,))


def _differ(got, want):
    return int((np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).any(axis=-1).sum())


_HOST = {}


def _host(api, scene, rays, key):
    """nrc_test_ray_aov_host, once per ray set"""
    if key not in _HOST:
        _HOST[key] = api.test_ray_aov_host(scene, rays)
    return _HOST[key]


# ---------------------------------------------------------------------------------------------------------------- 1. lists
@pytest.mark.parametrize("kind", KINDS)
def test_lists_equal_the_host_restatement_at_every_tail(api, sc, torch_gpu, kind):
    """the random segments of both volumes, the first n = 1, 63, 64, 65, 257, 1024 of them: lane tails, a full wave, a workgroup's tail;
    the same bits without the empty-space skip; nothing is written behind the list's end"""
    torch = torch_gpu
    for volume in ("blocks", "cloud"):
        scene = Q.volume_scene(sc, volume)
        rays = Q.random_segments(scene)
        want = _host(api, scene, rays, "random_" + volume)
        assert (want[:, 1] > 0).sum() > 100
        ren = _make(api, kind, scene, R.orbit_view(sc, 3))
        d_rays = _dev(torch, rays)
        for skip in (True, False):
            ren[0].SetEmptySkip(skip)
            for n in (1, 63, 64, 65, 257, 1024):
                out = torch.full((n + 1, 4), -7.0, device="cuda")
                ren[0].RayAov(d_rays[:n], out=out[:n])
                got = out.cpu().numpy()
                assert R.same_bits(got[:n], want[:n]), (volume, skip, n, _differ(got[:n], want[:n]))
                assert (got[n] == -7.0).all(), (volume, n)
        _destroy(ren)


@pytest.mark.parametrize("kind", KINDS)
def test_a_permuted_list_gives_the_permuted_results_and_bad_records_leave_their_neighbours_alone(api, sc, torch_gpu, kind):
    torch = torch_gpu
    scene = Q.volume_scene(sc, "cloud")
    rays = Q.random_segments(scene)
    ren = _make(api, kind, scene, R.orbit_view(sc, 3))
    base = _list(torch, ren[0], rays)
    perm = np.random.default_rng(2).permutation(rays.shape[0])
    assert R.same_bits(_list(torch, ren[0], rays[perm]), base[perm])
    # degenerate records (NaN, inf, zero direction, empty ranges) spread through the list
    bad, what = Q.degenerate_records()
    mixed = rays.copy()
    at = np.arange(len(bad)) * 29 + 3
    mixed[at] = bad
    got = _list(torch, ren[0], mixed)
    assert not np.isnan(got).any()
    not_empty = [w for w, e in zip(what, Q.is_empty(got[at])) if not e]
    assert not not_empty, not_empty
    keep = np.ones(len(rays), bool)
    keep[at] = False
    assert R.same_bits(got[keep], base[keep])
    assert R.same_bits(got, api.test_ray_aov_host(scene, mixed))
    # no rays: no work, whatever the pointers
    assert ren[0].RayAov(torch.empty((0, 8), device="cuda")).shape == (0, 4)
    with pytest.raises(ValueError):
        ren[0].RayAov(torch.empty((4, 7), device="cuda"))
    with pytest.raises(ValueError):
        ren[0].RayAov(_dev(torch, rays).double())
    _destroy(ren)


# ---------------------------------------------------------------------------------------------------------------- 2. holdouts
@pytest.mark.parametrize("w,h", [(48, 32), (44, 36)], ids=["48x32", "ragged44x36"])
@pytest.mark.parametrize("kind", KINDS)
def test_holdouts_equal_the_host_restatement_and_the_list_call(api, sc, torch_gpu, kind, w, h):
    """blocks V3, V1 and the inside view (the sphere's far root) on one renderer, cloud V3 on another, held out to the sphere of radius
    0.2 |size|: ViewAovToDepth == the host's walk of nrc_camera_rays' records with t_max = depth == RayAov on those records; with and
    without the empty-space skip; depth +inf gives ViewAov()'s bits, depth <= 0 and NaN the empty result"""
    torch = torch_gpu
    for volume, names in (("blocks", ("blocks_v3", "blocks_v1", "blocks_inside")), ("cloud", ("cloud_v3",))):
        scene = Q.volume_scene(sc, volume)
        radius = 0.2 * Q.scene_diagonal(scene)
        views = {"blocks_v3": R.orbit_view(sc, 3, w / h), "blocks_v1": R.orbit_view(sc, 1, w / h), "cloud_v3": R.orbit_view(sc, 3, w / h),
                 "blocks_inside": R.inside_view(sc, R.blocks_volume(), scene["size"], w / h)}
        ren = _make(api, kind, scene, views[names[0]], w, h)
        for name in names:
            cam = views[name]
            ren[0].SetCamera(None, cam)
            rays = api.camera_rays(cam, w, h)
            depth = Q.sphere_depths(rays, radius, far=(name == "blocks_inside"))
            recs = Q.with_depth(rays, depth)
            want = api.test_ray_aov_host(scene, recs)
            whole = api.test_view_aov_host(scene, cam, w, h)
            assert (want[..., 1] > 0).sum() > 100 and (want[..., 1] < whole[..., 1]).sum() > 50, name      # (the sphere does hold out)
            for skip in (True, False):
                ren[0].SetEmptySkip(skip)
                got = ren[0].ViewAovToDepth(_dev(torch, depth)).cpu().numpy()
                assert R.same_bits(got, want), (name, skip, _differ(got, want))
            assert R.same_bits(_list(torch, ren[0], recs), want), name
            ren[0].SetEmptySkip(True)
            inf = ren[0].ViewAovToDepth(torch.full((h, w), float("inf"), device="cuda")).cpu().numpy()
            assert R.same_bits(inf, ren[0].ViewAov().cpu().numpy()) and R.same_bits(inf, whole), name
            odd = np.full((h, w), np.inf, np.float32)
            odd[::3, ::2], odd[1::3, 1::2], odd[2::3, ::5] = 0.0, -4.0, np.nan
            got = ren[0].ViewAovToDepth(_dev(torch, odd)).cpu().numpy()
            assert not np.isnan(got).any() and Q.is_empty(got[~np.isposinf(odd)]).all(), name
            assert R.same_bits(got[np.isposinf(odd)], whole[np.isposinf(odd)]), name
        with pytest.raises(ValueError):
            ren[0].ViewAovToDepth(torch.zeros((h, w + 1), device="cuda"))
        _destroy(ren)


@pytest.mark.parametrize("kind", KINDS)
def test_three_ranks_of_column_strips_make_the_whole_holdout(api, sc, torch_gpu, kind):
    from nrc_hpm_renderer_amd import parallel
    torch = torch_gpu
    scene = Q.volume_scene(sc, "blocks")
    cam = R.orbit_view(sc, 3, 72 / 32)
    rays = api.camera_rays(cam, 72, 32)
    depth = Q.sphere_depths(rays, 0.2 * Q.scene_diagonal(scene))
    want = api.test_ray_aov_host(scene, Q.with_depth(rays, depth))
    whole = _make(api, kind, scene, cam, 72, 32)
    assert R.same_bits(whole[0].ViewAovToDepth(_dev(torch, depth)).cpu().numpy(), want) and (want[..., 1] > 0).sum() > 100
    parts = []
    for rank in range(3):
        ren = _make(api, kind, scene, cam, 24, 32, tile=(rank, 3, 72, 32, 8))
        cols = [((rank + (lx >> 3) * 3) << 3) + (lx & 7) for lx in range(24)]
        parts.append(ren[0].ViewAovToDepth(_dev(torch, depth[:, cols])).cpu().numpy())
        _destroy(ren)
    assert R.same_bits(parallel.gather_columns(parts, 72, 8), want)
    _destroy(whole)


# ---------------------------------------------------------------------------------------------------------------- 3. orthographic views
@pytest.mark.parametrize("w,h", [(32, 32), (20, 12)], ids=["32x32", "ragged20x12"])
@pytest.mark.parametrize("kind", KINDS)
def test_light_views_equal_the_host_restatement_and_the_list_call(api, sc, torch_gpu, kind, w, h):
    """scene.light_view of the scene's light and of l ~ (0.4, -0.7, 0.59), both volumes, on a renderer of another size: OrthoAov == the
    host's walk of nrc_ortho_rays' records == RayAov on those records; the same bits without the empty-space skip"""
    torch = torch_gpu
    for volume in ("blocks", "cloud"):
        scene = Q.volume_scene(sc, volume)
        ren = _make(api, kind, scene, R.orbit_view(sc, 3))
        for light in (None, Q.OTHER_LIGHT):
            _, view, rays = Q.light_rays(api, sc, volume, light, w, h)
            want = api.test_ray_aov_host(scene, rays)
            assert (want[..., 1] > 0).sum() > (100 if w == 32 else 20), (volume, light)
            for skip in (True, False):
                ren[0].SetEmptySkip(skip)
                got = ren[0].OrthoAov(view, w, h).cpu().numpy()
                assert got.shape == (h, w, 4) and R.same_bits(got, want), (volume, light, skip, _differ(got, want))
            assert R.same_bits(_list(torch, ren[0], rays), want), (volume, light)
        with pytest.raises(ValueError):
            ren[0].OrthoAov(view, 0, 4)
        _destroy(ren)


# ---------------------------------------------------------------------------------------------------------------- 4. the current medium and view
@pytest.mark.parametrize("kind", KINDS)
def test_every_change_of_view_or_medium_is_seen_by_the_next_call(api, sc, torch_gpu, kind):
    """after SetCamera, SetVolume, SetVolumeTime (and SetVolumeBricks, SetSceneParams) the three calls equal the host restatement of the
    new state: nothing is kept from the call before"""
    torch = torch_gpu
    blk = R.blocks_volume()
    scene = Q.volume_scene(sc, "blocks")
    cam = R.orbit_view(sc, 3)
    ren = _make(api, kind, scene, cam)
    segs = Q.random_segments(scene)[:257]
    view = sc.light_view(scene, 20, 12, light_dir=Q.OTHER_LIGHT)
    ortho = api.ortho_rays(view, 20, 12)
    radius = 0.2 * Q.scene_diagonal(scene)
    seen = []

    def check(vol, camera, what):
        s = vol if isinstance(vol, dict) else sc.make_scene(vol, scene_id=4)
        rays = api.camera_rays(camera, R.W, R.H)
        depth = Q.sphere_depths(rays, radius)
        got = [_list(torch, ren[0], segs), ren[0].ViewAovToDepth(_dev(torch, depth)).cpu().numpy(), ren[0].OrthoAov(view, 20, 12).cpu().numpy()]
        want = [api.test_ray_aov_host(s, segs), api.test_ray_aov_host(s, Q.with_depth(rays, depth)), api.test_ray_aov_host(s, ortho)]
        for g, w_, name in zip(got, want, ("RayAov", "ViewAovToDepth", "OrthoAov")):
            assert R.same_bits(g, w_), (what, name, _differ(g, w_))
        state = np.concatenate([g.reshape(-1) for g in got])
        assert not any(R.same_bits(state, s_) for s_ in seen), what      # (a state none of the earlier ones: the comparison shows the change)
        seen.append(state)

    check(blk, cam, "creation")
    cam1 = R.orbit_view(sc, 1)
    ren[0].SetCamera(None, cam1)
    check(blk, cam1, "SetCamera")
    rolled = np.ascontiguousarray(np.roll(blk, (5, 3, -4), axis=(0, 1, 2)))
    ren[0].SetVolume(torch.from_numpy(rolled).cuda())
    check(rolled, cam1, "SetVolume")
    sparse = np.ascontiguousarray(np.roll(blk, (-7, 2, 6), axis=(0, 1, 2)))
    sparse[:, :, 8:16] = 0
    ren[0].SetVolumeBricks(*sc.volume_to_bricks(sparse))
    check(sparse, cam1, "SetVolumeBricks")
    keys = np.stack([blk, rolled, np.ascontiguousarray(blk[::-1])])
    ren[0].SetVolumeKeys(keys)
    for t in (0.37, 1.5):
        ren[0].SetVolumeTime(t)
        check(sc.volume_at(keys, t), cam1, "SetVolumeTime(%g)" % t)
    thin = dict(scene, density=sc.volume_at(keys, 1.5), density_factor=float(np.float32(scene["density_factor"] * 0.35)))
    ren[0].SetSceneParams(thin)
    check(thin, cam1, "SetSceneParams")
    _destroy(ren)


# ---------------------------------------------------------------------------------------------------------------- 5. paths
def _nrc_state(ren, nrc):
    return dict(image=ren.GetImage().cpu().numpy().copy(), loss=nrc.GetLoss(), step=nrc.GetStep(), params=[nrc.GetParams(k).copy() for k in range(4)])


@pytest.mark.parametrize("kind", KINDS)
def test_path_aovs_to_depths_equal_the_loop_and_leave_the_frames_alone(api, sc, torch_gpu, kind):
    """RenderPath over 4 cameras with aov_out and aov_depths == SetCamera + ViewAovToDepth per camera == the host restatement; frames, the
    returned images and (NRC, training) loss, step and weights are bitwise those of the same path without either; the depths are consumed
    with the target; depths for another number of views, or without a target, are refused"""
    import torch
    scene = Q.volume_scene(sc, "blocks")
    cams = [R.orbit_view(sc, k) for k in (3, 1, 6, 0)]
    fr = sc.frame_randoms(8, seed=5)
    train = kind == "nrc"
    radius = 0.2 * Q.scene_diagonal(scene)
    rays = [api.camera_rays(c, R.W, R.H) for c in cams]
    depths = np.stack([Q.sphere_depths(r, radius) for r in rays])
    d_depths = _dev(torch, depths)
    plain, held = _make(api, kind, scene, cams[0]), _make(api, kind, scene, cams[0])
    aovs = torch.full((4, R.H, R.W, 4), float("nan"), device="cuda")
    out_plain = plain[0].RenderPath(cams, 2, fr, train)
    out_held = held[0].RenderPath(cams, 2, fr, train, aov_out=aovs, aov_depths=d_depths)
    torch.cuda.synchronize()
    assert R.same_bits(out_plain.cpu().numpy(), out_held.cpu().numpy())
    assert R.same_bits(plain[0].GetImage().cpu().numpy(), held[0].GetImage().cpu().numpy())
    if train:
        a, b = _nrc_state(plain[0], plain[1]), _nrc_state(held[0], held[1])
        assert a["step"] == b["step"] and np.float32(a["loss"]).view(np.uint32) == np.float32(b["loss"]).view(np.uint32)
        for k in range(4):
            assert np.array_equal(a["params"][k].view(np.uint32), b["params"][k].view(np.uint32)), k
    got = aovs.cpu().numpy()
    for i, cam in enumerate(cams):
        plain[0].SetCamera(None, cam)
        assert R.same_bits(got[i], plain[0].ViewAovToDepth(d_depths[i]).cpu().numpy()), i
        assert R.same_bits(got[i], api.test_ray_aov_host(scene, Q.with_depth(rays[i], depths[i]))), i
    assert (got[..., 1] < np.stack([api.test_view_aov_host(scene, c, R.W, R.H) for c in cams])[..., 1]).sum() > 200      # (held out, not whole)
    # consumed: the next path with a target alone writes whole rays
    held[0].RenderPath(cams[:2], 1, fr[:2], False, out=False, aov_out=aovs[:2])
    torch.cuda.synchronize()
    for i in range(2):
        assert R.same_bits(aovs[i].cpu().numpy(), api.test_view_aov_host(scene, cams[i], R.W, R.H)), i
    # depths of another number of views: refused, nothing enqueued, target and depths gone
    aovs.fill_(7.0)
    held[0].SetPathAovTarget(aovs[:3])
    held[0].SetPathAovDepths(d_depths[:2])
    before = held[0].GetImage().cpu().numpy().copy()
    with pytest.raises(RuntimeError, match="AOV depths"):
        held[0].RenderPath(cams[:3], 1, fr[:3], False, out=False)
    held[0].RenderPath(cams[:3], 1, fr[:3], False, out=False)
    torch.cuda.synchronize()
    assert (aovs.cpu().numpy() == 7.0).all()
    # depths without a target: refused
    held[0].SetPathAovDepths(d_depths[:3])
    with pytest.raises(RuntimeError, match="without an AOV target"):
        held[0].RenderPath(cams[:3], 1, fr[:3], False, out=False)
    with pytest.raises(ValueError):
        held[0].RenderPath(cams, 1, fr[:4], False, aov_depths=d_depths)
    with pytest.raises(ValueError):
        held[0].RenderPath(cams, 1, fr[:4], False, aov_out=aovs, aov_depths=d_depths[:3])
    del before
    _destroy(plain, held)


# ---------------------------------------------------------------------------------------------------------------- 6. the command line
def test_cli_writes_the_shadow_map_and_the_held_out_aov(api, sc, torch_gpu, tmp_path):
    """--shadow-map: FLOAT channels A, Z, Zhalf, tau of scene.light_view; --aov --holdout-sphere: the export's AOV channels are the camera
    rays' walk up to the analytic sphere, for the single view and for every view of an orbit -- each against the host restatement"""
    from nrc_hpm_renderer_amd import cli, io_exr
    w, h, n, radius = 64, 48, 24, 15.0
    scene = sc.make_scene(sc.quantize_density(sc.fbm_cloud_volume(32, seed=1337)), scene_id=api.AppConfig(["NRC-HPM-Renderer"] + cli.DEFAULT_ARGV).scene_id)
    common = ["--frames", "2", "--width", str(w), "--height", str(h), "--volume", "32", "--output", str(tmp_path / "output"), "--aov",
              "--holdout-sphere", str(radius)]

    def held_out(cam):
        rays = api.camera_rays(cam, w, h)
        return api.test_ray_aov_host(scene, Q.with_depth(rays, cli.sphere_depth(rays, radius))), api.test_view_aov_host(scene, cam, w, h)

    def check_file(path, want):
        planes = io_exr.read_exr_channels(path)
        assert sorted(planes) == ["A", "B", "G", "R", "Z", "Zhalf", "tau"]
        for name, i in (("A", 0), ("tau", 1), ("Z", 2), ("Zhalf", 3)):
            assert R.same_bits(planes[name], want[..., i]), (path, name)

    exr, shadow = str(tmp_path / "final.exr"), str(tmp_path / "shadow.exr")
    assert cli.main(common + ["--export", exr, "--shadow-map", shadow, "--shadow-size", str(n)]) == 0
    want, whole = held_out(sc.make_camera(aspect=w / h))
    assert (want[..., 1] > 0).sum() > 100 and (want[..., 1] < whole[..., 1]).sum() > 100      # (the cloud is seen, and the sphere holds out)
    check_file(exr, want)
    planes = io_exr.read_exr_channels(shadow)
    assert sorted(planes) == ["A", "Z", "Zhalf", "tau"]
    light = api.test_ray_aov_host(scene, api.ortho_rays(sc.light_view(scene, n, n), n, n))
    assert (light[..., 1] > 0).sum() > 50
    for name, i in (("A", 0), ("tau", 1), ("Z", 2), ("Zhalf", 3)):
        assert R.same_bits(planes[name], light[..., i]), name
    assert cli.main(common + ["--orbit", "2", "--export", str(tmp_path / "view_%04d.exr")]) == 0
    for i, cam in enumerate(sc.orbit_cameras(2, 64.0, 0.0, aspect=w / h)):
        check_file(str(tmp_path / ("view_%04d.exr" % i)), held_out(cam)[0])
