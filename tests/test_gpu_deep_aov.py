"""The deep AOV on the GPU (include/nrc_hpm.h "Deep AOV"; k_ray_aov<RayList | ViewDepth | OrthoView, DeepOut>): every plane and the flat result
equal, bit for bit, the host restatement nrc_test_deep_ray_aov_host -- the plain deep range walk of csrc/nrc_view_aov.hpp, which
tests/test_deep_aov_cpu.py pins to an fp64 reference -- although the kernel jumps out of empty cells by the occupancy bits, keeps its levels
in LDS, stores a depth when it is crossed and, for the camera's rays, skips tiles by the empty-space mask.  Every ray, every plane, no
exclusions."""
import json

import numpy as np
import pytest

import deep_aov_reference as D
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


def _list(torch, ren, rays, levels):
    """DeepRayAov of records [...][8] as numpy (planes [K][...], flat [...][4])"""
    recs = np.ascontiguousarray(rays, np.float32)
    z, flat = ren.DeepRayAov(_dev(torch, recs.reshape(-1, 8)), levels, flat=True)
    return z.cpu().numpy().reshape((len(levels),) + recs.shape[:-1]), flat.cpu().numpy().reshape(recs.shape[:-1] + (4,))


def _np(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def _same(got, want):
    return R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1])


# ---------------------------------------------------------------------------------------------------------------- 1. lists
@pytest.mark.parametrize("kind", KINDS)
def test_lists_equal_the_host_restatement_at_every_tail_and_level_set(api, sc, torch_gpu, kind):
    """the random segments of the blocks, dense-blocks and cloud volumes, the first n = 1, 63, 64, 65, 257, 1024 of them, every level set:
    lane tails, a full wave, a workgroup's tail; the same bits without the empty-space skip; nothing is written behind a plane's end or the
    flat list's end; without `flat` the planes are the same"""
    torch = torch_gpu
    for volume in ("blocks", "dense", "cloud"):
        scene = D.volume_scene(sc, volume)
        rays = Q.random_segments(scene)
        ren = _make(api, kind, scene, R.orbit_view(sc, 3))
        d_rays = _dev(torch, rays)
        for lname, levels in D.level_sets(sc).items():
            K = levels.size
            for skip in (True, False):
                ren[0].SetEmptySkip(skip)
                for n in (1, 63, 64, 65, 257, 1024):
                    want = api.deep_ray_aov_host(scene, rays[:n], levels)
                    z = torch.full((K * n + 1,), -7.0, device="cuda")
                    flat = torch.full((n + 1, 4), -7.0, device="cuda")
                    ren[0].DeepRayAov(d_rays[:n], levels, out=z[:K * n].view(K, n), flat=flat[:n])
                    gz, gf = z.cpu().numpy(), flat.cpu().numpy()
                    assert _same((gz[:K * n].reshape(K, n), gf[:n]), want), (volume, lname, skip, n)
                    assert gz[K * n] == -7.0 and (gf[n] == -7.0).all(), (volume, lname, n)
            assert R.same_bits(ren[0].DeepRayAov(d_rays, levels).cpu().numpy(), api.deep_ray_aov_host(scene, rays, levels)[0]), (volume, lname)
        _destroy(ren)


@pytest.mark.parametrize("kind", KINDS)
def test_one_level_at_ln2_is_todays_kernels_z_half(api, sc, torch_gpu, kind):
    """against the kernels that exist without the deep AOV: K = 1, {NRC_AOV_LN2} -- the plane is z_half of RayAov / ViewAov / ViewAovToDepth /
    OrthoAov and the flat result is their output, bit for bit"""
    torch = torch_gpu
    ln2 = D.level_sets(sc)["ln2"]
    for volume in ("blocks", "cloud"):
        scene = Q.volume_scene(sc, volume)
        cam = R.orbit_view(sc, 3)
        ren = _make(api, kind, scene, cam)
        d_rays = _dev(torch, Q.random_segments(scene))
        old = ren[0].RayAov(d_rays).cpu().numpy()
        z, flat = _np(ren[0].DeepRayAov(d_rays, ln2, flat=True))
        assert R.same_bits(z[0], old[:, 3]) and R.same_bits(flat, old) and np.isfinite(z[0]).sum() > 50, volume
        old = ren[0].ViewAov().cpu().numpy()
        z, flat = _np(ren[0].DeepViewAov(ln2, flat=True))
        assert R.same_bits(z[0], old[..., 3]) and R.same_bits(flat, old) and np.isfinite(z[0]).sum() > 50, volume
        depth = _dev(torch, Q.sphere_depths(api.camera_rays(cam, R.W, R.H), 0.2 * Q.scene_diagonal(scene)))
        old = ren[0].ViewAovToDepth(depth).cpu().numpy()
        z, flat = _np(ren[0].DeepViewAov(ln2, depth=depth, flat=True))
        assert R.same_bits(z[0], old[..., 3]) and R.same_bits(flat, old), volume
        view = sc.light_view(scene, 32, 32)
        old = ren[0].OrthoAov(view, 32, 32).cpu().numpy()
        z, flat = _np(ren[0].DeepOrthoAov(view, 32, 32, ln2, flat=True))
        assert R.same_bits(z[0], old[..., 3]) and R.same_bits(flat, old) and np.isfinite(z[0]).sum() > 50, volume
        _destroy(ren)


@pytest.mark.parametrize("kind", KINDS)
def test_bad_records_leave_their_neighbours_alone_and_bad_arguments_are_refused(api, sc, torch_gpu, kind):
    torch = torch_gpu
    scene = Q.volume_scene(sc, "cloud")
    rays = Q.random_segments(scene)
    levels = D.level_sets(sc)["k7"]
    ren = _make(api, kind, scene, R.orbit_view(sc, 3))
    bad, _ = Q.degenerate_records()
    mixed = rays.copy()
    at = np.arange(len(bad)) * 29 + 3
    mixed[at] = bad
    got = _list(torch, ren[0], mixed, levels)
    assert _same(got, api.deep_ray_aov_host(scene, mixed, levels))
    assert np.isposinf(got[0][:, at]).all() and Q.is_empty(got[1][at]).all() and not np.isnan(got[0]).any()
    keep = np.ones(len(rays), bool)
    keep[at] = False
    base = _list(torch, ren[0], rays, levels)
    assert R.same_bits(got[0][:, keep], base[0][:, keep]) and R.same_bits(got[1][keep], base[1][keep])
    # no rays: no work; the validation list: refused before anything is enqueued (the planes keep their fill)
    assert ren[0].DeepRayAov(torch.empty((0, 8), device="cuda"), levels).shape == (7, 0)
    d_rays = _dev(torch, rays[:65])
    z = torch.full((3, 65), -7.0, device="cuda")
    for bad_levels in ([1.0, 1.0, 2.0], [2.0, 1.0, 3.0], [0.0, 1.0, 2.0], [-1.0, 1.0, 2.0], [1.0, 2.0, np.inf], [1.0, np.nan, 2.0]):
        with pytest.raises(RuntimeError, match="deep AOV"):
            ren[0].DeepRayAov(d_rays, bad_levels, out=z)
        with pytest.raises(RuntimeError, match="deep AOV"):
            ren[0].DeepViewAov(bad_levels)
        with pytest.raises(RuntimeError, match="deep AOV"):
            ren[0].DeepOrthoAov(sc.light_view(scene, 8, 8), 8, 8, bad_levels)
    torch.cuda.synchronize()
    assert (z.cpu().numpy() == -7.0).all()
    for n_levels in (0, 33):
        with pytest.raises(ValueError):
            ren[0].DeepRayAov(d_rays, np.linspace(0.1, 3.0, n_levels))
    lv = np.array([1.0], np.float32)
    fn = ren[0]._medium("deep_ray_aov")
    assert fn(ren[0].h, 65, d_rays.data_ptr(), 0, lv.ctypes.data, z.data_ptr(), None) == -1
    assert fn(ren[0].h, 65, d_rays.data_ptr(), 33, lv.ctypes.data, z.data_ptr(), None) == -1
    assert fn(ren[0].h, 65, d_rays.data_ptr(), 1, None, z.data_ptr(), None) == -1
    assert fn(ren[0].h, 65, d_rays.data_ptr(), 1, lv.ctypes.data, None, None) == -1
    assert fn(ren[0].h, 65, None, 1, lv.ctypes.data, z.data_ptr(), None) == -1
    assert fn(ren[0].h, 0, None, 1, lv.ctypes.data, z.data_ptr(), None) == 0
    with pytest.raises(ValueError):
        ren[0].DeepRayAov(torch.empty((4, 7), device="cuda"), levels)
    with pytest.raises(ValueError):
        ren[0].DeepViewAov(levels, depth=torch.zeros((R.H, R.W + 1), device="cuda"))
    _destroy(ren)


# ---------------------------------------------------------------------------------------------------------------- 2. the camera's rays
@pytest.mark.parametrize("w,h", [(48, 32), (44, 36)], ids=["48x32", "ragged44x36"])
@pytest.mark.parametrize("kind", KINDS)
def test_views_equal_the_host_restatement_and_the_list_call(api, sc, torch_gpu, kind, w, h):
    """blocks V3, V1 and the inside view on one renderer, cloud V3 on another, whole rays and held out to the sphere of radius 0.2 |size|,
    every level set: DeepViewAov == the host's walk of nrc_camera_rays' records (t_max = depth) == DeepRayAov on those records, with and
    without the empty-space skip."""
    torch = torch_gpu
    sets = D.level_sets(sc)
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
            for lname, levels in sets.items():
                for recs, d_depth in ((rays, None), (Q.with_depth(rays, depth), _dev(torch, depth))):
                    want = api.deep_ray_aov_host(scene, recs, levels)
                    assert np.isfinite(want[0][0]).sum() > 50, (name, lname)
                    got = {}
                    for skip in (True, False):
                        ren[0].SetEmptySkip(skip)
                        got[skip] = _np(ren[0].DeepViewAov(levels, depth=d_depth, flat=True))
                        assert got[skip][0].shape == (levels.size, h, w) and _same(got[skip], want), (name, lname, skip, d_depth is None)
                    if lname in ("k7", "k32"):
                        assert _same(_list(torch, ren[0], recs, levels), want), (name, lname)
        _destroy(ren)


@pytest.mark.parametrize("kind", KINDS)
def test_no_depth_image_is_a_depth_image_of_inf(api, sc, torch_gpu, kind):
    """the view source's null depth at 48 x 32, blocks V3 and the inside view, every level set: DeepViewAov without a depth image returns
    ViewAov()'s bits as its flat result and, plane for plane, what it returns with a depth image of +inf"""
    torch = torch_gpu
    scene = Q.volume_scene(sc, "blocks")
    views = (R.orbit_view(sc, 3), R.inside_view(sc, R.blocks_volume(), scene["size"]))
    ren = _make(api, kind, scene, views[0])
    inf = torch.full((R.H, R.W), float("inf"), device="cuda")
    for i, cam in enumerate(views):
        ren[0].SetCamera(None, cam)
        whole = ren[0].ViewAov().cpu().numpy()
        for lname, levels in D.level_sets(sc).items():
            none = _np(ren[0].DeepViewAov(levels, depth=None, flat=True))
            assert R.same_bits(none[1], whole) and _same(none, _np(ren[0].DeepViewAov(levels, depth=inf, flat=True))), (i, lname)
            assert np.isfinite(none[0][0]).sum() > 50, (i, lname)
    _destroy(ren)


@pytest.mark.parametrize("kind", KINDS)
def test_pixels_of_rejected_tiles_hold_inf_in_every_plane_as_with_the_skip_off(api, sc, torch_gpu, kind):
    """a far view on 96 x 64 (test_gpu_view_aov.py: at radius 70 the boxes of this small volume reach into every tile of a 48 x 32 frame): the
    mask rejects some tiles and not all; their pixels hold +inf in all K planes and the empty flat result -- the bits they hold with the
    skip off, where their rays are walked -- whole rays and held out, K = 7 and K = 32"""
    torch = torch_gpu
    scene = Q.volume_scene(sc, "blocks")
    w, h = 96, 64
    cam = sc.orbit_cameras(8, radius=200.0, height=40.0, aspect=w / h)[3]
    ren = _make(api, kind, scene, cam, w, h)
    rays = api.camera_rays(cam, w, h)
    depth = Q.sphere_depths(rays, 0.2 * Q.scene_diagonal(scene))
    for lname in ("k7", "k32"):
        levels = D.level_sets(sc)[lname]
        for recs, d_depth in ((rays, None), (Q.with_depth(rays, depth), _dev(torch, depth))):
            ren[0].SetEmptySkip(True)
            with_mask = _np(ren[0].DeepViewAov(levels, depth=d_depth, flat=True))
            mask = ren[0].TileMask()
            tx, ty = w // 8, h // 8
            assert mask.size == (tx * ty + 31) // 32 + 1 and mask[-1] == 0
            bits = np.array([(int(mask[t >> 5]) >> (t & 31)) & 1 for t in range(tx * ty)], bool).reshape(ty, tx)
            assert 0 < (~bits).sum() < tx * ty
            rej = np.repeat(np.repeat(~bits, 8, axis=0), 8, axis=1)
            assert np.isposinf(with_mask[0][:, rej]).all() and Q.is_empty(with_mask[1][rej]).all()
            ren[0].SetEmptySkip(False)
            without = _np(ren[0].DeepViewAov(levels, depth=d_depth, flat=True))
            assert ren[0].TileMask().size == 0
            assert _same(with_mask, without) and _same(without, api.deep_ray_aov_host(scene, recs, levels))
            assert np.isfinite(without[0][0]).sum() > 20      # (the far view's cloud covers a few hundred pixels)
    _destroy(ren)


@pytest.mark.parametrize("kind", KINDS)
def test_three_ranks_of_column_strips_make_the_whole_images_planes(api, sc, torch_gpu, kind):
    from nrc_hpm_renderer_amd import parallel
    torch = torch_gpu
    scene = Q.volume_scene(sc, "blocks")
    levels = D.level_sets(sc)["k7"]
    cam = R.orbit_view(sc, 3, 72 / 32)
    rays = api.camera_rays(cam, 72, 32)
    depth = Q.sphere_depths(rays, 0.2 * Q.scene_diagonal(scene))
    for recs, dep in ((rays, None), (Q.with_depth(rays, depth), depth)):
        want = api.deep_ray_aov_host(scene, recs, levels)
        assert np.isfinite(want[0][0]).sum() > 100
        parts_z, parts_f = [], []
        for rank in range(3):
            ren = _make(api, kind, scene, cam, 24, 32, tile=(rank, 3, 72, 32, 8))
            cols = [((rank + (lx >> 3) * 3) << 3) + (lx & 7) for lx in range(24)]
            z, flat = _np(ren[0].DeepViewAov(levels, depth=None if dep is None else _dev(torch, dep[:, cols]), flat=True))
            parts_z.append(np.ascontiguousarray(np.moveaxis(z, 0, -1)))      # [h][lw][K]: columns gather like channels
            parts_f.append(flat)
            _destroy(ren)
        whole_z = np.moveaxis(parallel.gather_columns(parts_z, 72, 8), -1, 0)
        assert R.same_bits(whole_z, want[0]) and R.same_bits(parallel.gather_columns(parts_f, 72, 8), want[1])


# ---------------------------------------------------------------------------------------------------------------- 3. orthographic views
@pytest.mark.parametrize("w,h", [(32, 32), (20, 12)], ids=["32x32", "ragged20x12"])
@pytest.mark.parametrize("kind", KINDS)
def test_light_views_equal_the_host_restatement_and_the_list_call(api, sc, torch_gpu, kind, w, h):
    """scene.light_view of the scene's light and of l ~ (0.4, -0.7, 0.59), both volumes, every level set, on a renderer of another size:
    DeepOrthoAov == the host's walk of nrc_ortho_rays' records == DeepRayAov on those records; the same bits without the skip"""
    torch = torch_gpu
    for volume in ("blocks", "cloud"):
        scene = Q.volume_scene(sc, volume)
        ren = _make(api, kind, scene, R.orbit_view(sc, 3))
        for light in (None, Q.OTHER_LIGHT):
            _, view, rays = Q.light_rays(api, sc, volume, light, w, h)
            for lname, levels in D.level_sets(sc).items():
                want = api.deep_ray_aov_host(scene, rays, levels)
                assert np.isfinite(want[0][0]).sum() > (50 if w == 32 else 10), (volume, light, lname)
                for skip in (True, False):
                    ren[0].SetEmptySkip(skip)
                    got = _np(ren[0].DeepOrthoAov(view, w, h, levels, flat=True))
                    assert got[0].shape == (levels.size, h, w) and _same(got, want), (volume, light, lname, skip)
                if lname == "k7":
                    assert _same(_list(torch, ren[0], rays, levels), want), (volume, light)
        with pytest.raises(ValueError):
            ren[0].DeepOrthoAov(view, 0, 4, [1.0])
        _destroy(ren)


# ---------------------------------------------------------------------------------------------------------------- 4. the current medium and view
@pytest.mark.parametrize("kind", KINDS)
def test_every_change_of_view_or_medium_is_seen_by_the_next_call(api, sc, torch_gpu, kind):
    """after SetCamera, SetVolume, SetVolumeBricks, SetVolumeTime and SetSceneParams the three calls equal the host restatement of the new
    state: nothing is kept from the call before"""
    torch = torch_gpu
    blk = R.blocks_volume()
    scene = Q.volume_scene(sc, "blocks")
    levels = D.level_sets(sc)["k7"]
    cam = R.orbit_view(sc, 3)
    ren = _make(api, kind, scene, cam)
    segs = Q.random_segments(scene)[:257]
    view = sc.light_view(scene, 20, 12, light_dir=Q.OTHER_LIGHT)
    ortho = api.ortho_rays(view, 20, 12)
    seen = []

    def check(vol, camera, what):
        s = vol if isinstance(vol, dict) else sc.make_scene(vol, scene_id=4)
        rays = api.camera_rays(camera, R.W, R.H)
        got = [_list(torch, ren[0], segs, levels), _np(ren[0].DeepViewAov(levels, flat=True)), _np(ren[0].DeepOrthoAov(view, 20, 12, levels, flat=True))]
        want = [api.deep_ray_aov_host(s, segs, levels), api.deep_ray_aov_host(s, rays, levels), api.deep_ray_aov_host(s, ortho, levels)]
        for g, w_, name in zip(got, want, ("DeepRayAov", "DeepViewAov", "DeepOrthoAov")):
            assert _same(g, w_), (what, name)
        state = np.concatenate([g[0].reshape(-1) for g in got])
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


def _state(ren, nrc):
    out = dict(image=ren.GetImage().cpu().numpy().copy())
    if nrc is not None:
        out.update(loss=np.float32(nrc.GetLoss(wait=True)), step=nrc.GetStep(), params=[nrc.GetParams(k).copy() for k in range(4)])
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_frames_and_weights_are_untouched_by_the_deep_calls(api, sc, torch_gpu, kind):
    """render, call the three deep AOVs, render again: the framebuffer and (NRC) loss, step and weights of a renderer that never made the
    calls, bitwise"""
    torch = torch_gpu
    scene = Q.volume_scene(sc, "blocks")
    levels = D.level_sets(sc)["k32"]
    cam = R.orbit_view(sc, 3)
    fr = sc.frame_randoms(4, seed=5)
    plain, deep = _make(api, kind, scene, cam), _make(api, kind, scene, cam)
    d_rays = _dev(torch, Q.random_segments(scene))
    for i in range(4):
        for ren in (plain, deep):
            ren[0].SetFrameRandom(fr[i])
            if kind == "mc":
                ren[0].Render()
            else:
                ren[0].Render(None, True)
        if i in (0, 2):
            deep[0].DeepRayAov(d_rays, levels, flat=True)
            deep[0].DeepViewAov(levels, flat=True)
            deep[0].DeepOrthoAov(sc.light_view(scene, 20, 12), 20, 12, levels)
    torch.cuda.synchronize()
    a, b = _state(*plain), _state(*deep)
    assert R.same_bits(a["image"], b["image"]) and np.isfinite(a["image"]).all() and (a["image"][..., :3] > 0).any()
    if kind == "nrc":
        assert a["step"] == b["step"] and a["loss"].view(np.uint32) == b["loss"].view(np.uint32)
        for k in range(4):
            assert np.array_equal(a["params"][k].view(np.uint32), b["params"][k].view(np.uint32)), k
    _destroy(plain, deep)


GUARD_CHILD = """
import sys
import numpy as np
import torch
sys.path[:0] = [%r, %r]
from nrc_hpm_renderer_amd import api, scene as sc
import deep_aov_reference as D, ray_aov_reference as Q, view_aov_reference as R
L = api.load_library()
scene = D.volume_scene(sc, "dense")
levels = D.level_sets(sc)["k32"]
ren = api.McHpmRenderer(R.W, R.H, 8, False, R.orbit_view(sc, 3), scene)
assert L.nrc_debug_check_guards(None, 0) == 0, "guard mode is off, or damage before the call"
rays = Q.random_segments(scene)[:65]
z = torch.full((32 * 65 + 64,), -7.0, device="cuda")
flat = torch.full((66, 4), -7.0, device="cuda")
ren.DeepRayAov(torch.from_numpy(np.array(rays)).cuda(), levels, out=z[:32 * 65].view(32, 65), flat=flat[:65])
got, gf = z.cpu().numpy(), flat.cpu().numpy()
want = api.deep_ray_aov_host(scene, rays, levels)
assert (got[32 * 65:] == -7.0).all() and (gf[65] == -7.0).all()
assert R.same_bits(got[:32 * 65].reshape(32, 65), want[0]) and R.same_bits(gf[:65], want[1])
print("guards", L.nrc_debug_check_guards(None, 0))
ren.Destroy()
"""


def test_a_32_level_store_at_n_65_stays_inside_its_buffers(torch_gpu):
    """a fresh process under NRC_DEBUG=guard_alloc: after a [32][65] store (and the [65][4] flat one) nrc_debug_check_guards is clean, the
    fill behind the planes and behind the flat list is untouched, and the planes are the host restatement's"""
    import os
    import subprocess
    import sys
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", GUARD_CHILD % (os.path.dirname(tests), tests)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, NRC_DEBUG="guard_alloc"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "guards 0" in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---------------------------------------------------------------------------------------------------------------- 5. the command line
def test_cli_writes_the_deep_channels_and_the_levels(api, sc, torch_gpu, tmp_path):
    """--aov --deep 4 and --shadow-map --deep 4: the Zd* channels are the host restatement's planes, the other channels what they are without
    --deep, and the sidecar's levels are scene.deep_levels'"""
    from nrc_hpm_renderer_amd import cli, io_exr
    w, h, n = 64, 48, 24
    scene = sc.make_scene(sc.quantize_density(sc.fbm_cloud_volume(32, seed=1337)), scene_id=api.AppConfig(["NRC-HPM-Renderer"] + cli.DEFAULT_ARGV).scene_id)
    exr, shadow = str(tmp_path / "final.exr"), str(tmp_path / "shadow.exr")
    assert cli.main(["--frames", "2", "--width", str(w), "--height", str(h), "--volume", "32", "--output", str(tmp_path / "output"), "--aov",
                     "--deep", "4", "--export", exr, "--shadow-map", shadow, "--shadow-size", str(n)]) == 0
    levels = sc.deep_levels(4, cli.DEEP_TAU_MAX)
    names = ["Zd00", "Zd01", "Zd02", "Zd03"]
    for path, rays, flat_names in ((exr, api.camera_rays(sc.make_camera(aspect=w / h), w, h), ["A", "B", "G", "R", "Z", "Zhalf", "tau"]),
                                   (shadow, api.ortho_rays(sc.light_view(scene, n, n), n, n), ["A", "Z", "Zhalf", "tau"])):
        side = json.load(open(path[:-4] + ".json"))
        assert side["channels"] == names and R.same_bits(np.array(side["levels"], np.float32), levels)
        planes = io_exr.read_exr_channels(path)
        assert sorted(planes) == sorted(flat_names + names)
        z, flat = api.deep_ray_aov_host(scene, rays, levels)
        assert np.isfinite(z[0]).sum() > 50
        for k, name in enumerate(names):
            assert R.same_bits(planes[name], z[k]), (path, name)
        for name, i in (("A", 0), ("tau", 1), ("Z", 2), ("Zhalf", 3)):
            assert R.same_bits(planes[name], flat[..., i]), (path, name)
