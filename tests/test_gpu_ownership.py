"""Every device allocation the library makes belongs to an owning member (csrc/nrc_owned.hpp: DevBuf, Owned), so an object's whole life --
and a creation that fails half-way -- returns what it took.  api.live_allocations() (nrc_debug_live_allocations) counts what dev_alloc has
handed out and dev_free has not taken back; every test reads it first and compares at the end."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, N_VOX = 64, 32, 32
CFG = dict(train_batch_count=2, log2_train_batch_size=9, log2_infer_batch_size=14)
MODELS = {
    "default-6x64": dict(),
    "hashgrid": dict(pos_id=0, hashgrid_log2_size=14),
    "2x128-enc80": dict(nn_width=128, nn_depth=2, pos_id=3, dir_id=0),
    "long-paths-self-train": dict(compat_fix=2, train_ray_length=32, self_train=1),      # trace streams and staging sets
}


@pytest.fixture(scope="module")
def world(api, sc, torch_gpu):
    """the scene, the camera and two key volumes; and one MC frame rendered and thrown away, so that what the process allocates once per
    device and keeps (the free-flight table of the empty-space skip) exists before any test reads its baseline"""
    vol = sc.quantize_density(sc.sphere_volume(N_VOX))
    scene = sc.make_scene(vol, scene_id=4)
    cam = sc.make_camera(aspect=W / H)
    keys = np.ascontiguousarray(np.stack([vol, np.ascontiguousarray(np.roll(vol, 5, axis=2))]))
    mc = api.McHpmRenderer(W, H, 8, False, cam, scene)
    mc.Render()
    mc.Destroy()
    torch_gpu.cuda.synchronize()
    return dict(vol=vol, scene=scene, cam=cam, keys=keys)


def _randoms(n, seed):
    return np.random.default_rng(seed).random((n, 4), dtype=np.float32)


def test_a_failed_creation_returns_what_it_took(api, world, torch_gpu):
    """self_train = 2 is refused by the renderer's constructor AFTER it has allocated its frame images and train-ray buffers: all of them
    come back, and the cache it was given goes on to serve a renderer"""
    base = api.live_allocations()
    cfg = api.AppConfig(self_train=1, **CFG)
    nrc = api.NeuralRadianceCache(cfg)
    with_cache = api.live_allocations()
    assert with_cache > base
    with pytest.raises(RuntimeError, match="must be 0 or 1"):
        api.NrcHpmRenderer(W, H, False, world["cam"], api.AppConfig(self_train=2, **CFG), world["scene"], nrc)
    assert api.live_allocations() == with_cache
    ren = api.NrcHpmRenderer(W, H, False, world["cam"], cfg, world["scene"], nrc)
    assert api.live_allocations() > with_cache
    ren.RenderFrames(_randoms(2, 1), train=True)
    assert np.isfinite(ren.GetImage().cpu().numpy()).all()
    ren.Destroy()
    nrc.Destroy()
    assert api.live_allocations() == base


@pytest.mark.parametrize("model", list(MODELS))
def test_a_whole_life_cycle_returns_everything(api, sc, world, torch_gpu, model):
    """cache + NRC renderer + MC renderer through everything that allocates on first use or regrows: trained frames, the three volume
    setters (slots, scratch, staging, brick index, keys), a camera path (rectangles), the gather, the stand-alone training workspace
    and feature buffers beyond what the frames had sized"""
    torch = torch_gpu
    base = api.live_allocations()
    cfg = api.AppConfig(**dict(CFG, **MODELS[model]))
    nrc = api.NeuralRadianceCache(cfg)
    ren = api.NrcHpmRenderer(W, H, False, world["cam"], cfg, world["scene"], nrc)
    mc = api.McHpmRenderer(W, H, 8, False, world["cam"], world["scene"])
    ren.RenderFrames(_randoms(8, 2), train=True)
    mc.Render()
    vol, keys = world["vol"], world["keys"]
    origins, bricks = sc.volume_to_bricks(vol)
    views = sc.orbit_cameras(2, aspect=W / H)
    for r in (ren, mc):
        r.SetVolume(vol)
        r.SetVolumeBricks(origins, bricks)
        r.SetVolumeKeys(keys)
        r.SetVolumeTime(0.5)
    out = ren.RenderPath(views, 1, _randoms(2, 3), True)
    assert tuple(out.shape) == (2, H, W, 4)
    assert tuple(mc.RenderPath(views, 1, _randoms(2, 4)).shape) == (2, H, W, 4)
    assert tuple(ren.GatherFrame().shape) == (H, W, 4)
    ren.TileMask()
    mc.TileMask()
    rng = np.random.default_rng(5)

    def backward(n):
        x = torch.from_numpy(rng.random((n, 5), dtype=np.float32)).cuda()
        t = torch.from_numpy(rng.random((n, 3), dtype=np.float32)).cuda()
        nrc.Backward(x, t)

    def infer(n):
        x = torch.from_numpy(rng.random((n, 5), dtype=np.float32)).cuda()
        y = torch.empty((n, 3), device="cuda")
        nrc.Infer(x, y, useEma=True)
        torch.cuda.synchronize()
        assert np.isfinite(y.cpu().numpy()).all()

    backward(64)
    backward(256)
    infer(512)
    infer(2048)
    if model == "hashgrid":
        assert nrc.GridGradPack()[0] > 0
    # the frames' batches hold 512 samples and their inference covers 2 048 queries: these two regrow whatever came before
    backward(1024)
    infer(4096)
    assert api.live_allocations() > base
    mc.Destroy()
    ren.Destroy()
    nrc.Destroy()
    assert api.live_allocations() == base
