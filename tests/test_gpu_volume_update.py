"""nrc_renderer_set_volume / nrc_mc_renderer_set_volume: a live renderer's density volume replaced on the device (animated media).
The device rebuild (density, occupancy bits, empty-space boxes) equals what renderer creation builds on the host, bit for bit; frames
after a swap equal the oracle's / a fresh renderer's frames of the new volume; swaps inside the pipelined frame graph are ordered."""
import ctypes as C
import time

import numpy as np
import pytest

from conftest import FRAME_RANDOM, nrc_debug
from volume_common import _make, _sparse_512, _to_f32, assert_same_volume, same_bits, volume_buffers

pytestmark = pytest.mark.gpu


def _single_voxels(n=24):
    vols = []
    for p in (7, 8, 15, 16):
        for pos in ((p, p, p), (p, 3, 20), (11, p, 7), (8, 16, p), (p, 23 - p % 8, 15)):
            v = np.zeros((n, n, n), np.uint8)
            x, y, z = pos
            v[z, y, x] = 200
            vols.append(("voxel%d_%d_%d" % pos, v))
    return vols


def _volumes(cloud16):
    rng = np.random.default_rng(7)
    odd = (rng.random((29, 7, 13)) < 0.02).astype(np.uint8) * rng.integers(1, 256, (29, 7, 13)).astype(np.uint8)
    return [("zeros", np.zeros_like(cloud16)), ("full", np.full_like(cloud16, 255)), ("cloud16", cloud16),
            ("cloud16_rolled", np.ascontiguousarray(np.roll(cloud16, (17, -9, 40), axis=(0, 1, 2)))), ("odd13x7x29", odd)] + _single_voxels()


def _as_source(vol, source):
    import torch
    if source == "u8_host":
        return np.ascontiguousarray(vol)
    if source == "u8_device":
        return torch.from_numpy(np.ascontiguousarray(vol)).cuda()
    # (k + 0.5) / 255 quantises back to k (k = 255: above 1 -> 255)
    return torch.from_numpy((vol.astype(np.float32) + np.float32(0.5)) / np.float32(255.0)).cuda()


# device allocations a renderer's first SetVolume makes: four buffers per slot (density, occupancy bits, boxes, box count) and the rebuild
# scratch, two slots for NRC and one for MC.  Counted with live_allocations() at commit f36b916, before the slot choice moved.
FIRST_SWAP_ALLOCATIONS = {"nrc": 9, "mc": 5}


@pytest.mark.parametrize("kind", ["nrc", "mc"])
@pytest.mark.parametrize("source", ["u8_host", "u8_device", "f32_device"])
def test_device_rebuild_equals_creation_build(api, sc, cloud16, torch_gpu, kind, source):
    """density, occupancy bits and boxes after SetVolume(V) == those of a renderer created with V (the host builder), over empty, full,
    shifted, odd-sized, single-voxel (dilation across cell borders and diagonals) and 512x512x160 (16-voxel occupancy cells) volumes"""
    import torch
    groups = {}
    for name, v in _volumes(cloud16):
        groups.setdefault(v.shape, []).append((name, v))
    for shape, vols in groups.items():
        other = np.ascontiguousarray(np.flip(vols[0][1], axis=0) // 2 + 1)      # created with another volume of the same dims
        ren, nrc = _make(api, sc, kind, other)
        for i, (name, v) in enumerate(vols):
            fresh, fnrc = _make(api, sc, "mc", v)
            want = volume_buffers(fresh)
            fresh.Destroy()
            src = _as_source(v, source)
            held = api.live_allocations()
            ren.SetVolume(src)
            if source == "u8_device":      # (a device source: no staging buffer comes and goes)
                # DESIGN.md's memory table: nothing before the first swap, which allocates the slots -- NRC two, MC one -- and nothing after
                grown = api.live_allocations() - held
                print("%s %s SetVolume %d: %+d device allocations" % (kind, name, i, grown))
                assert grown == (FIRST_SWAP_ALLOCATIONS[kind] if i == 0 else 0), (kind, name, i, grown)
            got = volume_buffers(ren)
            assert_same_volume(got, want, name)
        ren.Destroy()
        if nrc is not None:
            nrc.Destroy()
    if source != "u8_host" or kind != "mc":
        return
    v = _sparse_512()
    fresh, _ = _make(api, sc, "mc", v)
    want = volume_buffers(fresh)
    fresh.Destroy()
    ren, _ = _make(api, sc, "mc", np.zeros_like(v))
    for src in (v, torch.from_numpy(v).cuda(), _as_source(v, "f32_device")):
        ren.SetVolume(src)
        assert_same_volume(volume_buffers(ren), want)
        ren.SetVolume(np.zeros_like(v))
    ren.Destroy()


# (nz, ny, nx), nx % 4 == 0: one workgroup per cell row, and two x-chunks with ragged y / z
UNALIGNED_SHAPES = {"64^3": (64, 64, 64), "264x9x10-two-chunks": (10, 9, 264)}


def _edge_volume(shape):
    """seeded sparse voxels, a block across cell borders and the volume's first and last voxels (the last four of x in the last row)"""
    rng = np.random.default_rng(shape[2])
    v = np.zeros(shape, np.uint8)
    idx = rng.integers(0, v.size, v.size // 200)
    v.reshape(-1)[idx] = rng.integers(1, 256, idx.size).astype(np.uint8)
    nz, ny, nx = shape
    v[nz // 2 - 1:nz // 2 + 2, 6:ny, 30:41] = 90
    v[0, 0, 0] = 1
    v[-1, -1, -4:] = (255, 3, 0, 7)
    return v


@pytest.mark.parametrize("fmt", ["u8", "f32"])
@pytest.mark.parametrize("name", list(UNALIGNED_SHAPES))
def test_unaligned_device_source_with_nx_a_multiple_of_four(api, sc, torch_gpu, name, fmt):
    """a device volume at element offset 1 of a larger tensor: nx % 4 == 0, but the source cannot be read four elements at a time, so the
    rebuild takes the scalar path with every lane's four voxels in range; the buffers equal those of a renderer created with the volume"""
    import torch
    v = _edge_volume(UNALIGNED_SHAPES[name])
    fresh, _ = _make(api, sc, "mc", v)
    want = volume_buffers(fresh)
    fresh.Destroy()
    host = v if fmt == "u8" else _to_f32(v)
    flat = torch.full((v.size + 8,), 1, dtype=torch.from_numpy(host).dtype, device="cuda")      # (non-zero around the volume)
    flat[1:1 + v.size] = torch.from_numpy(host.reshape(-1)).cuda()
    src = flat[1:1 + v.size].view(v.shape)
    assert src.data_ptr() % (4 * src.element_size()) != 0 and src.is_contiguous()
    ren, _ = _make(api, sc, "mc", np.zeros_like(v))
    ren.SetVolume(src)
    assert_same_volume(volume_buffers(ren), want, name)
    ren.Destroy()


def test_sparse_512_uses_16_voxel_occupancy_cells(api, sc, torch_gpu):
    """the 512x512x160 case above exercises occ_shift 4: 64 x 64 x 20 cells of 8 voxels would not fit the LDS table"""
    import torch
    v = _sparse_512()
    ren, nrc = _make(api, sc, "nrc", np.zeros_like(v))
    fresh, _ = _make(api, sc, "mc", v)
    want = volume_buffers(fresh)
    fresh.Destroy()
    assert want["occ_bits"].size == ((32 * 32 * 10 + 31) // 32 + 3) // 4 * 4
    ren.SetVolume(torch.from_numpy(v).cuda())
    assert_same_volume(volume_buffers(ren), want)
    ren.Destroy()
    nrc.Destroy()


def test_f32_quantisation(api, sc, torch_gpu):
    """NRC_VOLUME_F32: uint8(v * 255) truncated; v <= 0 and NaN -> 0, v >= 1 -> 255"""
    import torch
    k = np.arange(256, dtype=np.float32)
    exact = k / np.float32(255.0)
    vals = np.concatenate([exact, np.nextafter(exact, np.float32(-1)), np.nextafter(exact, np.float32(2)),
                           np.array([0.0, -0.0, 1.0, -1e-30, -0.5, -7.0, 1.0000001, 1.5, 300.0, np.nan, -np.nan, np.inf, -np.inf,
                                     1e-45, 0.9999999, 0.5, 0.003921568], np.float32)]).astype(np.float32)
    n = 16 * 16 * 16
    rng = np.random.default_rng(3)
    vol = np.concatenate([vals, rng.random(n - vals.size, dtype=np.float32) * np.float32(1.2) - np.float32(0.1)]).astype(np.float32)
    with np.errstate(invalid="ignore"):
        prod = vol * np.float32(255.0)
        want = np.where(~(vol > 0), 0, np.where(vol >= 1, 255, np.floor(np.where(np.isfinite(prod), prod, 0)))).astype(np.uint8)
    for kind in ("mc", "nrc"):
        ren, nrc = _make(api, sc, kind, np.zeros((16, 16, 16), np.uint8))
        ren.SetVolume(torch.from_numpy(vol.reshape(16, 16, 16)).cuda())
        got = ren.VolumeBuffer("density").cpu().numpy().reshape(-1)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
        ren.Destroy()
        if nrc is not None:
            nrc.Destroy()


def _rolled(cloud16):
    return np.ascontiguousarray(np.roll(cloud16, (30, 20, -50), axis=(0, 1, 2)))


@pytest.mark.parametrize("skip", [True, False], ids=["empty-skip", "no-skip"])
def test_mc_frame_after_swap_matches_oracle(api, orc, sc, cloud16, torch_gpu, skip):
    import torch
    W, H = 96, 54
    cam = sc.make_camera(aspect=W / H)
    A, B = cloud16, _rolled(cloud16)
    sa, sb = sc.make_scene(A, scene_id=4), sc.make_scene(B, scene_id=4)
    mc = api.McHpmRenderer(W, H, 32, False, cam, sa)
    mc.SetEmptySkip(skip)
    mc.SetFrameRandom(FRAME_RANDOM)
    mc.Render()
    first = mc.GetImage().cpu().numpy().copy()
    ref_a, _, _ = orc.mc_render(sa, cam, W, H, 32, FRAME_RANDOM, threads=8)
    assert same_bits(first, ref_a)
    mc.SetVolume(torch.from_numpy(B).cuda())
    mc.SetFrameRandom(FRAME_RANDOM)
    mc.Render()
    img = mc.GetImage().cpu().numpy()
    ref_b, _, _ = orc.mc_render(sb, cam, W, H, 32, FRAME_RANDOM, threads=8)
    assert same_bits(img, ref_b)
    assert not same_bits(img, first)
    mc.Destroy()


def test_nrc_primary_after_swap_matches_oracle(api, orc, sc, cloud16, torch_gpu):
    import torch
    W, H = 96, 54
    A, B = cloud16, _rolled(cloud16)
    sb = sc.make_scene(B, scene_id=3)
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=10, log2_infer_batch_size=14, scene_id=3)
    nrc = api.NeuralRadianceCache(cfg)
    cam = sc.make_camera(aspect=W / H)
    ren = api.NrcHpmRenderer(W, H, False, cam, cfg, sc.make_scene(A, scene_id=3), nrc)
    for f in range(2):
        ren.Render(None, True)
    ren.SetVolume(torch.from_numpy(B).cuda())
    ren.SetFrameRandom(FRAME_RANDOM)
    ren.Render(None, False)
    o = orc.nrc_gen_rays(sb, cam, W, H, 1, 0.0, FRAME_RANDOM, threads=8)
    prim = ren.Buffer("primary").cpu().numpy().reshape(H, W, 4)
    assert same_bits(prim, o["primary"])
    ren.Destroy()
    nrc.Destroy()


def test_nrc_frame_after_swap_equals_fresh_renderer_with_blending(api, sc, cloud16, torch_gpu):
    """blending restarts: with the same frame randoms and cache, the first frame after SetVolume(B) == a fresh renderer's first frame of B"""
    import torch
    W, H = 128, 80
    A, B = cloud16, _rolled(cloud16)
    cam = sc.make_camera(aspect=W / H)
    frs = sc.frame_randoms(4, seed=5)
    imgs = []
    for vol in ("swap", "fresh"):
        cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=10, log2_infer_batch_size=14, seed=42)
        nrc = api.NeuralRadianceCache(cfg)
        ren = api.NrcHpmRenderer(W, H, True, cam, cfg, sc.make_scene(A if vol == "swap" else B, scene_id=4), nrc)
        if vol == "swap":
            for f in range(3):
                ren.SetFrameRandom(frs[f])
                ren.Render(None, False)
            ren.SetVolume(torch.from_numpy(B).cuda())
        ren.SetFrameRandom(frs[3])
        ren.Render(None, False)
        imgs.append(ren.GetImage().cpu().numpy().copy())
        ren.Destroy()
        nrc.Destroy()
    assert np.isfinite(imgs[0]).all()
    assert same_bits(imgs[0], imgs[1])


@pytest.mark.parametrize("fix", [0, 2], ids=["default", "q2-long-trace"])
def test_swaps_inside_pipelined_graph_equal_single_stream(api, sc, cloud16, torch_gpu, monkeypatch, fix):
    """a SetVolume from one of three device volumes before each of 12 trained frames, no host wait: the four-stream graph (with quirk
    Q2 fixed: plus the trace streams) ends with the framebuffer, loss and parameters of the single-stream order, bit for bit"""
    import torch
    W, H = 256, 160
    vols = [torch.from_numpy(v).cuda() for v in (cloud16, _rolled(cloud16), np.ascontiguousarray(cloud16[::-1]))]
    extra = dict(compat_fix=2, train_ray_length=32, train_spp=1) if fix else {}
    frs = sc.frame_randoms(12, seed=9)
    results = []
    for single in (True, False):
        nrc_debug(monkeypatch, single_stream=single, poison_alloc=True)
        cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=10, log2_infer_batch_size=14, **extra)
        nrc = api.NeuralRadianceCache(cfg)
        cam = sc.make_camera(aspect=W / H)
        ren = api.NrcHpmRenderer(W, H, True, cam, cfg, sc.make_scene(cloud16, scene_id=4), nrc)
        for f in range(12):
            ren.SetVolume(vols[(f + 1) % 3])
            ren.SetFrameRandom(frs[f])
            ren.Render(None, True)
        results.append((ren.GetImage().cpu().numpy().copy(), nrc.GetLoss(), nrc.GetParams(0).copy(), nrc.GetParams(1).copy()))
        ren.Destroy()
        nrc.Destroy()
    nrc_debug(monkeypatch)
    a, b = results
    assert np.isfinite(a[0]).all()
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert a[1] == b[1]
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32))


def test_set_volume_does_not_wait_for_the_gpu(api, sc, torch_gpu):
    """behind a backlog of 32 frames at 1080p, SetVolume from a device tensor returns long before the backlog has run"""
    import torch
    W, H = 1920, 1080
    A = sc.cached_volume("cloud", 128, seed=1337)
    B = sc.cached_volume("cloud", 128, seed=1338)
    dB = torch.from_numpy(B).cuda()
    cfg = api.AppConfig()
    cam = sc.make_camera(aspect=W / H)
    renders = []
    for vol in ("swap", "fresh"):
        nrc = api.NeuralRadianceCache(cfg)
        ren = api.NrcHpmRenderer(W, H, False, cam, cfg, sc.make_scene(A if vol == "swap" else B, scene_id=4), nrc)
        renders.append((ren, nrc))
    ren, _ = renders[0]
    ren.SetVolume(torch.from_numpy(A).cuda())      # (first call: slots allocated)
    ren.RenderFrames(sc.frame_randoms(4, seed=1), train=True)
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(s)
    ren.RenderFrames(sc.frame_randoms(32, seed=2), train=True)
    ren.GetImage()      # (the stream waits for the last compositing on the device)
    end.record(s)
    t0 = time.perf_counter()
    ren.SetVolume(dB)
    host_ms = (time.perf_counter() - t0) * 1e3
    end.synchronize()
    gpu_ms = start.elapsed_time(end)
    assert host_ms < 0.25 * gpu_ms, (host_ms, gpu_ms)
    prims = []
    for r, _ in renders:
        r.SetFrameRandom(FRAME_RANDOM)
        r.Render(None, False)
        prims.append(r.Buffer("primary").cpu().numpy().copy())
    assert np.isfinite(renders[0][0].GetImage().cpu().numpy()).all()
    assert same_bits(prims[0], prims[1])      # the frame after the swap shows B
    for r, n in renders:
        r.Destroy()
        n.Destroy()


def test_errors_leave_the_renderer_unchanged(api, sc, cloud16, torch_gpu):
    import torch
    W, H = 96, 54
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=10, log2_infer_batch_size=14)
    nrc = api.NeuralRadianceCache(cfg)
    cam = sc.make_camera(aspect=W / H)
    scene = sc.make_scene(cloud16, scene_id=4)
    ren = api.NrcHpmRenderer(W, H, False, cam, cfg, scene, nrc)
    mc = api.McHpmRenderer(W, H, 16, False, cam, scene)

    def frames():
        ren.SetFrameRandom(FRAME_RANDOM)
        ren.Render(None, False)
        mc.SetFrameRandom(FRAME_RANDOM)
        mc.Render()
        return ren.Buffer("primary").cpu().numpy().copy(), mc.GetImage().cpu().numpy().copy()

    before = frames()
    wrong = torch.zeros((cloud16.shape[0], cloud16.shape[1], cloud16.shape[2] + 1), dtype=torch.uint8, device="cuda")
    good = torch.from_numpy(np.full_like(cloud16, 255)).cuda()
    nz, ny, nx = cloud16.shape
    L = api.load_library()
    for r, set_fn in ((ren, L.nrc_renderer_set_volume), (mc, L.nrc_mc_renderer_set_volume)):
        with pytest.raises(RuntimeError, match="SkyRenderer ERROR"):
            r.SetVolume(wrong)
        with pytest.raises(RuntimeError, match="SkyRenderer ERROR"):
            r.SetVolume(np.zeros((nz, ny, nx), np.float64))
        assert set_fn(r.h, C.c_void_p(good.data_ptr()), nx, ny, nz, 7, 1) != 0      # unknown format
        assert b"SkyRenderer ERROR" in L.nrc_last_error()
        assert set_fn(r.h, None, nx, ny, nz, 0, 1) != 0                              # NULL
        assert b"SkyRenderer ERROR" in L.nrc_last_error()
    after = frames()
    assert same_bits(before[0], after[0])
    assert same_bits(before[1], after[1])
    ren.Destroy()
    mc.Destroy()
    nrc.Destroy()
