"""nrc_renderer_set_volume_bricks / nrc_mc_renderer_set_volume_bricks: a live renderer's density volume replaced from a list of 8^3
bricks.  The device buffers equal, byte for byte, those of a renderer created with the densified list (scene.bricks_to_volume) and those
after the dense SetVolume of it; frames after a brick swap equal a fresh renderer's / the oracle's; bad host lists change nothing."""
import ctypes as C
import time

import numpy as np
import pytest

from conftest import FRAME_RANDOM, nrc_debug
from volume_common import _make, _sparse_512, _to_f32, assert_same_volume, same_bits, volume_buffers

pytestmark = pytest.mark.gpu


def _destroy(*objs):
    for o in objs:
        if o is not None:
            o.Destroy()


def _created_with(api, sc, vol):
    """the buffers renderer creation builds on the host for vol"""
    fresh, _ = _make(api, sc, "mc", np.ascontiguousarray(vol))
    want = volume_buffers(fresh)
    fresh.Destroy()
    return want


def _odd():
    """[nz][ny][nx] = 70 x 45 x 61: no dim a multiple of 8, nx % 4 != 0"""
    rng = np.random.default_rng(5)
    v = np.zeros((70, 45, 61), np.uint8)
    idx = rng.integers(0, v.size, 300)
    v.reshape(-1)[idx] = rng.integers(1, 256, idx.size).astype(np.uint8)
    v[10:23, 30:45, 50:61] = rng.integers(0, 256, (13, 15, 11)).astype(np.uint8)
    v[60:70, 0:9, 0:3] = 77
    return v


def _cube64():
    rng = np.random.default_rng(6)
    v = np.zeros((64, 64, 64), np.uint8)
    v[7:9, 15:17, 23:25] = 200            # across cell borders in every axis
    v[40:64, 0:20, 56:64] = rng.integers(0, 256, (24, 20, 8)).astype(np.uint8)
    v[0, 0, 0] = 1
    v[63, 63, 63] = 255
    return v


def _as_lists(origins, bricks_u8, source):
    """the brick list as one of the four kinds of source: u8 / f32, host (numpy) / device (torch)"""
    import torch
    fmt, where = source.split("_")
    # (an empty cell's voxels must stay 0 in f32 too)
    b = bricks_u8 if fmt == "u8" else np.where(bricks_u8 > 0, _to_f32(bricks_u8), np.float32(0.0)).astype(np.float32)
    o, b = np.ascontiguousarray(origins, np.int32), np.ascontiguousarray(b)
    if where == "host":
        return o, b
    return torch.from_numpy(o).cuda(), torch.from_numpy(b).cuda()


SOURCES = ["u8_host", "u8_device", "f32_host", "f32_device"]


@pytest.mark.parametrize("kind", ["nrc", "mc"])
@pytest.mark.parametrize("source", SOURCES)
def test_brick_rebuild_equals_creation_and_dense_rebuild(api, sc, cloud16, torch_gpu, kind, source):
    """density, occupancy bits and boxes after SetVolumeBricks(volume_to_bricks(V)) == those of a renderer created with V == those after
    the dense SetVolume(V), over the fixture cloud, 61x45x70 (no dim a multiple of 8, nx % 4 != 0) and 64^3"""
    for name, v in (("cloud16", cloud16), ("odd61x45x70", _odd()), ("cube64", _cube64())):
        origins, bricks = sc.volume_to_bricks(v)
        assert np.array_equal(sc.bricks_to_volume(origins, bricks, v.shape), v)
        want = _created_with(api, sc, v)
        other = np.ascontiguousarray(np.flip(v, axis=0) // 2 + 1)      # created with another, dense volume of the same dims
        ren, nrc = _make(api, sc, kind, other)
        ren.SetVolumeBricks(*_as_lists(origins, bricks, source))
        got = volume_buffers(ren)
        assert_same_volume(got, want, name)
        ren.SetVolume(np.ascontiguousarray(v))
        assert_same_volume(volume_buffers(ren), got, name + " dense")
        ren.SetVolumeBricks(*_as_lists(origins, bricks, source))      # (NRC: the other slot, which held `other`'s successor)
        assert_same_volume(volume_buffers(ren), want, name + " again")
        _destroy(ren, nrc)


@pytest.mark.parametrize("source", SOURCES)
def test_sparse_512_bricks(api, sc, torch_gpu, source):
    """512 x 512 x 160 (16-voxel occupancy cells), a few thousand bricks: equals creation and the dense rebuild on both renderers"""
    v = _sparse_512()
    origins, bricks = sc.volume_to_bricks(v)
    assert 3000 < len(origins) < 64 * 64 * 20
    want = _created_with(api, sc, v)
    assert want["occ_bits"].size == ((32 * 32 * 10 + 31) // 32 + 3) // 4 * 4
    full = np.full_like(v, 3)
    for kind in ("mc", "nrc"):
        ren, nrc = _make(api, sc, kind, full)
        ren.SetVolumeBricks(*_as_lists(origins, bricks, source))
        assert_same_volume(volume_buffers(ren), want, kind)
        if source == "u8_device":
            ren.SetVolume(full)
            ren.SetVolume(v)
            assert_same_volume(volume_buffers(ren), want, kind + " dense")
            ren.SetVolumeBricks(*_as_lists(origins, bricks, source))
            assert_same_volume(volume_buffers(ren), want, kind + " reused slot")
        _destroy(ren, nrc)


@pytest.mark.parametrize("kind", ["nrc", "mc"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_reused_slot_keeps_nothing_of_its_old_contents(api, sc, cloud16, torch_gpu, kind, where):
    """A -> B -> C -> (dense D) -> A on one renderer: the NRC renderer's two slots and the MC renderer's one are each rewritten while
    holding a volume whose cells the new list does not cover; every state equals the creation build of the densified list"""
    nz, ny, nx = cloud16.shape
    a = cloud16
    b = np.zeros_like(a)
    b[100:140, 10:30, 0:40] = a[100:140, 10:30, 0:40]       # a corner of the cloud's grid
    b[30, 80, 120] = 9                                         # (outside c)
    c = np.zeros_like(a)
    c[0:20, 60:86, 90:126] = 200                              # another corner, up to the y and x edges
    d = np.ascontiguousarray(np.roll(a, (30, 20, -50), axis=(0, 1, 2)))
    assert not (b.astype(bool) & c.astype(bool)).any()
    want = {k: _created_with(api, sc, v) for k, v in (("a", a), ("b", b), ("c", c), ("d", d))}
    ren, nrc = _make(api, sc, kind, np.full_like(a, 255))
    vols = dict(a=a, b=b, c=c, d=d)
    for step in ("a", "b", "c", "b", "d", "c", "a"):
        if step == "d":
            ren.SetVolume(d)                                  # dense and brick swaps share the slots
        else:
            ren.SetVolumeBricks(*_as_lists(*sc.volume_to_bricks(vols[step]), "u8_" + where))
        assert_same_volume(volume_buffers(ren), want[step], step)
    _destroy(ren, nrc)


def test_empty_list_is_the_empty_medium(api, sc, cloud16, torch_gpu):
    import torch
    W, H = 96, 54
    cam = sc.make_camera(aspect=W / H)
    zeros = np.zeros_like(cloud16)
    want = _created_with(api, sc, zeros)
    fresh = api.McHpmRenderer(W, H, 16, False, cam, sc.make_scene(zeros, scene_id=4))
    fresh.SetFrameRandom(FRAME_RANDOM)
    fresh.Render()
    ref = fresh.GetImage().cpu().numpy().copy()
    fresh.Destroy()
    L = api.load_library()
    for where in ("host", "device", "null"):
        mc = api.McHpmRenderer(W, H, 16, False, cam, sc.make_scene(cloud16, scene_id=4))
        if where == "host":
            mc.SetVolumeBricks(np.zeros((0, 3), np.int32), np.zeros((0, 8, 8, 8), np.uint8))
        elif where == "device":
            mc.SetVolumeBricks(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), torch.zeros((0, 8, 8, 8), dtype=torch.float32, device="cuda"))
        else:
            assert L.nrc_mc_renderer_set_volume_bricks(mc.h, None, None, 0, api.VOLUME_U8, 1) == 0
        got = volume_buffers(mc)
        assert not got["density"].any() and got["boxes"].shape == (0, 6) and not got["occ_bits"].any()
        assert_same_volume(got, want, where)
        mc.SetFrameRandom(FRAME_RANDOM)
        mc.Render()
        assert same_bits(mc.GetImage().cpu().numpy(), ref)
        mc.Destroy()
    ren, nrc = _make(api, sc, "nrc", cloud16)
    ren.SetVolumeBricks(np.zeros((0, 3), np.int32), np.zeros((0, 8, 8, 8), np.float32))
    assert_same_volume(volume_buffers(ren), want, "nrc")
    _destroy(ren, nrc)


@pytest.mark.parametrize("kind", ["nrc", "mc"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_zero_bricks_duplicates_and_edges(api, sc, torch_gpu, kind, where):
    """an all-zero brick leaves its cell empty; of several bricks naming one cell the highest index wins, whole (its zeros too); a brick
    poking past the edge is cropped -- on 29 x 21 x 43 (nx 29: the scalar-store path) and 32 x 24 x 40 (the 4-byte-store path)"""
    import torch
    rng = np.random.default_rng(8)
    for nx, ny, nz in ((29, 21, 43), (32, 24, 40)):
        corner = ((nx - 1) // 8 * 8, (ny - 1) // 8 * 8, (nz - 1) // 8 * 8)
        cells = [(x, y, z) for z in range(0, nz, 8) for y in range(0, ny, 8) for x in range(0, nx, 8) if (x, y, z) != corner]
        pick = rng.permutation(len(cells))[:20]
        origins = np.array([cells[i] for i in pick] + [cells[pick[0]], cells[pick[1]], cells[pick[0]], cells[pick[5]]], np.int32)
        bricks = (rng.random((len(origins), 8, 8, 8)) < 0.1) * rng.integers(1, 256, (len(origins), 8, 8, 8))
        bricks = bricks.astype(np.uint8)
        bricks[3] = 0                      # an all-zero brick
        bricks[len(origins) - 1] = 0       # an all-zero brick that wins over a non-zero one (cells[pick[5]])
        bricks[5, 0, 0, 0] = 99
        last = np.array([corner], np.int32)      # pokes past every edge of 29 x 21 x 43
        origins = np.concatenate([origins, last])
        bricks = np.concatenate([bricks, np.full((1, 8, 8, 8), 255, np.uint8)])
        dense = sc.bricks_to_volume(origins, bricks, (nz, ny, nx))
        assert dense[nz - 1, ny - 1, nx - 1] == 255 and not dense[cells[pick[5]][2], cells[pick[5]][1], cells[pick[5]][0]]
        want = _created_with(api, sc, dense)
        ren, nrc = _make(api, sc, kind, np.full((nz, ny, nx), 7, np.uint8))
        for fmt in ("u8", "f32"):
            ren.SetVolumeBricks(*_as_lists(origins, bricks, fmt + "_" + where))
            assert_same_volume(volume_buffers(ren), want, (nx, fmt))
        if where == "device":              # a brick pointer aligned to one element only (a view into a larger tensor)
            o, b = _as_lists(origins, bricks, "u8_device")
            shifted = torch.zeros(b.numel() + 1, dtype=torch.uint8, device="cuda")
            shifted[1:] = b.reshape(-1)
            ren.SetVolume(np.full((nz, ny, nx), 7, np.uint8))
            ren.SetVolumeBricks(o, shifted[1:].view(-1, 8, 8, 8))
            assert_same_volume(volume_buffers(ren), want, (nx, "unaligned"))
        _destroy(ren, nrc)


@pytest.mark.parametrize("where", ["host", "device"])
def test_f32_quantisation(api, sc, torch_gpu, where):
    """NRC_VOLUME_F32 bricks: uint8(v * 255) truncated; v <= 0 and NaN -> 0, v >= 1 -> 255 (the dense call's rule)"""
    import torch
    k = np.arange(256, dtype=np.float32)
    exact = k / np.float32(255.0)
    vals = np.concatenate([exact, np.nextafter(exact, np.float32(-1)), np.nextafter(exact, np.float32(2)),
                           np.array([0.0, -0.0, 1.0, -1e-30, -0.5, -7.0, 1.0000001, 1.5, 300.0, np.nan, -np.nan, np.inf, -np.inf,
                                     1e-45, 0.9999999, 0.5, 0.003921568], np.float32)]).astype(np.float32)
    rng = np.random.default_rng(3)
    n = 8 * 512
    flat = np.concatenate([vals, rng.random(n - vals.size, dtype=np.float32) * np.float32(1.2) - np.float32(0.1)]).astype(np.float32)
    bricks = flat.reshape(8, 8, 8, 8)
    origins = np.array([[x, y, z] for z in (0, 8) for y in (0, 8) for x in (0, 8)], np.int32)
    with np.errstate(invalid="ignore"):
        prod = bricks * np.float32(255.0)
        q = np.where(~(bricks > 0), 0, np.where(bricks >= 1, 255, np.floor(np.where(np.isfinite(prod), prod, 0)))).astype(np.uint8)
    want = sc.bricks_to_volume(origins, q, (16, 16, 16))
    for kind in ("mc", "nrc"):
        ren, nrc = _make(api, sc, kind, np.zeros((16, 16, 16), np.uint8))
        if where == "host":
            ren.SetVolumeBricks(origins, bricks)
        else:
            ren.SetVolumeBricks(torch.from_numpy(origins).cuda(), torch.from_numpy(bricks).cuda())
        got = ren.VolumeBuffer("density").cpu().numpy()
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]
        assert_same_volume(volume_buffers(ren), _created_with(api, sc, want), kind)
        _destroy(ren, nrc)


def _rolled(cloud16):
    return np.ascontiguousarray(np.roll(cloud16, (30, 20, -50), axis=(0, 1, 2)))


@pytest.mark.parametrize("single", [False, True], ids=["pipelined", "single-stream"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_nrc_frames_after_brick_swap_equal_fresh_renderer(api, sc, cloud16, torch_gpu, monkeypatch, single, where):
    """a blending renderer: three untrained frames of A (the weights stay as created), SetVolumeBricks(B), then four trained frames.
    The first of them equals the first trained frame of a fresh renderer created with B (blending restarted, weights as created: the
    statement of test_gpu_volume_update.py::test_nrc_frame_after_swap_equals_fresh_renderer_with_blending).  The later ones cannot be held
    against the fresh renderer: the swap keeps the training ring (include/nrc_hpm.h), every frame pushes its rays into it, trained or
    not, so from the second step on the swapped renderer trains on rays of A that the fresh one never saw.  They are held, image by
    image and in the trained weights, against a renderer with the same history that B reached through the dense SetVolume -- through
    the pipelined graph and in single-stream order."""
    import torch
    W, H = 128, 80
    A, B = cloud16, _rolled(cloud16)
    cam = sc.make_camera(aspect=W / H)
    frs = sc.frame_randoms(7, seed=5)
    nrc_debug(monkeypatch, single_stream=single)
    runs = {}
    for how in ("bricks", "dense", "fresh"):
        cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=10, log2_infer_batch_size=14, seed=42)
        nrc = api.NeuralRadianceCache(cfg)
        ren = api.NrcHpmRenderer(W, H, True, cam, cfg, sc.make_scene(B if how == "fresh" else A, scene_id=4), nrc)
        if how != "fresh":
            for f in range(3):
                ren.SetFrameRandom(frs[f])
                ren.Render(None, False)
            if how == "bricks":
                ren.SetVolumeBricks(*_as_lists(*sc.volume_to_bricks(B), "u8_" + where))
            else:
                ren.SetVolume(torch.from_numpy(B).cuda())
        imgs = []
        for f in range(3, 7):
            ren.SetFrameRandom(frs[f])
            ren.Render(None, True)
            imgs.append(ren.GetImage().cpu().numpy().copy())
        imgs.append(nrc.GetParams(0).copy())
        runs[how] = imgs
        _destroy(ren, nrc)
    nrc_debug(monkeypatch)
    assert all(np.isfinite(i).all() for i in runs["bricks"])
    assert same_bits(runs["bricks"][0], runs["fresh"][0])
    for f in range(4):
        assert same_bits(runs["bricks"][f], runs["dense"][f]), f
    assert np.array_equal(runs["bricks"][4].view(np.uint32), runs["dense"][4].view(np.uint32))
    assert not same_bits(runs["bricks"][3], runs["bricks"][0])

@pytest.mark.parametrize("where", ["host", "device"])
def test_mc_frame_after_brick_swap_matches_oracle(api, orc, sc, cloud16, torch_gpu, where):
    W, H = 96, 54
    cam = sc.make_camera(aspect=W / H)
    A, B = cloud16, _rolled(cloud16)
    origins, bricks = sc.volume_to_bricks(B)
    sb = sc.make_scene(sc.bricks_to_volume(origins, bricks, B.shape), scene_id=4)
    mc = api.McHpmRenderer(W, H, 32, False, cam, sc.make_scene(A, scene_id=4))
    mc.SetFrameRandom(FRAME_RANDOM)
    mc.Render()
    first = mc.GetImage().cpu().numpy().copy()
    mc.SetVolumeBricks(*_as_lists(origins, bricks, "f32_" + where))
    mc.SetFrameRandom(FRAME_RANDOM)
    mc.Render()
    img = mc.GetImage().cpu().numpy()
    ref_b, _, _ = orc.mc_render(sb, cam, W, H, 32, FRAME_RANDOM, threads=8)
    assert same_bits(img, ref_b)
    assert not same_bits(img, first)
    mc.Destroy()


def test_bad_host_lists_leave_the_renderer_unchanged(api, sc, cloud16, torch_gpu):
    import torch
    W, H = 96, 54
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=10, log2_infer_batch_size=14)
    nrc = api.NeuralRadianceCache(cfg)
    cam = sc.make_camera(aspect=W / H)
    scene = sc.make_scene(cloud16, scene_id=4)
    ren = api.NrcHpmRenderer(W, H, False, cam, cfg, scene, nrc)
    mc = api.McHpmRenderer(W, H, 16, False, cam, scene)
    nz, ny, nx = cloud16.shape

    def state():
        ren.SetFrameRandom(FRAME_RANDOM)
        ren.Render(None, False)
        mc.SetFrameRandom(FRAME_RANDOM)
        mc.Render()
        return (ren.Buffer("primary").cpu().numpy().copy(), mc.GetImage().cpu().numpy().copy(), volume_buffers(ren), volume_buffers(mc))

    before = state()
    good_b = np.full((3, 8, 8, 8), 255, np.uint8)
    L = api.load_library()
    bad_origins = {"unaligned": [[0, 0, 0], [8, 8, 8], [8, 12, 8]], "x out of range": [[0, 0, 0], [8, 8, 8], [nx // 8 * 8 + 8, 0, 0]],
                   "z out of range": [[0, 0, 0], [8, 8, 8], [0, 0, (nz + 7) // 8 * 8]], "negative": [[0, 0, 0], [8, 8, 8], [-8, 0, 0]]}
    for r, fn in ((ren, L.nrc_renderer_set_volume_bricks), (mc, L.nrc_mc_renderer_set_volume_bricks)):
        for name, o in bad_origins.items():
            with pytest.raises(RuntimeError, match="SkyRenderer ERROR.*brick 2"):
                r.SetVolumeBricks(np.array(o, np.int32), good_b)
        o = np.array([[0, 0, 0], [8, 8, 8], [16, 0, 0]], np.int32)
        assert fn(r.h, C.c_void_p(o.ctypes.data), C.c_void_p(good_b.ctypes.data), 3, 7, 0) == -1      # NRC_ERR_INVALID: unknown format
        assert b"SkyRenderer ERROR" in L.nrc_last_error()
        assert fn(r.h, None, C.c_void_p(good_b.ctypes.data), 3, 0, 0) == -1                              # NULL origins, n > 0
        assert b"SkyRenderer ERROR" in L.nrc_last_error()
        assert fn(r.h, C.c_void_p(o.ctypes.data), None, 3, 0, 0) == -1                                   # NULL bricks, n > 0
        assert b"SkyRenderer ERROR" in L.nrc_last_error()
        d_o = torch.from_numpy(o).cuda()
        assert fn(r.h, C.c_void_p(d_o.data_ptr()), None, 3, 0, 1) == -1
        for args in ((o, good_b[:2]), (o.astype(np.int64), good_b), (o, good_b.astype(np.float64)), (o, torch.from_numpy(good_b).cuda()),
                     (o.reshape(-1), good_b)):
            with pytest.raises(RuntimeError, match="SkyRenderer ERROR"):
                r.SetVolumeBricks(*args)
    after = state()
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
    assert_same_volume(after[2], before[2], "nrc")
    assert_same_volume(after[3], before[3], "mc")
    _destroy(ren, mc, nrc)


@pytest.mark.parametrize("kind", ["nrc", "mc"])
def test_invalid_origins_in_a_device_list_are_ignored(api, sc, cloud16, torch_gpu, kind):
    """a device list cannot be checked without a wait: its unaligned, negative and out-of-range bricks count as absent (also as
    duplicates: a later invalid brick does not displace a valid one), and the frame is that of the valid bricks alone"""
    import torch
    nz, ny, nx = cloud16.shape
    origins, bricks = sc.volume_to_bricks(cloud16)
    bad = np.array([[4, 0, 0], [0, 8, 3], [-8, 0, 0], [0, -16, 0], [(nx + 7) // 8 * 8, 0, 0], [0, (ny + 7) // 8 * 8, 0],
                    [0, 0, (nz + 7) // 8 * 8], [2 ** 31 - 8, 0, 0], [0, 0, -2 ** 31], [8, 8, 2 ** 30]], np.int32)
    rng = np.random.default_rng(2)
    pos = np.sort(rng.integers(0, len(origins), len(bad)))
    o = np.insert(origins, pos, bad, axis=0)
    b = np.insert(bricks, pos, np.full((len(bad), 8, 8, 8), 255, np.uint8), axis=0)
    o, b = np.concatenate([o, bad]), np.concatenate([b, np.full((len(bad), 8, 8, 8), 255, np.uint8)])
    assert np.array_equal(sc.bricks_to_volume(o, b, cloud16.shape, ignore_invalid=True), cloud16)
    want = _created_with(api, sc, cloud16)
    W, H = 96, 54
    ren, nrc = _make(api, sc, kind, np.zeros_like(cloud16), W, H)
    fresh, fnrc = _make(api, sc, kind, cloud16, W, H)
    ren.SetVolumeBricks(torch.from_numpy(o).cuda(), torch.from_numpy(b).cuda())
    assert_same_volume(volume_buffers(ren), want, kind)
    imgs = []
    for r in (ren, fresh):
        r.SetFrameRandom(FRAME_RANDOM)
        if kind == "mc":
            r.Render()
            imgs.append(r.GetImage().cpu().numpy().copy())
        else:
            r.Render(None, False)
            imgs.append(r.Buffer("primary").cpu().numpy().copy())
    assert same_bits(imgs[0], imgs[1])
    _destroy(ren, fresh, nrc, fnrc)


def test_device_list_call_does_not_wait_for_the_gpu(api, sc, torch_gpu):
    """behind a backlog of 32 frames at 1080p, SetVolumeBricks from device tensors returns long before the backlog has run
    (the method of test_gpu_volume_update.py::test_set_volume_does_not_wait_for_the_gpu)"""
    import torch
    W, H = 1920, 1080
    A = sc.cached_volume("cloud", 128, seed=1337)
    B = sc.cached_volume("cloud", 128, seed=1338)
    oB, bB = (torch.from_numpy(x).cuda() for x in sc.volume_to_bricks(B))
    cfg = api.AppConfig()
    cam = sc.make_camera(aspect=W / H)
    renders = []
    for vol in ("swap", "fresh"):
        nrc = api.NeuralRadianceCache(cfg)
        ren = api.NrcHpmRenderer(W, H, False, cam, cfg, sc.make_scene(A if vol == "swap" else B, scene_id=4), nrc)
        renders.append((ren, nrc))
    ren, _ = renders[0]
    ren.SetVolumeBricks(*(torch.from_numpy(x).cuda() for x in sc.volume_to_bricks(A)))      # (first call: slots and index allocated)
    ren.RenderFrames(sc.frame_randoms(4, seed=1), train=True)
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(s)
    ren.RenderFrames(sc.frame_randoms(32, seed=2), train=True)
    ren.GetImage()      # (the stream waits for the last compositing on the device)
    end.record(s)
    t0 = time.perf_counter()
    ren.SetVolumeBricks(oB, bB)
    host_ms = (time.perf_counter() - t0) * 1e3
    end.synchronize()
    gpu_ms = start.elapsed_time(end)
    print("SetVolumeBricks host %.3f ms, backlog %.3f ms" % (host_ms, gpu_ms))
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
