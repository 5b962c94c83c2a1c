"""Volume keyframes (nrc_renderer_set_volume_keys / _set_volume_time / _render_path_timed and their nrc_mc_renderer_ twins).  The
specification is an equivalence, and every comparison here is for equal bytes: SetVolumeTime(t) is SetVolume(scene.volume_at(keys, t)) --
the same three device buffers, the same frames, the same training -- and RenderPath(times=...) is the loop SetVolumeTime + SetCamera +
k x Render, enqueued by one call that does not wait for the GPU."""
import ctypes as C
import time

import numpy as np
import pytest

from conftest import nrc_debug
from volume_common import _make as _small, assert_same_volume, volume_buffers

pytestmark = pytest.mark.gpu

CFG = dict(train_batch_count=1, log2_train_batch_size=10, log2_infer_batch_size=14)
# (nz, ny, nx): the smallest shapes at which k_vol_ingest takes another path with the blended source (VolLerp)
SHAPES = {"61x45x70-ragged-no-vec": (70, 45, 61), "64^3-vec": (64, 64, 64), "264x9x10-two-chunks-vec": (10, 9, 264),
          "261x9x10-two-chunks-no-vec": (10, 9, 261)}
N_KEYS = 5      # cloud, rolled cloud, zeros, synthetic A, synthetic B
WEIGHTS = (0, 1, 128, 129, 255, 256)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _fit(vol, shape):
    """the middle of `vol`, cropped or padded with zeros to `shape`"""
    out = np.zeros(shape, np.uint8)
    src, dst = [], []
    for n, m in zip(vol.shape, shape):
        k = min(n, m)
        src.append(slice((n - k) // 2, (n - k) // 2 + k))
        dst.append(slice((m - k) // 2, (m - k) // 2 + k))
    out[tuple(dst)] = vol[tuple(src)]
    return out


def _synthetic_pair(shape):
    """key A: isolated voxels of value 1 and 255 (alternating) on cell corners, cell edges and the volume's faces, every one alone in
    its 8^3 cell and with empty cells around it where the shape allows; key B: zero there and non-zero everywhere else"""
    nz, ny, nx = shape
    a = np.zeros(shape, np.uint8)
    spots = []
    for cz in range(0, (nz + 7) // 8, 2):
        for cy in range(0, (ny + 7) // 8, 2):
            for cx in range(0, (nx + 7) // 8, 2):
                k = len(spots)
                corner = ((0, 0, 0), (7, 7, 7), (7, 0, 7), (0, 7, 0))[k % 4]
                edge = ((0, 0, 3), (7, 4, 7), (2, 7, 0))[k % 3]
                dz, dy, dx = corner if k % 2 == 0 else edge
                spots.append((min(cz * 8 + dz, nz - 1), min(cy * 8 + dy, ny - 1), min(cx * 8 + dx, nx - 1)))
    spots += [(0, ny // 2, nx // 2), (nz - 1, ny // 2, nx // 3), (nz // 2, 0, nx // 2), (nz // 3, ny - 1, nx // 2), (nz // 2, ny // 2, 0),
              (nz // 2, ny // 3, nx - 1), (nz - 1, ny - 1, nx - 1), (0, 0, 0)]
    for k, p in enumerate(spots):
        a[p] = 1 if (k // 2) % 2 == 0 else 255      # (corners and edges alternate with k: both get both values)
    rng = np.random.default_rng(nx * 1000 + ny)
    b = np.where(a != 0, 0, rng.integers(1, 256, shape)).astype(np.uint8)
    return a, b


_KEYS = {}


def keys_of(cloud16, shape):
    """the key sequence of a shape (computed once, never written to): the fixture cloud cropped / padded, a rolled copy of it, an all-zero key
    and the synthetic pair"""
    if shape not in _KEYS:
        cloud = _fit(cloud16, shape)
        rolled = np.ascontiguousarray(np.roll(cloud, (shape[0] // 3, -(shape[1] // 4), shape[2] // 5), axis=(0, 1, 2)))
        a, b = _synthetic_pair(shape)
        keys = np.ascontiguousarray(np.stack([cloud, rolled, np.zeros(shape, np.uint8), a, b]))
        keys.setflags(write=False)
        _KEYS[shape] = keys
    return _KEYS[shape]


def time_of(i, W):
    """a time whose key pair and weight are exactly (i, W), W = 256 included (the last fp32 below i + 1)"""
    return float(np.nextafter(np.float32(i + 1), np.float32(0))) if W == 256 else i + W / 256.0


def times_of(shape):
    """the tested times of a shape's keys: every pair at WEIGHTS and two seeded weights, and the last key itself"""
    rng = np.random.default_rng(shape[2])
    ts = [time_of(i, W) for i in range(N_KEYS - 1) for W in WEIGHTS + tuple(int(w) for w in rng.integers(2, 255, 2))]
    return ts + [float(N_KEYS - 1)]


def _cells(vol):
    nz, ny, nx = vol.shape
    p = np.zeros(((nz + 7) // 8 * 8, (ny + 7) // 8 * 8, (nx + 7) // 8 * 8), bool)
    p[:nz, :ny, :nx] = vol != 0
    return p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8, p.shape[2] // 8, 8).any(axis=(1, 3, 5))


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_inputs_are_not_vacuous(sc, cloud16, name):
    """on the CPU, before any GPU call: for at least one tested time the in-between differs from both of its keys in at least 1 % of the
    voxels, and for at least one an 8^3 cell is occupied in a key and empty in the in-between (the occupancy has to follow q, not the keys)"""
    shape = SHAPES[name]
    keys = keys_of(cloud16, shape)
    differs = vanishes = 0
    for t in times_of(shape):
        i, W = sc.key_of_time(t, N_KEYS)
        if W in (0, 256):
            continue
        q = sc.volume_at(keys, t)
        differs = max(differs, min(float((q != keys[i]).mean()), float((q != keys[i + 1]).mean())))
        gone = (_cells(keys[i]) | _cells(keys[i + 1])) & ~_cells(q)
        vanishes = max(vanishes, int(gone.sum()))
    assert differs >= 0.01, differs
    assert vanishes >= 1


def _destroy(*pairs):
    for ren, nrc in pairs:
        ren.Destroy()
        if nrc is not None:
            nrc.Destroy()


def _as_keys(keys, source):
    import torch
    keys = np.array(keys)
    if source.startswith("f32"):      # (k + 0.5) / 255 quantises back to k (k = 255: above 1 -> 255)
        keys = (keys.astype(np.float32) + np.float32(0.5)) / np.float32(255.0)
    return torch.from_numpy(keys).cuda() if source.endswith("device") else keys


_WANT = {}


def dense_buffers(api, sc, cloud16, shape):
    """the reference of test 1, computed once per shape: the buffers after SetVolume(scene.volume_at(keys, t)) for every tested time"""
    if shape not in _WANT:
        keys = keys_of(cloud16, shape)
        ref, _ = _small(api, sc, "mc", np.zeros(shape, np.uint8))
        want = {}
        for t in times_of(shape) + [0.0]:
            ref.SetVolume(sc.volume_at(keys, t))
            want[t] = volume_buffers(ref)
        ref.Destroy()
        _WANT[shape] = want
    return _WANT[shape]


# ---------------------------------------------------------------------------------------------------------------- 1. buffers
@pytest.mark.parametrize("kind", ["nrc", "mc"])
@pytest.mark.parametrize("source", ["u8_host", "u8_device", "f32_host", "f32_device"])
def test_buffers_after_set_volume_time_equal_those_of_the_dense_call(api, sc, cloud16, torch_gpu, kind, source):
    """density, occupancy bits and boxes after SetVolumeTime(t) == those after SetVolume(scene.volume_at(keys, t)), for every key pair at
    W in {0, 1, 128, 129, 255, 256} and two seeded weights, at every shape; then slots reused back and forth, the last key, the state
    after a plain SetVolume in between, and a sequence of one key"""
    for name, shape in SHAPES.items():
        keys = keys_of(cloud16, shape)
        want = dense_buffers(api, sc, cloud16, shape)
        ren, nrc = _small(api, sc, kind, np.full(shape, 7, np.uint8))
        assert ren.VolumeKeyCount() == 0
        ren.SetVolumeKeys(_as_keys(keys, source))
        assert ren.VolumeKeyCount() == N_KEYS
        for t in times_of(shape):
            ren.SetVolumeTime(t)
            assert_same_volume(volume_buffers(ren), want[t], (name, t))
        a, b = time_of(0, 128), time_of(3, 129)
        for k in range(5):      # both slots of the NRC renderer (the one slot of the MC renderer) written over and over
            t = (a, b)[k % 2]
            ren.SetVolumeTime(t)
            assert_same_volume(volume_buffers(ren), want[t], (name, "reuse", k))
        ren.SetVolumeTime(N_KEYS - 1)
        assert_same_volume(volume_buffers(ren), want[float(N_KEYS - 1)], (name, "last key"))
        ren.SetVolumeTime(a)
        ren.SetVolume(np.array(keys[1]))
        assert_same_volume(volume_buffers(ren), want[time_of(1, 0)], (name, "dense in between"))
        ren.SetVolumeTime(a)
        assert_same_volume(volume_buffers(ren), want[a], (name, "after a dense call"))
        ren.SetVolumeKeys(_as_keys(keys[:1], source))      # a sequence of one key: time 0 is all there is
        assert ren.VolumeKeyCount() == 1
        ren.SetVolumeTime(0)
        assert_same_volume(volume_buffers(ren), want[0.0], (name, "one key"))
        with pytest.raises(RuntimeError, match="SkyRenderer ERROR"):
            ren.SetVolumeTime(0.5)
        _destroy((ren, nrc))


# ---------------------------------------------------------------------------------------------------------------- 2. F32 keys
@pytest.mark.parametrize("where", ["host", "device"])
def test_f32_keys_are_quantised_as_set_volume_quantises(api, sc, torch_gpu, where):
    """the keys read back through SetVolumeTime(i) are vol_quantize of the source: uint8(v * 255) truncated; v <= 0 and NaN -> 0,
    v >= 1 -> 255 (the values of test_gpu_volume_update.py::test_f32_quantisation)"""
    import torch
    k = np.arange(256, dtype=np.float32)
    exact = k / np.float32(255.0)
    vals = np.concatenate([exact, np.nextafter(exact, np.float32(-1)), np.nextafter(exact, np.float32(2)),
                           np.array([0.0, -0.0, 1.0, -1e-30, -0.5, -7.0, 1.0000001, 1.5, 300.0, np.nan, -np.nan, np.inf, -np.inf,
                                     1e-45, 0.9999999, 0.5, 0.003921568], np.float32)]).astype(np.float32)
    n = 16 * 16 * 16
    rng = np.random.default_rng(3)
    vol = np.concatenate([vals, rng.random(n - vals.size, dtype=np.float32) * np.float32(1.2) - np.float32(0.1)]).astype(np.float32)
    src = np.ascontiguousarray(np.stack([vol, vol[::-1]]).reshape(2, 16, 16, 16))
    with np.errstate(invalid="ignore"):
        prod = src * np.float32(255.0)
        want = np.where(~(src > 0), 0, np.where(src >= 1, 255, np.floor(np.where(np.isfinite(prod), prod, 0)))).astype(np.uint8)
    for kind in ("mc", "nrc"):
        ren, nrc = _small(api, sc, kind, np.zeros((16, 16, 16), np.uint8))
        ren.SetVolumeKeys(torch.from_numpy(src).cuda() if where == "device" else src)
        for i in range(2):
            ren.SetVolumeTime(i)
            got = ren.VolumeBuffer("density").cpu().numpy()
            assert np.array_equal(got, want[i]), (kind, i, np.nonzero(got != want[i])[0][:8])
        _destroy((ren, nrc))


# ---------------------------------------------------------------------------------------------------------------- 3. frames
def frame_keys(cloud16):
    """three keys of the fixture's own dims"""
    if "frames" not in _KEYS:
        keys = np.ascontiguousarray(np.stack([cloud16, np.roll(cloud16, (30, 20, -50), axis=(0, 1, 2)), cloud16[::-1]]))
        keys.setflags(write=False)
        _KEYS["frames"] = keys
    return _KEYS["frames"]


SIZES = [(128, 80), (100, 52), (8, 6)]


@pytest.mark.parametrize("W,H", SIZES, ids=["128x80", "ragged100x52", "tiny8x6"])
def test_mc_frame_after_set_volume_time_matches_the_oracle(api, orc, sc, cloud16, torch_gpu, W, H):
    keys = frame_keys(cloud16)
    cam = sc.make_camera(aspect=W / H)
    fr = sc.frame_randoms(2, seed=31)
    mc = api.McHpmRenderer(W, H, 8, False, cam, sc.make_scene(np.array(keys[0]), scene_id=4))
    mc.SetVolumeKeys(np.array(keys))
    mc.SetFrameRandom(fr[0])
    mc.Render()
    first = mc.GetImage().cpu().numpy().copy()
    mc.SetVolumeTime(1.5)
    mc.SetFrameRandom(fr[1])
    mc.Render()
    img = mc.GetImage().cpu().numpy()
    ref, _, _ = orc.mc_render(sc.make_scene(sc.volume_at(keys, 1.5), scene_id=4), cam, W, H, 8, fr[1], threads=8)
    assert same_bits(img, ref)
    assert not same_bits(img, first)
    mc.Destroy()


@pytest.mark.parametrize("mode", ["pipelined", "single-stream"])
@pytest.mark.parametrize("W,H", SIZES, ids=["128x80", "ragged100x52", "tiny8x6"])
def test_nrc_frames_after_set_volume_time_equal_fresh_and_dense(api, sc, cloud16, torch_gpu, monkeypatch, W, H, mode):
    """blending on: the first trained frame after SetVolumeTime(1.5) == a fresh renderer's first trained frame of volume_at(keys, 1.5) ==
    the frame after SetVolume of that volume; the trained frames that follow, the loss and the weights equal those after the dense call"""
    import torch
    if mode == "single-stream":
        nrc_debug(monkeypatch, single_stream=True, poison_alloc=True)
    keys = frame_keys(cloud16)
    vol = sc.volume_at(keys, 1.5)
    cam = sc.make_camera(aspect=W / H)
    frs = sc.frame_randoms(6, seed=32)
    state = {}
    for who in ("time", "dense", "fresh"):
        cfg = api.AppConfig(seed=42, **CFG)
        nrc = api.NeuralRadianceCache(cfg)
        ren = api.NrcHpmRenderer(W, H, True, cam, cfg, sc.make_scene(vol if who == "fresh" else np.array(keys[0]), scene_id=4), nrc)
        if who != "fresh":
            for f in range(2):      # (untrained: the three caches stay the same)
                ren.SetFrameRandom(frs[f])
                ren.Render(None, False)
        if who == "time":
            ren.SetVolumeKeys(torch.from_numpy(np.array(keys)).cuda())
            ren.SetVolumeTime(1.5)
        elif who == "dense":
            ren.SetVolume(torch.from_numpy(vol).cuda())
        imgs = []
        for f in range(2, 6 if who != "fresh" else 3):
            ren.SetFrameRandom(frs[f])
            ren.Render(None, True)
            imgs.append(ren.GetImage().cpu().numpy().copy())
        state[who] = (imgs, nrc.GetLoss(), [nrc.GetParams(k).copy() for k in range(4)], nrc.GetStep())
        ren.Destroy()
        nrc.Destroy()
    nrc_debug(monkeypatch)
    t, d, f = state["time"], state["dense"], state["fresh"]
    assert np.isfinite(t[0][0]).all()
    assert same_bits(t[0][0], f[0][0]) and same_bits(d[0][0], f[0][0])
    for k in range(4):
        assert same_bits(t[0][k], d[0][k]), k
    assert not same_bits(t[0][0], t[0][1])
    assert bits(np.float32(t[1])) == bits(np.float32(d[1])) and t[3] == d[3] == 4
    for k in range(4):
        assert np.array_equal(bits(t[2][k]), bits(d[2][k])), k


# ---------------------------------------------------------------------------------------------------------------- 4. paths
TIMES = [0.0, 0.5, 0.5, 1.25, 2.0]      # three keys; view 2 keeps view 1's medium


def views_of(sc, aspect):
    """the five views of tests/test_gpu_camera_path.py (every branch of the tile mask: partial rectangles, an eye inside the volume, a far
    eye that looks past the cloud)"""
    orbit = sc.orbit_cameras(5, radius=70.0, height=25.0, aspect=aspect)
    return [sc.make_camera(aspect=aspect), orbit[1], sc.make_camera(pos=(10.0, 0.0, 0.0), aspect=aspect),
            sc.make_camera(pos=(200.0, 0.0, 0.0), view_dir=(-1.0, 0.0, 2.5), aspect=aspect), orbit[3]]


def _make(api, sc, kind, scene, W, H, cam, blend=False, **cfg_kw):
    if kind == "mc":
        return api.McHpmRenderer(W, H, 8, blend, cam, scene), None
    kw = dict(CFG)
    kw.update(cfg_kw)
    cfg = api.AppConfig(**kw)
    nrc = api.NeuralRadianceCache(cfg)
    return api.NrcHpmRenderer(W, H, blend, cam, cfg, scene, nrc), nrc


def _render(ren, kind, train=False):
    if kind == "mc":
        ren.Render()
    else:
        ren.Render(None, train)


def _nrc_state(ren, nrc):
    return dict(image=ren.GetImage().cpu().numpy().copy(), loss=nrc.GetLoss(), step=nrc.GetStep(),
                params=[nrc.GetParams(k).copy() for k in range(4)], ring=ren.Buffer("ring").cpu().numpy().copy())


def _assert_same_state(a, b):
    assert np.isfinite(a["image"]).all()
    assert same_bits(a["image"], b["image"])
    assert bits(np.float32(a["loss"])) == bits(np.float32(b["loss"])), (a["loss"], b["loss"])
    assert a["step"] == b["step"]
    for k in range(4):
        assert np.array_equal(bits(a["params"][k]), bits(b["params"][k])), k
    assert np.array_equal(a["ring"], b["ring"])


@pytest.mark.parametrize("mode", ["pipelined", "single-stream", "q2-long-trace", "self-train"])
def test_nrc_timed_path_equals_the_loop(api, sc, cloud16, torch_gpu, monkeypatch, mode):
    """128x80, blending on, train=True, 5 views x 3 frames at TIMES: images, framebuffer, loss, step, master / EMA weights, Adam moments and
    the ring equal those of a second renderer + cache driven by SetVolumeTime / SetCamera / SetFrameRandom / Render"""
    import torch
    W, H, FPC = 128, 80, 3
    views = views_of(sc, W / H)
    frs = sc.frame_randoms(len(views) * FPC, seed=41)
    extra = {"q2-long-trace": dict(compat_fix=2, train_ray_length=32, train_spp=1), "self-train": dict(self_train=1)}.get(mode, {})
    if mode == "single-stream":
        nrc_debug(monkeypatch, single_stream=True, poison_alloc=True)
    keys = frame_keys(cloud16)
    scene = sc.make_scene(np.array(keys[2]), scene_id=4)      # (created with the medium of no view but the last)
    start = sc.make_camera(pos=(0.0, 0.0, 80.0), view_dir=(0.0, 0.0, -1.0), aspect=W / H)
    path, loop = (_make(api, sc, "nrc", scene, W, H, start, blend=True, **extra) for _ in range(2))
    for ren, _ in (path, loop):
        ren.SetVolumeKeys(torch.from_numpy(np.array(keys)).cuda())
    out = torch.full((len(views), H, W, 4), float("nan"), device="cuda")
    got = path[0].RenderPath(views, FPC, frs, train=True, out=out, times=TIMES)
    assert got is out
    want = []
    for i, v in enumerate(views):
        loop[0].SetVolumeTime(TIMES[i])
        loop[0].SetCamera(None, v)
        for k in range(FPC):
            loop[0].SetFrameRandom(frs[i * FPC + k])
            loop[0].Render(None, True)
        want.append(loop[0].GetImage().cpu().numpy().copy())
    imgs = out.cpu().numpy()
    for i in range(len(views)):
        assert same_bits(imgs[i], want[i]), i
    a, b = _nrc_state(*path), _nrc_state(*loop)
    assert a["step"] == len(views) * FPC
    _assert_same_state(a, b)
    assert same_bits(a["image"], imgs[-1])
    assert_same_volume(volume_buffers(path[0]), volume_buffers(loop[0]))
    _destroy(path, loop)
    nrc_debug(monkeypatch)


def test_mc_timed_path_equals_the_loop_and_the_oracle(api, orc, sc, cloud16, torch_gpu):
    """100x52, path length 8, 5 views x 2 frames, bitwise; view 0's image (time 0.75: a true in-between) is also the oracle's MC frame of
    that view's last random numbers on volume_at(keys, 0.75); view 1 keeps view 0's medium"""
    W, H, FPC = 100, 52, 2
    views = views_of(sc, W / H)
    frs = sc.frame_randoms(len(views) * FPC, seed=42)
    times = [0.75, 0.75, 0.0, 1.25, 2.0]
    keys = frame_keys(cloud16)
    scene = sc.make_scene(np.array(keys[2]), scene_id=4)
    path, loop = (_make(api, sc, "mc", scene, W, H, views[2]) for _ in range(2))
    for ren, _ in (path, loop):
        ren.SetVolumeKeys(np.array(keys))
    imgs = path[0].RenderPath(views, FPC, frs, times=times).cpu().numpy()
    for i, v in enumerate(views):
        loop[0].SetVolumeTime(times[i])
        loop[0].SetCamera(None, v)
        for k in range(FPC):
            loop[0].SetFrameRandom(frs[i * FPC + k])
            loop[0].Render()
        assert same_bits(imgs[i], loop[0].GetImage().cpu().numpy()), i
    assert same_bits(path[0].GetImage().cpu().numpy(), imgs[-1])
    ref, _, _ = orc.mc_render(sc.make_scene(sc.volume_at(keys, times[0]), scene_id=4), views[0], W, H, 8, frs[FPC - 1], threads=8)
    assert same_bits(imgs[0], ref)
    assert not same_bits(imgs[0], imgs[1])
    _destroy(path, loop)


@pytest.mark.parametrize("kind", ["nrc", "mc"])
def test_paths_without_times_with_equal_times_and_after_a_dense_call(api, sc, cloud16, torch_gpu, kind):
    """times=None is RenderPath as it is; all-equal times equal RenderPath after one SetVolumeTime (the rebuild is skipped from the second
    view on, and for every view when SetVolumeTime went before); a SetVolume in between makes the sequence's state unknown: the path
    rebuilds"""
    import torch
    W, H = 128, 80
    views = views_of(sc, W / H)
    frs = sc.frame_randoms(len(views), seed=43)
    keys = frame_keys(cloud16)
    scene = sc.make_scene(np.array(keys[0]), scene_id=4)
    train = kind == "nrc"

    def run(prepare, **kw):
        pair = _make(api, sc, kind, scene, W, H, views[0], blend=True, seed=42)
        pair[0].SetVolumeKeys(np.array(keys))
        prepare(pair[0])
        imgs = pair[0].RenderPath(views, 1, frs, train=train, **kw).cpu().numpy().copy()
        buf = volume_buffers(pair[0])
        _destroy(pair)
        return imgs, buf

    plain, _ = run(lambda r: None)
    none, _ = run(lambda r: None, times=None)
    assert np.isfinite(plain).all() and same_bits(plain, none)
    want, want_buf = run(lambda r: r.SetVolumeTime(0.5))
    assert not same_bits(want, plain)
    equal, buf = run(lambda r: None, times=[0.5] * len(views))
    assert same_bits(equal, want)
    assert_same_volume(buf, want_buf)
    both, _ = run(lambda r: r.SetVolumeTime(0.5), times=[0.5] * len(views))
    assert same_bits(both, want)
    other = torch.from_numpy(np.array(keys[2])).cuda()
    after_dense, buf = run(lambda r: (r.SetVolumeTime(0.5), r.SetVolume(other)), times=[0.5] * len(views))
    assert same_bits(after_dense, want)
    assert_same_volume(buf, want_buf)
    # (0, 256) and (1, 0) are one volume
    a, _ = run(lambda r: None, times=[time_of(0, 256)] * len(views))
    b, _ = run(lambda r: r.SetVolumeTime(1.0))
    assert same_bits(a, b)


@pytest.mark.parametrize("kind", ["nrc", "mc"])
def test_timed_path_frames_do_not_depend_on_the_empty_skip(api, sc, cloud16, torch_gpu, kind):
    W, H = 128, 80
    views = views_of(sc, W / H)
    frs = sc.frame_randoms(len(views), seed=44)
    keys = frame_keys(cloud16)
    scene = sc.make_scene(np.array(keys[0]), scene_id=4)
    imgs = []
    for skip in (True, False):
        pair = _make(api, sc, kind, scene, W, H, views[0])
        pair[0].SetEmptySkip(skip)
        pair[0].SetVolumeKeys(np.array(keys))
        imgs.append(pair[0].RenderPath(views, 1, frs, times=TIMES).cpu().numpy().copy())
        assert (pair[0].TileMask().size > 0) == skip
        _destroy(pair)
    assert np.isfinite(imgs[0]).all()
    assert same_bits(imgs[0], imgs[1])


# ---------------------------------------------------------------------------------------------------------------- 5. no host wait
def test_set_volume_time_and_a_timed_path_do_not_wait_for_the_gpu(api, sc, torch_gpu):
    """behind a backlog of 32 trained frames at 1080p, SetVolumeTime and a 4-view timed RenderPath return long before the backlog has run;
    the path's frames are those a second renderer on the same cache makes of the in-between volumes and views afterwards"""
    import torch
    W, H = 1920, 1080
    keys = np.ascontiguousarray(np.stack([sc.cached_volume("cloud", 128, seed=1337), sc.cached_volume("cloud", 128, seed=1338)]))
    scene = sc.make_scene(keys[0], scene_id=4)
    cfg = api.AppConfig()
    views = sc.orbit_cameras(4, radius=64.0, height=10.0, aspect=W / H)
    frs = sc.frame_randoms(4, seed=4)
    times = [0.5, 0.75, 0.75, 1.0]
    nrc = api.NeuralRadianceCache(cfg)
    ren = api.NrcHpmRenderer(W, H, False, views[0], cfg, scene, nrc)
    other = api.NrcHpmRenderer(W, H, False, views[0], cfg, scene, nrc)
    out = torch.empty((4, H, W, 4), device="cuda")
    ren.SetVolumeKeys(torch.from_numpy(keys).cuda())
    ren.SetVolumeTime(0.125)      # (first calls: the slots and the rectangle scratch are allocated, the capped states selected)
    ren.RenderPath(views[:1], 1, frs[:1], out=False, times=[0.25])
    ren.RenderFrames(sc.frame_randoms(4, seed=1), train=True)
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record(s)
    ren.RenderFrames(sc.frame_randoms(32, seed=2), train=True)
    ren.GetImage()      # (the stream waits for the last compositing on the device)
    end.record(s)
    t0 = time.perf_counter()
    ren.SetVolumeTime(0.375)
    t1 = time.perf_counter()
    ren.RenderPath(views, 1, frs, train=False, out=out, times=times)
    t2 = time.perf_counter()
    end.synchronize()
    gpu_ms = start.elapsed_time(end)
    print("SetVolumeTime returned after %.3f ms, RenderPath(times) after %.3f ms more; the backlog in front of them ran %.3f ms" %
          ((t1 - t0) * 1e3, (t2 - t1) * 1e3, gpu_ms))
    assert (t2 - t0) * 1e3 < 0.25 * gpu_ms, (t0, t1, t2, gpu_ms)
    imgs = out.cpu().numpy()      # (on the renderer's stream: ordered behind the last copy)
    assert np.isfinite(imgs).all()
    for i, v in enumerate(views):
        other.SetVolume(sc.volume_at(keys, times[i]))
        other.SetCamera(None, v)
        other.SetFrameRandom(frs[i])
        other.Render(None, False)
        assert same_bits(imgs[i], other.GetImage().cpu().numpy()), i
    ren.Destroy()
    other.Destroy()
    nrc.Destroy()


# ---------------------------------------------------------------------------------------------------------------- 6. errors
def test_errors_leave_the_renderers_and_the_keys_unchanged(api, sc, cloud16, torch_gpu):
    import torch
    W, H = 96, 54
    views = views_of(sc, W / H)
    keys = frame_keys(cloud16)
    scene = sc.make_scene(np.array(keys[0]), scene_id=4)
    frs = sc.frame_randoms(3, seed=45)
    nz, ny, nx = keys.shape[1:]
    L = api.load_library()
    INVALID = -1      # NRC_ERR_INVALID
    for kind in ("nrc", "mc"):
        used, untouched = (_make(api, sc, kind, scene, W, H, views[0], blend=True) for _ in range(2))
        for ren, _ in (used, untouched):
            ren.SetFrameRandom(frs[0])
            _render(ren, kind)
        ren = used[0]
        sym = "nrc_renderer_" if kind == "nrc" else "nrc_mc_renderer_"
        set_keys, set_time = getattr(L, sym + "set_volume_keys"), getattr(L, sym + "set_volume_time")

        def bad_calls(count):
            for t in (-0.125, count - 1 + 2.0 ** -10 if count else 0.0, float(count), float("nan"), float("inf")):
                assert set_time(ren.h, C.c_float(t)) == INVALID, t
                assert b"SkyRenderer ERROR" in L.nrc_last_error()
                with pytest.raises(RuntimeError, match="SkyRenderer ERROR"):
                    ren.SetVolumeTime(t)
            with pytest.raises(RuntimeError, match="SkyRenderer ERROR"):      # one bad time in the middle: nothing of the path is rendered
                ren.RenderPath(views[1:4], 1, frs, times=[0.0, float(count) + 3.0, 0.0])
            with pytest.raises(ValueError):
                ren.RenderPath(views[1:4], 1, frs, times=[0.0, 0.5])
            assert ren.VolumeKeyCount() == count

        bad_calls(0)      # no keys set: every time is outside
        dev = torch.from_numpy(np.array(keys)).cuda()
        ren.SetVolumeKeys(dev)      # (not an error -- and it does not touch the medium)
        bad_calls(3)
        with pytest.raises(RuntimeError, match="SkyRenderer ERROR"):      # keys of other dims
            ren.SetVolumeKeys(np.zeros((2, nz, ny, nx + 1), np.uint8))
        with pytest.raises(RuntimeError, match="SkyRenderer ERROR"):
            ren.SetVolumeKeys(np.zeros((2, nz, ny, nx), np.float64))
        assert set_keys(ren.h, None, 2, nx, ny, nz, 0, 1) == INVALID      # a NULL source
        assert b"SkyRenderer ERROR" in L.nrc_last_error()
        assert set_keys(ren.h, C.c_void_p(dev.data_ptr()), 2, nx, ny, nz, 7, 1) == INVALID      # an unknown format
        assert b"SkyRenderer ERROR" in L.nrc_last_error()
        assert ren.VolumeKeyCount() == 3
        for r, _ in (used, untouched):      # still the creation medium and the first view, blending not restarted
            r.SetFrameRandom(frs[1])
            _render(r, kind)
        assert same_bits(used[0].GetImage().cpu().numpy(), untouched[0].GetImage().cpu().numpy())
        # the previous keys are still there, whole
        used[0].SetVolumeTime(1.5)
        untouched[0].SetVolume(sc.volume_at(keys, 1.5))
        for r, _ in (used, untouched):
            r.SetFrameRandom(frs[2])
            _render(r, kind)
        assert same_bits(used[0].GetImage().cpu().numpy(), untouched[0].GetImage().cpu().numpy())
        assert_same_volume(volume_buffers(used[0]), volume_buffers(untouched[0]))
        ren.SetVolumeKeys(None)      # n_keys = 0 drops the keys; the medium stays
        bad_calls(0)
        assert_same_volume(volume_buffers(used[0]), volume_buffers(untouched[0]))
        _destroy(used, untouched)
