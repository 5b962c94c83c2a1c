"""Sparse volume keys (nrc_renderer_set_volume_key_bricks and its nrc_mc_renderer_ twin): a key sequence held as lists of 8^3 bricks.
The specification is an equivalence, and every comparison here is for equal bytes: with brick keys SetVolumeTime(t) leaves the three
device buffers a renderer with the densified keys (SetVolumeKeys) has after SetVolumeTime(t), and a timed path renders and trains the
same.  tests/test_volume_key_bricks_host.py shows on the CPU that the key sequence used here has cells with a brick in one key only, in
both and in neither."""
import ctypes as C

import numpy as np
import pytest

from key_bricks_common import N_KEYS, SHAPES, cells_of, key_bricks_of, keys_of, time_of, times_of
from volume_common import _make as _small, _to_f32, assert_same_volume, volume_buffers

pytestmark = pytest.mark.gpu

CFG = dict(train_batch_count=1, log2_train_batch_size=10, log2_infer_batch_size=14)
INVALID = -1      # NRC_ERR_INVALID


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _destroy(*pairs):
    for ren, nrc in pairs:
        ren.Destroy()
        if nrc is not None:
            nrc.Destroy()


def _as_lists(parts, source):
    """(counts, origins, bricks) as the source a test names: u8 / f32 bricks, host arrays / device tensors (counts stay on the host)"""
    import torch
    counts, origins, bricks = (np.array(p) for p in parts)
    if source.startswith("f32"):
        bricks = _to_f32(bricks)
    if source.endswith("device"):
        return counts, torch.from_numpy(origins).cuda(), torch.from_numpy(bricks).cuda()
    return counts, origins, bricks


def formula(counts, shape):
    cells = 1
    for n in shape:
        cells *= (n + 7) // 8
    return 512 * int(np.asarray(counts, np.uint64).sum()) + 4 * len(counts) * cells


_WANT = {}


def dense_twin_buffers(api, sc, cloud16, shape):
    """the reference, computed once per shape: the buffers of a renderer that holds the densified keys (SetVolumeKeys) after SetVolumeTime(t),
    for every tested time"""
    if shape not in _WANT:
        dense = sc.key_bricks_to_volumes(*key_bricks_of(sc, cloud16, shape), shape)
        assert np.array_equal(dense, keys_of(cloud16, shape))
        twin, _ = _small(api, sc, "mc", np.zeros(shape, np.uint8))
        twin.SetVolumeKeys(dense)
        assert twin.VolumeKeyBytes() == dense.nbytes
        want = {}
        for t in times_of(shape) + [0.0]:
            twin.SetVolumeTime(t)
            want[t] = volume_buffers(twin)
        twin.Destroy()
        _WANT[shape] = want
    return _WANT[shape]


# ---------------------------------------------------------------------------------------------------------------- 1. buffers
@pytest.mark.parametrize("kind", ["nrc", "mc"])
@pytest.mark.parametrize("source", ["u8_host", "u8_device", "f32_host", "f32_device"])
def test_buffers_after_set_volume_time_equal_those_of_the_dense_twin(api, sc, cloud16, torch_gpu, kind, source):
    """density, occupancy bits and boxes after SetVolumeTime(t) on brick keys == those of the dense-key twin, and the density ==
    scene.volume_at(densified keys, t): every key pair at W in {0, 1, 128, 129, 255, 256} and two seeded weights, the last key, at every
    shape; then slots reused back and forth and a sequence of one key"""
    for name, shape in SHAPES.items():
        keys = keys_of(cloud16, shape)
        parts = key_bricks_of(sc, cloud16, shape)
        want = dense_twin_buffers(api, sc, cloud16, shape)
        ren, nrc = _small(api, sc, kind, np.full(shape, 7, np.uint8))
        assert ren.VolumeKeyCount() == 0 and ren.VolumeKeyBytes() == 0
        ren.SetVolumeKeyBricks(*_as_lists(parts, source))
        assert ren.VolumeKeyCount() == N_KEYS
        assert ren.VolumeKeyBytes() == formula(parts[0], shape) == sc.key_brick_bytes(parts[0], shape)
        for t in times_of(shape):
            ren.SetVolumeTime(t)
            got = volume_buffers(ren)
            assert_same_volume(got, want[t], (name, t))
            assert np.array_equal(got["density"].reshape(shape), sc.volume_at(keys, t)), (name, t)
        a, b = time_of(0, 128), time_of(3, 129)
        for k in range(5):      # both slots of the NRC renderer (the one slot of the MC renderer) written over and over
            t = (a, b)[k % 2]
            ren.SetVolumeTime(t)
            assert_same_volume(volume_buffers(ren), want[t], (name, "reuse", k))
        first = int(parts[0][0])
        ren.SetVolumeKeyBricks(*_as_lists((parts[0][:1], parts[1][:first], parts[2][:first]), source))      # one key: time 0 is all there is
        assert ren.VolumeKeyCount() == 1 and ren.VolumeKeyBytes() == formula(parts[0][:1], shape)
        ren.SetVolumeTime(0)
        assert_same_volume(volume_buffers(ren), want[0.0], (name, "one key"))
        with pytest.raises(RuntimeError, match="SkyRenderer ERROR"):
            ren.SetVolumeTime(0.5)
        _destroy((ren, nrc))


# ---------------------------------------------------------------------------------------------------------------- 2. brick rules
def rule_lists(sc, cloud16, shape, with_invalid):
    """three keys that use every rule of a brick list: key 0 the cloud's bricks shuffled, with one cell named three times (the highest
    index has to win) and a brick of zeros on a cell nothing else names; key 1 no bricks; key 2 the synthetic key B with a zero brick
    displacing a real one (it comes later) -- and, for a device list, bricks with invalid origins spread through keys 0 and 2"""
    nz, ny, nx = shape
    keys = keys_of(cloud16, shape)
    rng = np.random.default_rng(17)
    o0, b0 = sc.volume_to_bricks(keys[0])
    perm = rng.permutation(len(o0))
    o0, b0 = o0[perm], b0[perm]
    dup = o0[3].copy()
    cz, cy, cx = (int(v[0]) for v in np.nonzero(~cells_of(keys[0])))      # (the first cell the cropped cloud leaves empty)
    empty_cell = np.array([cx * 8, cy * 8, cz * 8], np.int32)
    assert not (o0 == empty_cell).all(axis=1).any()
    o0 = np.concatenate([o0[:1], [dup], o0[1:], [dup], [empty_cell], [dup]]).astype(np.int32)
    b0 = np.concatenate([b0[:1], np.full((1, 8, 8, 8), 9, np.uint8), b0[1:], np.full((1, 8, 8, 8), 200, np.uint8), np.zeros((1, 8, 8, 8), np.uint8),
                         rng.integers(0, 256, (1, 8, 8, 8)).astype(np.uint8)])
    o2, b2 = sc.volume_to_bricks(keys[4])
    o2 = np.concatenate([o2, o2[5:6]]).astype(np.int32)
    b2 = np.concatenate([b2, np.zeros((1, 8, 8, 8), np.uint8)])
    if with_invalid:
        bad = np.array([[4, 0, 0], [0, 8, 3], [-8, 0, 0], [(nx + 7) // 8 * 8, 0, 0], [0, (ny + 7) // 8 * 8, 0], [0, 0, (nz + 7) // 8 * 8],
                        [2 ** 31 - 8, 0, 0], [0, 0, -2 ** 31]], np.int32)
        for lists in ("0", "2"):
            o, b = (o0, b0) if lists == "0" else (o2, b2)
            pos = np.sort(rng.integers(0, len(o) + 1, len(bad)))
            o, b = np.insert(o, pos, bad, axis=0), np.insert(b, pos, np.full((len(bad), 8, 8, 8), 255, np.uint8), axis=0)
            o, b = np.concatenate([o, bad[:2]]), np.concatenate([b, np.full((2, 8, 8, 8), 255, np.uint8)])      # (the highest indices too)
            if lists == "0":
                o0, b0 = o, b
            else:
                o2, b2 = o, b
    counts = np.array([len(o0), 0, len(o2)], np.uint32)
    return counts, np.ascontiguousarray(np.concatenate([o0, o2]).astype(np.int32)), np.ascontiguousarray(np.concatenate([b0, b2]))


@pytest.mark.parametrize("kind", ["nrc", "mc"])
@pytest.mark.parametrize("source", ["u8_host", "f32_host", "u8_device", "f32_device"])
def test_every_key_follows_the_rules_of_a_brick_list(api, sc, cloud16, torch_gpu, kind, source):
    """a duplicated cell (the highest index wins), a brick of zeros, a shuffled order, an empty key and -- in a device list -- invalid
    origins, which are ignored: the buffers are those of the dense twin that holds scene.key_bricks_to_volumes of the lists"""
    shape = SHAPES["61x45x70-ragged-no-vec"]
    device = source.endswith("device")
    counts, origins, bricks = rule_lists(sc, cloud16, shape, with_invalid=device)
    dense = sc.key_bricks_to_volumes(counts, origins, bricks, shape, ignore_invalid=device)
    keys = keys_of(cloud16, shape)
    # (the duplicate changed key 0 and the zero brick key 2, both in one cell only; the empty key is empty)
    assert 0 < int((dense[0] != keys[0]).sum()) <= 512 and 0 < int((dense[2] != keys[4]).sum()) <= 512 and not dense[1].any()
    twin, _ = _small(api, sc, "mc", np.zeros(shape, np.uint8))
    twin.SetVolumeKeys(dense)
    ren, nrc = _small(api, sc, kind, np.full(shape, 7, np.uint8))
    ren.SetVolumeKeyBricks(*_as_lists((counts, origins, bricks), source))
    assert ren.VolumeKeyCount() == 3 and ren.VolumeKeyBytes() == formula(counts, shape)      # (every brick is held, the displaced ones too)
    for t in (0.0, time_of(0, 1), 0.5, time_of(0, 129), time_of(0, 256), 1.0, time_of(1, 77), time_of(1, 255), 2.0):
        ren.SetVolumeTime(t)
        twin.SetVolumeTime(t)
        got = volume_buffers(ren)
        assert_same_volume(got, volume_buffers(twin), (source, t))
        assert np.array_equal(got["density"].reshape(shape), sc.volume_at(dense, t)), t
    _destroy((ren, nrc), (twin, None))


# ---------------------------------------------------------------------------------------------------------------- 3. timed paths
def frame_keys(cloud16):
    """three keys of the fixture's own dims"""
    keys = np.ascontiguousarray(np.stack([cloud16, np.roll(cloud16, (30, 20, -50), axis=(0, 1, 2)), cloud16[::-1]]))
    keys.setflags(write=False)
    return keys


# view 1 repeats view 0's (i, W); view 2 is (0, 256) and view 3 (1, 0): one volume, no rebuild between them
TIMES = [0.5, 0.5, time_of(0, 256), 1.0, 1.25]


def views_of(sc, aspect):
    orbit = sc.orbit_cameras(5, radius=70.0, height=25.0, aspect=aspect)
    return [sc.make_camera(aspect=aspect), orbit[1], sc.make_camera(pos=(10.0, 0.0, 0.0), aspect=aspect),
            sc.make_camera(pos=(200.0, 0.0, 0.0), view_dir=(-1.0, 0.0, 2.5), aspect=aspect), orbit[3]]


def _make(api, sc, kind, scene, W, H, cam, blend=False):
    if kind == "mc":
        return api.McHpmRenderer(W, H, 8, blend, cam, scene), None
    cfg = api.AppConfig(**CFG)
    nrc = api.NeuralRadianceCache(cfg)
    return api.NrcHpmRenderer(W, H, blend, cam, cfg, scene, nrc), nrc


def test_nrc_timed_path_from_brick_keys_equals_the_one_from_dense_keys(api, sc, cloud16, torch_gpu):
    """128x80, blending on, train=True, 5 views x 2 frames at TIMES: images, loss, step, weights (master, EMA, Adam moments) and the ring
    equal, by bits, those of a second renderer + cache that holds the same keys dense"""
    import torch
    W, H, FPC = 128, 80, 2
    views = views_of(sc, W / H)
    frs = sc.frame_randoms(len(views) * FPC, seed=51)
    keys = frame_keys(cloud16)
    scene = sc.make_scene(np.array(keys[2]), scene_id=4)
    start = sc.make_camera(pos=(0.0, 0.0, 80.0), view_dir=(0.0, 0.0, -1.0), aspect=W / H)
    sparse, dense = (_make(api, sc, "nrc", scene, W, H, start, blend=True) for _ in range(2))
    counts, origins, bricks = sc.volumes_to_key_bricks(keys)
    sparse[0].SetVolumeKeyBricks(counts, torch.from_numpy(origins).cuda(), torch.from_numpy(bricks).cuda())
    dense[0].SetVolumeKeys(torch.from_numpy(np.array(keys)).cuda())
    assert sparse[0].VolumeKeyBytes() == formula(counts, cloud16.shape) < dense[0].VolumeKeyBytes() == keys.nbytes
    imgs = [r.RenderPath(views, FPC, frs, train=True, times=TIMES).cpu().numpy().copy() for r, _ in (sparse, dense)]
    assert np.isfinite(imgs[0]).all()
    for i in range(len(views)):
        assert same_bits(imgs[0][i], imgs[1][i]), i
    assert not same_bits(imgs[0][3], imgs[0][4])
    state = [dict(image=r.GetImage().cpu().numpy().copy(), loss=n.GetLoss(), step=n.GetStep(), params=[n.GetParams(k).copy() for k in range(4)],
                  ring=r.Buffer("ring").cpu().numpy().copy()) for r, n in (sparse, dense)]
    a, b = state
    assert a["step"] == b["step"] == len(views) * FPC
    assert same_bits(a["image"], b["image"]) and same_bits(a["image"], imgs[0][-1])
    assert bits(np.float32(a["loss"])) == bits(np.float32(b["loss"])), (a["loss"], b["loss"])
    for k in range(4):
        assert np.array_equal(bits(a["params"][k]), bits(b["params"][k])), k
    assert np.array_equal(a["ring"], b["ring"])
    assert_same_volume(volume_buffers(sparse[0]), volume_buffers(dense[0]))
    _destroy(sparse, dense)


def test_mc_timed_path_from_brick_keys_equals_the_one_from_dense_keys(api, sc, cloud16, torch_gpu):
    W, H, FPC = 100, 52, 2
    views = views_of(sc, W / H)
    frs = sc.frame_randoms(len(views) * FPC, seed=52)
    keys = frame_keys(cloud16)
    scene = sc.make_scene(np.array(keys[2]), scene_id=4)
    sparse, dense = (_make(api, sc, "mc", scene, W, H, views[2]) for _ in range(2))
    sparse[0].SetVolumeKeyBricks(*sc.volumes_to_key_bricks(keys))
    dense[0].SetVolumeKeys(np.array(keys))
    imgs = [r.RenderPath(views, FPC, frs, times=TIMES).cpu().numpy().copy() for r, _ in (sparse, dense)]
    assert np.isfinite(imgs[0]).all()
    for i in range(len(views)):
        assert same_bits(imgs[0][i], imgs[1][i]), i
    assert not same_bits(imgs[0][3], imgs[0][4])
    assert_same_volume(volume_buffers(sparse[0]), volume_buffers(dense[0]))
    _destroy(sparse, dense)


# ---------------------------------------------------------------------------------------------------------------- 4. bytes and kinds
@pytest.mark.parametrize("kind", ["nrc", "mc"])
def test_one_sequence_dense_or_bricks_and_the_rebuild_rule(api, sc, cloud16, torch_gpu, kind):
    """dense after bricks and bricks after dense replace each other (count and bytes follow, the medium is untouched by the setters);
    SetVolume and SetVolumeBricks between two equal times make the sequence's state unknown: the second SetVolumeTime rebuilds"""
    shape = SHAPES["61x45x70-ragged-no-vec"]
    keys = keys_of(cloud16, shape)
    parts = key_bricks_of(sc, cloud16, shape)
    want = dense_twin_buffers(api, sc, cloud16, shape)
    t = time_of(0, 128)
    ren, nrc = _small(api, sc, kind, np.full(shape, 7, np.uint8))
    created = volume_buffers(ren)
    ren.SetVolumeKeyBricks(*(np.array(p) for p in parts))
    assert (ren.VolumeKeyCount(), ren.VolumeKeyBytes()) == (N_KEYS, formula(parts[0], shape))
    assert_same_volume(volume_buffers(ren), created, "the setter does not touch the medium")
    ren.SetVolumeTime(t)
    assert_same_volume(volume_buffers(ren), want[t], "bricks")
    ren.SetVolumeKeys(np.array(keys[:3]))      # dense replaces bricks
    assert (ren.VolumeKeyCount(), ren.VolumeKeyBytes()) == (3, 3 * keys[0].size)
    assert_same_volume(volume_buffers(ren), want[t], "the setter does not touch the medium")
    ren.SetVolumeTime(time_of(1, 0))
    assert_same_volume(volume_buffers(ren), want[time_of(1, 0)], "dense after bricks")
    with pytest.raises(RuntimeError, match="SkyRenderer ERROR"):      # (three keys now: key 3 is gone)
        ren.SetVolumeTime(time_of(3, 129))
    ren.SetVolumeKeyBricks(*(np.array(p) for p in parts))      # bricks replace dense
    assert (ren.VolumeKeyCount(), ren.VolumeKeyBytes()) == (N_KEYS, formula(parts[0], shape))
    ren.SetVolumeTime(time_of(3, 129))
    assert_same_volume(volume_buffers(ren), want[time_of(3, 129)], "bricks after dense")
    # a dense call and a brick call between two equal times
    ren.SetVolumeTime(t)
    ren.SetVolume(np.array(keys[1]))
    assert_same_volume(volume_buffers(ren), want[time_of(1, 0)], "SetVolume in between")
    ren.SetVolumeTime(t)
    assert_same_volume(volume_buffers(ren), want[t], "after SetVolume")
    ren.SetVolumeBricks(*sc.volume_to_bricks(keys[1]))
    assert_same_volume(volume_buffers(ren), want[time_of(1, 0)], "SetVolumeBricks in between")
    ren.SetVolumeTime(t)
    assert_same_volume(volume_buffers(ren), want[t], "after SetVolumeBricks")
    # (the last key through its resident index, after the brick call used the renderer's own index buffer)
    ren.SetVolumeTime(N_KEYS - 1)
    assert_same_volume(volume_buffers(ren), want[float(N_KEYS - 1)], "last key")
    ren.SetVolumeKeyBricks(None, None, None)      # n_keys = 0 drops the sequence; the medium stays
    assert (ren.VolumeKeyCount(), ren.VolumeKeyBytes()) == (0, 0)
    assert_same_volume(volume_buffers(ren), want[float(N_KEYS - 1)], "dropped")
    with pytest.raises(RuntimeError, match="SkyRenderer ERROR"):
        ren.SetVolumeTime(0.0)
    ren.SetVolumeKeyBricks([0, 0], np.zeros((0, 3), np.int32), np.zeros((0, 8, 8, 8), np.uint8))      # keys without a brick: the empty medium
    assert (ren.VolumeKeyCount(), ren.VolumeKeyBytes()) == (2, formula([0, 0], shape))
    ren.SetVolumeTime(0.5)
    assert_same_volume(volume_buffers(ren), want[time_of(2, 0)], "two empty keys")      # (key 2 is the all-zero key)
    _destroy((ren, nrc))


# ---------------------------------------------------------------------------------------------------------------- 5. failures
@pytest.mark.parametrize("previous", ["bricks", "dense"])
def test_failures_leave_the_renderers_and_the_previous_sequence_unchanged(api, sc, cloud16, torch_gpu, previous):
    """a bad host origin (the message names the key and the brick), NULL pointers and an unknown format: the previous sequence, of either
    kind, the buffers and a frame are afterwards what an untouched renderer has, by bits"""
    import torch
    W, H = 96, 54
    shape = cloud16.shape
    nz, ny, nx = shape
    keys = frame_keys(cloud16)
    counts, origins, bricks = sc.volumes_to_key_bricks(keys)
    scene = sc.make_scene(np.array(keys[0]), scene_id=4)
    cam = sc.make_camera(aspect=W / H)
    frs = sc.frame_randoms(3, seed=53)
    L = api.load_library()
    for kind in ("nrc", "mc"):
        used, untouched = (_make(api, sc, kind, scene, W, H, cam, blend=True) for _ in range(2))

        def render(k):
            out = []
            for r, _ in (used, untouched):
                r.SetFrameRandom(frs[k])
                if kind == "mc":
                    r.Render()
                else:
                    r.Render(None, False)
                out.append(r.GetImage().cpu().numpy().copy())
            return out

        for r, _ in (used, untouched):
            if previous == "bricks":
                r.SetVolumeKeyBricks(counts, origins, bricks)
            else:
                r.SetVolumeKeys(np.array(keys))
        held = untouched[0].VolumeKeyBytes()
        assert held == (formula(counts, shape) if previous == "bricks" else keys.nbytes)
        first = render(0)
        assert same_bits(*first)
        ren = used[0]
        fn = getattr(L, ("nrc_renderer_" if kind == "nrc" else "nrc_mc_renderer_") + "set_volume_key_bricks")
        first1 = int(counts[0])
        bad_origins = {"unaligned": [8, 12, 8], "x out of range": [(nx + 7) // 8 * 8, 0, 0], "z out of range": [0, 0, (nz + 7) // 8 * 8],
                       "negative": [-8, 0, 0]}
        for name, o in bad_origins.items():      # key 1's brick 2
            bad = origins.copy()
            bad[first1 + 2] = o
            with pytest.raises(RuntimeError, match=r"SkyRenderer ERROR.*key 1, brick 2 has origin \(%d, %d, %d\)" % tuple(o)):
                ren.SetVolumeKeyBricks(counts, bad, bricks)
            with pytest.raises(RuntimeError, match="SkyRenderer ERROR.*key 1, brick 2"):
                ren.SetVolumeKeyBricks(counts, bad, _to_f32(bricks))
        p_counts, p_origins, p_bricks = (C.c_void_p(a.ctypes.data) for a in (counts, origins, bricks))
        d_origins, d_bricks = torch.from_numpy(origins).cuda(), torch.from_numpy(bricks).cuda()
        calls = {"unknown format": (p_counts, p_origins, p_bricks, 3, 7, 0), "NULL counts": (None, p_origins, p_bricks, 3, 0, 0),
                 "NULL origins": (p_counts, None, p_bricks, 3, 0, 0), "NULL bricks": (p_counts, p_origins, None, 3, 0, 0),
                 "NULL device bricks": (p_counts, C.c_void_p(d_origins.data_ptr()), None, 3, 1, 1),
                 "NULL device origins": (p_counts, None, C.c_void_p(d_bricks.data_ptr()), 3, 0, 1),
                 "unknown format, device": (p_counts, C.c_void_p(d_origins.data_ptr()), C.c_void_p(d_bricks.data_ptr()), 3, -1, 1)}
        for name, a in calls.items():
            assert fn(ren.h, *a) == INVALID, name
            assert b"SkyRenderer ERROR: set_volume_key_bricks" in L.nrc_last_error(), name
        with pytest.raises(RuntimeError, match="SkyRenderer ERROR"):      # counts that do not add up to the lists
            ren.SetVolumeKeyBricks(counts[:2], origins, bricks)
        assert ren.VolumeKeyCount() == 3 and ren.VolumeKeyBytes() == held
        # still the creation medium, blending not restarted
        assert same_bits(*render(1))
        assert_same_volume(volume_buffers(used[0]), volume_buffers(untouched[0]), "medium")
        # the previous sequence is still there, whole
        for r, _ in (used, untouched):
            r.SetVolumeTime(1.5)
        assert same_bits(*render(2))
        assert_same_volume(volume_buffers(used[0]), volume_buffers(untouched[0]), "in-between")
        assert np.array_equal(volume_buffers(used[0])["density"].reshape(shape), sc.volume_at(keys, 1.5))
        _destroy(used, untouched)


# ---------------------------------------------------------------------------------------------------------------- 6. CLI
def test_cli_animate_sparse_keys_renders_what_dense_keys_of_the_same_lists_render(api, sc, torch_gpu, tmp_path, capsys):
    """`--orbit 3 --vdb a b a --animate --sparse-keys`: the run holds the files as brick keys (the byte counts it prints are the formula's)
    and every view's exported image is, by bits, what a renderer of the same configuration renders from the densified lists as dense keys"""
    import os

    from conftest import GOLDEN
    from nrc_hpm_renderer_amd import cli, io_exr, io_vdb
    vdb = os.path.join(GOLDEN, "cloud_sixteenth_excerpt.vdb")
    W, H, FRAMES, VIEWS = 128, 80, 2, 3
    config = ["RelativeL2Luminance", "Adam", "0.01", "0.99", "3", "0", "64", "6", "14", "10", "1", "4", "1.0", "1", "1", "0.0", "32"]
    pattern = str(tmp_path / "view_%02d.exr")
    argv = config + ["--frames", str(FRAMES), "--width", str(W), "--height", str(H), "--orbit", str(VIEWS), "--vdb", vdb, vdb, vdb, "--animate",
                     "--sparse-keys", "--time-scale", "0.75", "--output", str(tmp_path / "output"), "--export", pattern]
    assert cli.main(argv) == 0
    out = capsys.readouterr().out
    bbox = io_vdb.aligned_bbox(io_vdb.union_bbox([vdb]))
    dims = tuple(int(hi - lo + 1) for lo, hi in zip(bbox[0], bbox[1]))[::-1]
    origins, bricks = io_vdb.read_vdb_bricks(vdb, bbox)
    held, dense = formula([len(origins)] * 3, dims), 3 * dims[0] * dims[1] * dims[2]
    assert "3 keys, %d bricks: %d bytes on the device as brick keys; dense keys %d bytes" % (3 * len(origins), held, dense) in out, out
    assert held < dense
    key = (sc.bricks_to_volume(origins, bricks, dims) * np.float32(255.0)).astype(np.uint8)
    cfg = api.AppConfig(["NRC-HPM-Renderer"] + config)
    nrc = api.NeuralRadianceCache(cfg)
    ren = api.NrcHpmRenderer(W, H, False, sc.make_camera(aspect=W / H), cfg, sc.make_scene(key, scene_id=cfg.scene_id), nrc)
    ren.SetVolumeKeys(np.ascontiguousarray(np.stack([key] * 3)))
    views = sc.orbit_cameras(VIEWS, 64.0, 0.0, aspect=W / H)
    want = ren.RenderPath(views, FRAMES, train=True, times=cli.animate_times(VIEWS, 3, 0.75)).cpu().numpy()
    for v in range(VIEWS):
        got = io_exr.read_exr(pattern % v)
        assert got.shape == (H, W, 4) and np.isfinite(got).all()
        assert same_bits(got, want[v]), v
    assert not same_bits(want[0], want[1])
    _destroy((ren, nrc))
