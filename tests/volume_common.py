"""What the GPU tests of the volume setters share (test_gpu_volume_update.py, test_gpu_volume_bricks.py, test_gpu_volume_keys.py): the
three device buffers of a renderer's volume compared bit for bit, small renderers, and common volumes."""
import numpy as np


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def volume_buffers(ren):
    return {k: ren.VolumeBuffer(k).cpu().numpy().copy() for k in ("density", "occ_bits", "boxes")}


def assert_same_volume(got, want, name=""):
    assert np.array_equal(got["density"], want["density"]), name
    assert np.array_equal(got["occ_bits"], want["occ_bits"]), name
    assert got["boxes"].shape == want["boxes"].shape, (name, got["boxes"].shape, want["boxes"].shape)
    assert np.array_equal(got["boxes"].view(np.uint32), want["boxes"].view(np.uint32)), name


def _make(api, sc, kind, vol, W=32, H=16):
    scene = sc.make_scene(vol, scene_id=4)
    cam = sc.make_camera(aspect=W / H)
    if kind == "mc":
        return api.McHpmRenderer(W, H, 8, False, cam, scene), None
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=8, log2_infer_batch_size=12)
    nrc = api.NeuralRadianceCache(cfg)
    return api.NrcHpmRenderer(W, H, False, cam, cfg, scene, nrc), nrc


def _sparse_512():
    """[nz][ny][nx] = 160 x 512 x 512: 64 x 64 x 20 cells of 8 voxels would not fit the LDS table (16-voxel occupancy cells)"""
    rng = np.random.default_rng(11)
    v = np.zeros((160, 512, 512), np.uint8)
    idx = rng.integers(0, v.size, 4000)
    v.reshape(-1)[idx] = rng.integers(1, 256, idx.size).astype(np.uint8)
    v[40:56, 100:140, 300:331] = 90       # a block across cell borders
    return v


def _to_f32(u8):
    """(k + 0.5) / 255 quantises back to k (k = 255: above 1 -> 255)"""
    return ((u8.astype(np.float32) + np.float32(0.5)) / np.float32(255.0)).astype(np.float32)
