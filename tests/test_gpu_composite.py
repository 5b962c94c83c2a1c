"""k_composite (nrc/render.comp) to the bit.  The kernel is compiled without floating-point contraction, so given the device's own
primary colour / throughput, didScatter image and inferred radiance of a frame, the framebuffer is defined exactly: the tests read those
three buffers back after every frame, apply tests/image_reference.py's composite_fp32 to them -- chained on the REFERENCE's previous image,
never on the device's -- and require GetImage() to equal the result bit for bit.  That sees what the oracle-pipeline tests' slack (the
oracle's radiance differs from the device's by ~5e-5) hides: the clamp fmax(0, y), the info == 1 gate, the throughput factor p.w, the
tile-major addressing of the radiance (query_index), the blend chain 1/k and the alpha channel.

The weights are randomised first, so that the cache's radiance is negative at some scattered pixels and positive at others (asserted): the
clamp is exercised.  cloud16, scene 4 under a procedural sky, 2^8 train rays."""
import numpy as np
import pytest

import image_reference as ir
from conftest import nrc_debug

pytestmark = pytest.mark.gpu

f32 = np.float32
FUSED = (3, 0, 64, 6, 0)      # pos_id, dir_id, width, depth, hashgrid_log2_size


def randomize(nrc, seed=5, scale=1.5, noise=0.01):
    """non-trivial asymmetric weights (EMA != master), the way test_gpu_mlp.py::randomize sets them"""
    rng = np.random.default_rng(seed)
    n = nrc.ParamCount()
    w = (np.array(nrc.GetParams(0)) * scale + (rng.standard_normal(n) * noise).astype(f32)).astype(f32)
    e = (w + (rng.standard_normal(n) * 0.02).astype(f32)).astype(f32)
    nrc.SetParams(0, w)
    nrc.SetParams(1, e)
    return w, e


def setup(api, sc, cloud16, W, H, model=FUSED, tile=None, aspect=None, infer_log2=12, poison=None):
    scene = sc.make_scene(cloud16, scene_id=4, env=sc.procedural_sky(64, 32))
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=8, log2_infer_batch_size=infer_log2, pos_id=model[0], dir_id=model[1],
                        nn_width=model[2], nn_depth=model[3], hashgrid_log2_size=model[4])
    nrc = api.NeuralRadianceCache(cfg)
    # (a HashGrid table starts at +-1e-4: with the small noise the position would not reach the output, and the radiance of a whole view has
    # one sign -- the larger noise makes it vary from pixel to pixel)
    w, e = randomize(nrc, noise=0.3 if model[0] == 0 else 0.01)
    if poison is not None:
        for v, which in ((w, 0), (e, 1)):
            v[poison] = np.nan
            nrc.SetParams(which, v)
    cam = sc.make_camera(aspect=aspect or W / H)
    ren = api.NrcHpmRenderer(W, H, False, cam, cfg, scene, nrc, tile=tile)
    return nrc, ren


def buffers(ren, W, H):
    """the last frame's primary [H][W][4], info [H][W] and radiance [W * H][3] (x * H + y order), as the device holds them"""
    return (ren.Buffer("primary").cpu().numpy().reshape(H, W, 4).copy(), ren.Buffer("info").cpu().numpy().reshape(H, W).copy(),
            ren.Buffer("infer_output").cpu().numpy().reshape(W * H, 3).copy())


def radiance_signs(info, y, W, H):
    """(scattered pixels with a negative radiance channel, with a positive one, with a NaN one)"""
    live = y.reshape(W, H, 3).transpose(1, 0, 2)[info == f32(1.0)]
    return int((live < 0).any(axis=1).sum()), int((live > 0).any(axis=1).sum()), int(np.isnan(live).any(axis=1).sum())


class Chain:
    """one renderer's frames and the reference image chained beside them"""

    def __init__(self, ren, W, H):
        self.ren, self.W, self.H = ren, W, H
        self.want = np.zeros((H, W, 4), f32)
        self.neg = self.pos = 0

    def frame(self, fr, k, train=True, show_nrc=1):
        """render one frame whose blend factor is 1 / k and compare"""
        self.ren.SetFrameRandom(fr)
        self.ren.Render(None, train)
        return self.check(k, show_nrc)

    def check(self, k, show_nrc=1):
        img = self.ren.GetImage().cpu().numpy().copy()
        p, info, y = buffers(self.ren, self.W, self.H)
        self.want = ir.composite_fp32(p, info, y, self.want, f32(1.0) / f32(k), show_nrc)
        bad = (img.view(np.uint32) != self.want.view(np.uint32)) & ~(np.isnan(img) & np.isnan(self.want))
        assert not bad.any(), "%d of %d pixels differ from the fp32 statement, first at %s" % (
            bad.any(axis=2).sum(), self.W * self.H, np.argwhere(bad)[0])
        assert (img[..., 3] == 1.0).all()
        neg, pos, _ = radiance_signs(info, y, self.W, self.H)
        self.neg, self.pos = self.neg + neg, self.pos + pos
        return img, (p, info, y)

    def clamp_was_exercised(self):
        assert self.neg > 0 and self.pos > 0, (self.neg, self.pos)


def test_blend_chain_trained_then_unblended_then_without_the_cache(api, sc, cloud16, torch_gpu):
    """100 x 52 (ragged 8 x 8 tiles, two inference batches of 2^12): four trained frames blended 1, 1/2, 1/3, 1/4; blending off (factor 1);
    the cache switched off (primary colour only)"""
    W, H = 100, 52
    nrc, ren = setup(api, sc, cloud16, W, H)
    ren.SetBlend(True)
    ch = Chain(ren, W, H)
    frs = sc.frame_randoms(6, seed=41)
    for k in range(1, 5):
        img, (p, info, y) = ch.frame(frs[k - 1], k)
    assert 0.05 * W * H < (info == 1.0).sum() < 0.95 * W * H      # both sides of the gate
    assert not ir.same_bits(img, ir.composite_fp32(p, info, y, np.zeros_like(img), 1.0, 1))      # (the chain matters)
    ren.SetBlend(False)
    img, (p, info, y) = ch.frame(frs[4], 1)
    live = info == 1.0
    assert not ir.same_bits(img[live][:, :3], p[live][:, :3])      # the cache's radiance is in the picture
    ren.SetShowNrc(False)
    img, (p, info, y) = ch.frame(frs[5], 1, show_nrc=0)
    assert ir.same_bits(img[..., :3], p[..., :3])
    ch.clamp_was_exercised()
    ren.Destroy()
    nrc.Destroy()


def test_tiny_frame(api, sc, cloud16, torch_gpu):
    """8 x 6: one partial tile"""
    W, H = 8, 6
    nrc, ren = setup(api, sc, cloud16, W, H)
    ren.SetBlend(True)
    ch = Chain(ren, W, H)
    frs = sc.frame_randoms(2, seed=43)
    for k in (1, 2):
        ch.frame(frs[k - 1], k)
    ch.clamp_was_exercised()
    ren.Destroy()
    nrc.Destroy()


@pytest.mark.parametrize("no_list", [False, True], ids=["live-list", "no-live-list"])
@pytest.mark.parametrize("model", [(2, 2, 64, 3, 0), (3, 0, 128, 2, 0), (0, 0, 64, 2, 11)], ids=["generic", "enc80-128", "hashgrid"])
def test_every_inference_writer(api, sc, cloud16, torch_gpu, model, no_list, monkeypatch):
    """the radiance compositing reads is written by k_infer_gen, the enc80 / 128-wide kernel or the HashGrid path, from the frame's
    live-query list (one inference batch) or without it (NRC_DEBUG=no_live_list): 128 x 80, two blended frames each"""
    W, H = 128, 80
    nrc_debug(monkeypatch, no_live_list=no_list)
    nrc, ren = setup(api, sc, cloud16, W, H, model=model, infer_log2=21)
    ren.SetBlend(True)
    ch = Chain(ren, W, H)
    frs = sc.frame_randoms(2, seed=45)
    for k in (1, 2):
        ch.frame(frs[k - 1], k, train=False)
    ch.clamp_was_exercised()
    ren.Destroy()
    nrc.Destroy()


def test_column_tile(api, sc, cloud16, torch_gpu):
    """tile 1 of 3 of a 200-wide frame: the radiance is addressed by the tile's LOCAL columns"""
    from nrc_hpm_renderer_amd import parallel
    GW, H = 200, 96
    W = parallel.local_width(1, 3, GW)
    assert W == 64
    nrc, ren = setup(api, sc, cloud16, W, H, tile=parallel.column_tile(1, 3, GW, H), aspect=GW / H)
    ren.SetBlend(True)
    ch = Chain(ren, W, H)
    frs = sc.frame_randoms(2, seed=47)
    for k in (1, 2):
        ch.frame(frs[k - 1], k)
    ch.clamp_was_exercised()
    ren.Destroy()
    nrc.Destroy()


def test_deferred_compositing(api, sc, cloud16, torch_gpu):
    """RenderFrames with the schedule's composite_defer on: frames 1 and 2 are composited with the frame after them, on another stream.
    The reference is chained from single Render calls of a second renderer on an identically randomised cache; the image after three
    trained, blended frames equals it, and equals one more reference step from the RenderFrames renderer's own last-frame buffers"""
    W, H = 100, 52
    frs = sc.frame_randoms(3, seed=49)
    nrc_b, ren_b = setup(api, sc, cloud16, W, H)
    ren_b.SetBlend(True)
    ch = Chain(ren_b, W, H)
    for k in (1, 2):
        ch.frame(frs[k - 1], k)
    after_two = ch.want.copy()
    ch.frame(frs[2], 3)
    ch.clamp_was_exercised()

    nrc_a, ren_a = setup(api, sc, cloud16, W, H)
    ren_a.SetSchedule(composite_defer=1)
    assert ren_a.GetSchedule()["composite_defer"] == 1
    ren_a.SetBlend(True)
    ren_a.RenderFrames(frs, True)
    img = ren_a.GetImage().cpu().numpy().copy()
    assert ir.same_bits(img, ch.want)
    p, info, y = buffers(ren_a, W, H)
    assert ir.same_bits(img, ir.composite_fp32(p, info, y, after_two, f32(1.0) / f32(3.0), 1))
    for x in (ren_a, ren_b, nrc_a, nrc_b):
        x.Destroy()


def test_nan_radiance_adds_nothing(api, sc, cloud16, torch_gpu):
    """output-layer weights of the EMA and master vectors set to NaN -- one per output channel (a weight of the output matrix reaches one
    channel only) in either orientation of the matrix: every channel of every scattered pixel's radiance is NaN, fmax(0, NaN) = 0, and
    the image is the primary colour -- the show_nrc = 0 composite -- bit for bit, and finite"""
    W, H = 100, 52
    first = -3 * 64                                     # (from the end of the vector)
    poison = [first, first + 1, first + 2, first + 64, first + 128]
    nrc, ren = setup(api, sc, cloud16, W, H, poison=poison)
    assert nrc.ParamCount() == 25792                    # no table behind the MLP: the output matrix is the last 3 x 64 numbers
    assert np.isnan(nrc.GetParams(1)[poison]).all() and np.isnan(nrc.GetParams(0)[poison]).all()
    ren.SetFrameRandom(sc.frame_randoms(1, seed=51)[0])
    ren.Render(None, False)
    img = ren.GetImage().cpu().numpy().copy()
    p, info, y = buffers(ren, W, H)
    live = y.reshape(W, H, 3).transpose(1, 0, 2)[info == 1.0]
    assert live.shape[0] > 500 and np.isnan(live).all(), (live.shape, np.isnan(live).mean(axis=0))
    zero = np.zeros((H, W, 4), f32)
    assert ir.same_bits(img, ir.composite_fp32(p, info, y, zero, 1.0, 0)) and np.isfinite(img).all()
    assert np.array_equal(img.view(np.uint32), ir.composite_fp32(p, info, y, zero, 1.0, 1).view(np.uint32))
    ren.Destroy()
    nrc.Destroy()
