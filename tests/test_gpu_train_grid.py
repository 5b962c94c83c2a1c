"""The train-ray path -- k_gen_rays' on-grid vertex store, k_train_scan, k_prep_train<0|1|2>, k_ring_push -- against the oracle and the ring
model of tests/train_grid_cases.py at every train-grid shape of its table: grids with partial 16x16 / 8x8 tiles, T no multiple of 128, tall
and square frames, x_dist != y_dist, grids that overshoot the frame, scan threads that own 2, 3, 4 and 80 train indices or none, rings
larger than T, of a tenth of a frame's pushes, and of size 0.  Everything is bit for bit: the path is specified fp32 arithmetic."""
import os
import subprocess
import sys

import numpy as np
import pytest

import train_grid_cases as tc
from conftest import nrc_debug

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def config_of(case, long_paths=False, **kw):
    c = dict(train_batch_count=case["count"], log2_train_batch_size=case["log2"], log2_infer_batch_size=14, compat_fix=case["fix_q1"],
             train_ring_buf_size=case["frac"], scene_id=4)
    if long_paths:                                # quirk Q2 fixed: 4 vertices x 2 samples, the 32-rays-per-wave kernels
        c.update(compat_fix=2 | case["fix_q1"], train_ray_length=4, train_spp=2)
    c.update(kw)
    return c


def setup(api, case, **cfg_kw):
    cfg = api.AppConfig(**cfg_kw)
    nrc = api.NeuralRadianceCache(cfg)
    ren = api.NrcHpmRenderer(case["W"], case["H"], False, tc.make_camera(case), cfg, tc.make_scene(case), nrc)
    return nrc, ren


def ring_of(ren):
    """(head, tail, entries [max(T, ring_size)][6]) of the renderer's ring"""
    rb = ren.Buffer("ring").cpu().numpy()
    return int(rb[0].view(np.uint32)), int(rb[1].view(np.uint32)), rb[2:].view(np.float32).reshape(-1, 6)


def check_frame(ren, name, f, want, model):
    """after frame f of case `name`: train data and ring against the oracle's frame `want` and the ring model's frame `model`"""
    assert same_bits(ren.Buffer("train_input").cpu().numpy(), want["tin"]), (name, f)
    assert same_bits(ren.Buffer("train_target").cpu().numpy(), want["tgt"]), (name, f)
    head, tail, entries = ring_of(ren)
    assert (head, tail) == tuple(want["head_tail"]) == tuple(model["head_tail"]), (name, f)
    assert same_bits(entries, want["ring"]) and same_bits(entries, model["ring"]), (name, f)


@pytest.mark.parametrize("name", list(tc.CASES))
def test_train_rays_and_ring_match_oracle_at_every_grid(api, orc, torch_gpu, name):
    case, g = tc.CASES[name], tc.case_grid(tc.CASES[name])
    nrc, ren = setup(api, case, **config_of(case))
    assert ren.TrainGrid() == g
    gens, frames = tc.oracle_frames(orc, name)
    models = tc.model_frames(name)
    for f, fr in enumerate(tc.frame_randoms(case)):
        ren.SetFrameRandom(fr)
        ren.Render(None, False)
        check_frame(ren, name, f, frames[f], models[f])
        if name == "Z":                            # no ring: no kernel writes train data or moves head / tail
            ring, _ = tc.new_ring(g)
            head, tail, entries = ring_of(ren)
            assert head == 0 and tail == 0 and same_bits(entries, ring)
            assert not ren.Buffer("train_input").cpu().numpy().any() and not ren.Buffer("train_target").cpu().numpy().any()
    ren.Destroy()
    nrc.Destroy()


@pytest.mark.parametrize("name", ["A-tall", "SQ", "C1", "D", "TALL2"])
def test_vertex_images_hold_exactly_the_grid_pixels(api, orc, torch_gpu, name):
    """k_gen_rays' on_grid: origin and direction are stored at the scattered train pixels inside the frame and nowhere else, also where
    x_dist != y_dist and where the grid's last rows lie below the frame"""
    case, g = tc.CASES[name], tc.case_grid(tc.CASES[name])
    W, H = case["W"], case["H"]
    nrc, ren = setup(api, case, **config_of(case))
    o = tc.gen_rays_of(orc, name, case)[0]
    ren.SetFrameRandom(tc.frame_randoms(case)[0])
    ren.Render(None, False)
    assert ren.VertexImageBytes() == g["tw"] * g["th"] * 32
    gy, gx, inside = tc.train_pixels(g, W, H)
    gy, gx = gy[inside], gx[inside]
    on = o["info"][gy, gx] == 1
    assert on.any() and not on.all()
    org = ren.Buffer("origin").cpu().numpy().reshape(H, W, 4)
    drc = ren.Buffer("dir").cpu().numpy().reshape(H, W, 4)
    assert same_bits(org[gy[on], gx[on]], o["origin"][gy[on], gx[on]]) and same_bits(drc[gy[on], gx[on]], o["dir"][gy[on], gx[on]])
    elsewhere = np.ones((H, W), bool)
    elsewhere[gy[on], gx[on]] = False
    assert (org[elsewhere] == 0).all() and (drc[elsewhere] == 0).all()
    assert same_bits(ren.Buffer("info").cpu().numpy().reshape(H, W), o["info"])
    ren.Destroy()
    nrc.Destroy()


def zero_output_layer(nrc, width=64):
    """the output matrix is the last 3 x width entries of a model without a table: the cache then answers 0 everywhere"""
    for which in (0, 1):
        p = nrc.GetParams(which)
        p[-3 * width:] = 0.0
        nrc.SetParams(which, p)


@pytest.mark.parametrize("variant", ["long-pipelined", "long-single-stream", "self-train"])
@pytest.mark.parametrize("name", ["A", "B", "C1", "D"])
def test_every_train_kernel_variant_at_ragged_grids(api, orc, torch_gpu, monkeypatch, name, variant):
    """long-pipelined: k_prep_train<1> on the 16x16 tiling plus <2> at 32 rays per wave on a stream of its own; long-single-stream: <0> at 32
    rays per wave; self-train: <0, true> with its tail records (a zeroed cache: the targets are the oracle's single-path targets) -- three
    frames each on grids with partial tiles and a ragged last block"""
    case, g = tc.CASES[name], tc.case_grid(tc.CASES[name])
    T = g["tw"] * g["th"]
    nrc_debug(monkeypatch, single_stream=variant == "long-single-stream")
    if variant == "self-train":
        spp, L = 1, 1
        nrc, ren = setup(api, case, **config_of(case, self_train=1))
        _, longer = tc.oracle_frames(orc, name, spp, L + 1)
    else:
        spp, L = 2, 4
        nrc, ren = setup(api, case, **config_of(case, long_paths=True))
    assert ren.TrainGrid() == g
    gens, frames = tc.oracle_frames(orc, name, spp, L)
    models = tc.model_frames(name)
    tails_checked = 0
    for f, fr in enumerate(tc.frame_randoms(case)):
        if variant == "self-train":
            zero_output_layer(nrc)
        ren.SetFrameRandom(fr)
        ren.Render(None, variant == "self-train")
        check_frame(ren, name, f, frames[f], models[f])
        if variant == "self-train":
            rec = ren.Buffer("tail_record").cpu().numpy()
            q = ren.Buffer("tail_query").cpu().numpy()
            assert rec.shape == (T * spp, 4) and q.shape == (T * spp, 5)
            assert np.isin(rec[:, 3], np.float32([0.0, 0.5 ** L])).all()
            assert (rec[:, 3] > 0).any() and (rec[:, 3] == 0).any()
            assert (q[rec[:, 3] == 0] == 0).all()                 # no tail: a zero query
            # where one more vertex changes the oracle's target, the path went on after L vertices: its record has a tail
            rows = (longer[f]["tgt"].view(np.uint32) != frames[f]["tgt"].view(np.uint32)).any(axis=1)
            assert rows.any() and (rec[rows, 3] > 0).all()
            tails_checked += int(rows.sum())
    assert variant != "self-train" or tails_checked > 0
    ren.Destroy()
    nrc.Destroy()


GUARD_CHILD = """
import sys
import numpy as np
import torch
sys.path[:0] = [%r, %r]
from nrc_hpm_renderer_amd import api
import train_grid_cases as tc
import test_gpu_train_grid as t
L = api.load_library()
assert L.nrc_debug_check_guards(None, 0) == 0, "guard mode is off"
for name in ("A", "C1", "F", "Z"):
    case = tc.CASES[name]
    for long_paths in (False, True):
        nrc, ren = t.setup(api, case, **t.config_of(case, long_paths=long_paths))
        for fr in tc.frame_randoms(case)[:2]:
            ren.SetFrameRandom(fr)
            ren.Render(None, True)
        head, tail, entries = t.ring_of(ren)
        assert np.isfinite(entries).all() and (head > 0) == (name != "Z")
        torch.cuda.synchronize()
        ren.Destroy()
        nrc.Destroy()
        # (the count is cumulative: live allocations' guard bands now, and what every free found -- the slack up to 256 bytes included)
        print(name, long_paths, "guards", L.nrc_debug_check_guards(None, 0))
"""


def test_odd_train_grids_stay_inside_their_buffers(torch_gpu):
    """a fresh process under NRC_DEBUG=guard_alloc: two trained frames each on a ragged grid, a ring smaller than T, a ring larger than T and
    no ring, with short and with long train paths -- after each renderer is gone nrc_debug_check_guards has found every canary intact"""
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", GUARD_CHILD % (os.path.dirname(tests), tests)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, NRC_DEBUG="guard_alloc"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [line for line in r.stdout.splitlines() if "guards" in line]
    assert len(lines) == 8 and all(line.endswith("guards 0") for line in lines), (r.stdout + r.stderr)[-3000:]
