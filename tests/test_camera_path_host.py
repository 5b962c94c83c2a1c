"""Camera paths, the parts that need no GPU: the turntable helper, the CLI's --orbit / --export pattern, and the new entry points in the
header and both mirrors."""
import argparse
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_orbit_cameras_match_look_at_and_perspective(sc):
    n, radius, height, aspect = 7, 50.0, 12.0, 1.6
    fovy, near, far = math.radians(60.0), 0.1, 100.0
    cams = sc.orbit_cameras(n, radius, height, aspect)
    assert len(cams) == n
    proj = sc.perspective(fovy, aspect, near, far)
    for k, cam in enumerate(cams):
        a = 2.0 * math.pi * k / n
        eye = np.array([radius * math.cos(a), height, radius * math.sin(a)])
        assert np.allclose(cam["pos"], eye, rtol=0, atol=1e-5) and cam["pos"].dtype == np.float32
        assert abs(np.linalg.norm(cam["pos"][[0, 2]]) - radius) < 1e-4 and abs(cam["pos"][1] - height) < 1e-6
        want = np.linalg.inv(proj @ sc.look_at(eye, np.zeros(3), (0.0, 1.0, 0.0))).T.astype(np.float32).reshape(16)
        assert cam["inv_proj_view"].shape == (16,) and cam["inv_proj_view"].dtype == np.float32
        assert np.allclose(cam["inv_proj_view"], want, rtol=1e-5, atol=1e-6), k
        # the centre of the image looks at the volume's centre: ndc (0, 0) unprojects onto the line eye -> origin
        inv = cam["inv_proj_view"].reshape(4, 4).T.astype(np.float64)
        p = inv @ np.array([0.0, 0.0, 0.0, 1.0])
        d = p[:3] / p[3] - eye
        assert np.allclose(d / np.linalg.norm(d), -eye / np.linalg.norm(eye), atol=1e-5), k


def test_orbit_view_zero_is_the_default_camera_and_arguments_are_checked(sc):
    d, o = sc.make_camera(aspect=1.25), sc.orbit_cameras(4, aspect=1.25)[0]
    assert np.array_equal(d["pos"], o["pos"]) and np.allclose(d["inv_proj_view"], o["inv_proj_view"], rtol=1e-6, atol=1e-7)
    moved = sc.orbit_cameras(2, radius=10.0, height=3.0, center=(1.0, 2.0, 3.0), start_angle=math.pi / 2)
    assert np.allclose(moved[0]["pos"], (1.0, 5.0, 13.0), atol=1e-5) and np.allclose(moved[1]["pos"], (1.0, 5.0, -7.0), atol=1e-5)
    wide = sc.orbit_cameras(1, fovy=math.radians(90.0))[0]
    assert np.allclose(wide["inv_proj_view"], sc.make_camera(fovy=math.radians(90.0))["inv_proj_view"], rtol=1e-6, atol=1e-7)
    with pytest.raises(ValueError):
        sc.orbit_cameras(0)
    with pytest.raises(ValueError):
        sc.orbit_cameras(3, radius=0.0, height=0.0)


def test_cli_export_pattern():
    from nrc_hpm_renderer_amd import cli
    assert cli.export_paths(None, 3) == []
    assert cli.export_paths("out.exr", 3) == ["out.exr"]
    assert cli.export_paths("out_%04d.exr", 3) == ["out_0000.exr", "out_0001.exr", "out_0002.exr"]
    assert cli.export_paths("dir/v%d.exr", 2) == ["dir/v0.exr", "dir/v1.exr"]
    for bad in ("out_%s.exr", "out_%q.exr", "out_%d_%d.exr", "out_%.exr", "out%%.exr", "out_%5.2f.exr", "out_%-4d.exr"):
        with pytest.raises(SystemExit, match="SkyRenderer ERROR"):
            cli.export_paths(bad, 2)


def _args(**kw):
    d = dict(orbit=None, frames=4, benchmark=False, vdb=None, gpus=1, export=None)
    d.update(kw)
    return argparse.Namespace(**d)


def test_cli_orbit_argument():
    from nrc_hpm_renderer_amd import cli
    assert cli.check_orbit_args(_args()) == 0
    assert cli.check_orbit_args(_args(export="literal_%d.exr")) == 0      # without --orbit the name is taken as it is
    assert cli.check_orbit_args(_args(orbit=8, export="o_%03d.exr")) == 8
    assert cli.check_orbit_args(_args(orbit=1, export="o.exr", gpus=2)) == 1
    for bad in (dict(orbit=0), dict(orbit=-3), dict(orbit=4, frames=0), dict(orbit=4, benchmark=True), dict(orbit=4, vdb=["a.vdb", "b.vdb"]),
                dict(orbit=4, gpus=2, export="o_%d.exr"), dict(orbit=4, export="o_%s.exr")):
        with pytest.raises(SystemExit, match="SkyRenderer ERROR"):
            cli.check_orbit_args(_args(**bad))
    # the parser itself: --orbit takes an integer, and a bad combination ends the run before anything touches the GPU
    with pytest.raises(SystemExit):
        cli.main(["--orbit", "many"])
    with pytest.raises(SystemExit, match="SkyRenderer ERROR"):
        cli.main(["--orbit", "4", "--benchmark"])
    with pytest.raises(SystemExit, match="SkyRenderer ERROR"):
        cli.main(["--orbit", "0"])


NEW_SYMBOLS = ["nrc_renderer_render_path", "nrc_mc_renderer_render_path", "nrc_renderer_tile_mask", "nrc_mc_renderer_tile_mask"]


def test_new_symbols_are_in_the_header_and_both_mirrors(api):
    header = open(os.path.join(ROOT, "include", "nrc_hpm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    hpp = open(os.path.join(ROOT, "include", "nrc_hpm.hpp")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), s
        assert s + "(" in hpp, s
        assert s in api.ABI_SYMBOLS, s
        assert hasattr(api.load_library(), s), s
    assert re.search(r"int nrc_renderer_render_path\(nrc_renderer_t\* r, uint32_t n_cameras, const nrc_camera\* cameras, uint32_t frames_per_camera,\s*"
                     r"const float\* frame_randoms, int train, float\* d_frames\);", code)
    assert re.search(r"int nrc_mc_renderer_render_path\(nrc_mc_renderer_t\* r, uint32_t n_cameras, const nrc_camera\* cameras, uint32_t frames_per_camera,\s*"
                     r"const float\* frame_randoms, float\* d_frames\);", code)
    for cls in ("NrcHpmRenderer", "McHpmRenderer"):
        body = hpp.split("class %s {" % cls)[1].split("\n};")[0]
        assert "void RenderPath(" in body and "TileMask()" in body, cls
        py = getattr(api, cls)
        assert callable(py.RenderPath) and callable(py.TileMask), cls
    import inspect
    assert list(inspect.signature(api.NrcHpmRenderer.RenderPath).parameters) == ["self", "cameras", "framesPerCamera", "frameRandoms", "train", "out"]
