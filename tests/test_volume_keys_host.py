"""Volume keyframes, the parts that need no GPU: a time's key pair and weight (scene.key_of_time against csrc/nrc_volume_keys.hpp, which
tests/cpp/volume_keys_main.cpp drives on the CPU under ASan + UBSan), the integer in-between voxel, the CLI's --animate rules, and the new
entry points in the header and both mirrors."""
import argparse
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nrc-hpm-renderer_amd", "csrc")
HEADER = "nrc_volume_keys.hpp"


# ---------------------------------------------------------------------------------------------------------------- time -> (i, W)
def test_key_of_time_cases(sc):
    n = 4
    last = np.float32(n - 1)
    assert sc.key_of_time(0, n) == (0, 0)
    assert sc.key_of_time(0.5, n) == (0, 128)
    assert sc.key_of_time(129 / 256, n) == (0, 129)
    assert sc.key_of_time(1.5, n) == (1, 128)
    assert sc.key_of_time(n - 1, n) == (n - 1, 0)                               # the last key: its successor is never read
    assert sc.key_of_time(np.nextafter(last, np.float32(0)), n) == (n - 2, 256)      # just below it: all of key n - 1, named through n - 2
    assert sc.key_of_time(0, 1) == (0, 0)                                       # a sequence of one key
    # W rounds to nearest: 1/512 below a step stays, the half step itself goes up
    assert sc.key_of_time(1 + 127 / 512, n) == (1, 64) and sc.key_of_time(1 + 255 / 512 - 2.0 ** -12, n) == (1, 127)
    for i in range(n - 1):
        for W in range(257):
            assert sc.key_of_time(i + W / 256, n) == ((i, W) if W < 256 else (i + 1, 0))
    for bad in (float("nan"), -1e-30, -1.0, n - 1 + 2.0 ** -20, float(n), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            sc.key_of_time(bad, n)
    for bad_n, t in ((0, 0.0), (1, 0.5), (1, 2.0 ** -20)):
        with pytest.raises(ValueError):
            sc.key_of_time(t, bad_n)
    # the time is an fp32 (what the C entry point takes): a double that rounds onto the last key is the last key
    assert sc.key_of_time(n - 1 + 1e-12, n) == (n - 1, 0)


# ---------------------------------------------------------------------------------------------------------------- the in-between voxel
def test_lerp_volume_ends_bounds_and_every_combination(sc):
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    assert np.array_equal(sc.lerp_volume(a, b, 0), a) and np.array_equal(sc.lerp_volume(a, b, 256), b)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    for W in range(257):      # all 256 x 256 x 257 combinations, against Python's own integers
        q = sc.lerp_volume(a, b, W)
        assert q.dtype == np.uint8 and q.shape == a.shape
        want = [(x * (256 - W) + y * W + 128) >> 8 for x in range(256) for y in range(256)]
        assert q.reshape(-1).tolist() == want, W
        assert (q >= lo).all() and (q <= hi).all(), W
    # single voxels: the corners and a seeded sample
    rng = np.random.default_rng(5)
    sample = [(0, 0, 0), (255, 255, 256), (255, 0, 128), (0, 255, 128), (255, 0, 1), (1, 0, 128), (1, 0, 129)] + \
             [tuple(int(v) for v in rng.integers(0, (256, 256, 257))) for _ in range(4000)]
    for x, y, W in sample:
        got = int(sc.lerp_volume(np.array([x], np.uint8), np.array([y], np.uint8), W)[0])
        assert got == (x * (256 - W) + y * W + 128) >> 8 and min(x, y) <= got <= max(x, y), (x, y, W)
    for W in (-1, 257):
        with pytest.raises(ValueError):
            sc.lerp_volume(a, b, W)
    with pytest.raises(ValueError):
        sc.lerp_volume(a, b.astype(np.float32), 3)


def test_a_voxel_of_one_fades_out_between_128_and_129(sc):
    one, zero = np.array([1], np.uint8), np.array([0], np.uint8)
    for W in range(257):
        assert int(sc.lerp_volume(one, zero, W)[0]) == (1 if W <= 128 else 0), W
        assert int(sc.lerp_volume(zero, one, W)[0]) == (1 if W >= 128 else 0), W


def test_volume_at(sc):
    rng = np.random.default_rng(9)
    keys = rng.integers(0, 256, (3, 5, 6, 7)).astype(np.uint8)
    assert np.array_equal(sc.volume_at(keys, 0), keys[0]) and np.array_equal(sc.volume_at(keys, 1), keys[1])
    assert np.array_equal(sc.volume_at(keys, 2), keys[2])
    assert np.array_equal(sc.volume_at(keys, 1.25), sc.lerp_volume(keys[1], keys[2], 64))
    assert np.array_equal(sc.volume_at(keys, np.nextafter(np.float32(2), np.float32(0))), keys[2])
    assert sc.volume_at(keys, 0.5).flags.c_contiguous and sc.volume_at(keys, 1).flags.c_contiguous
    assert np.array_equal(sc.volume_at(keys[:1], 0), keys[0])
    for bad in (2.5, -0.5, float("nan")):
        with pytest.raises(ValueError):
            sc.volume_at(keys, bad)
    with pytest.raises(ValueError):
        sc.volume_at(keys.astype(np.float32), 0.5)


# ---------------------------------------------------------------------------------------------------------------- the device-free header
def test_the_header_compiles_without_rocm_and_the_library_depends_on_it():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-include", HEADER, "-x", "c++", os.devnull],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-4000:]
    code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, HEADER)).read())
    code, n = re.subn(r"#if defined\(__HIPCC__\)\n#define NRC_KEYS_HD [^\n]*\n#else\n#define NRC_KEYS_HD inline\n#endif\n", "", code)
    assert n == 1
    assert not re.search(r"hip|nccl|__device__|__host__", code, re.I)
    assert "nrc_common.hpp" not in code
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^KEY_HDRS = " + re.escape(HEADER) + "$", makefile, re.M)
    assert re.search(r"^SRCS = [^\n]*\$\(KEY_HDRS\)", makefile, re.M)      # among the build id's sources
    for obj in ("nrc_api.o", "nrc_integrator.o"):
        rule = re.search(r"^\$\(OUT\)/" + re.escape(obj) + r":([^\n]*)$", makefile, re.M)
        assert rule and "$(KEY_HDRS)" in rule.group(1), obj


def test_key_of_time_of_the_library_equals_the_python_statement_under_the_sanitizers(sc):
    """tests/cpp/volume_keys_main.cpp: its own main, built from the device-free header alone with ASan + UBSan (no recovery) and run
    directly; every (i, W) it prints -- the cases above for 0 .. 1000 keys and a sweep of t across every key -- is scene.key_of_time's"""
    build = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "volume_keys_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "volume_keys_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out and "FAILED" not in out, out[-4000:]
    m = re.search(r"^volume_keys: (\d+) checks, 0 failed$", out, re.M)
    assert m and int(m.group(1)) > 256 * 256 * 257, out[-400:]
    lines = re.findall(r"^key ([0-9a-f]{8}) (\d+) (-?\d+) (-?\d+)$", out, re.M)
    assert len(lines) > 20000
    accepted = rejected = 0
    weights = set()
    for bits, n, i, W in lines:
        t = np.array([int(bits, 16)], np.uint32).view(np.float32)[0]
        try:
            want = sc.key_of_time(t, int(n))
            accepted += 1
            weights.add(want[1])
        except ValueError:
            want = (-1, -1)
            rejected += 1
        assert (int(i), int(W)) == want, (bits, float(t), n, i, W, want)
    assert accepted > 10000 and rejected > 1000 and weights == set(range(257))


# ---------------------------------------------------------------------------------------------------------------- CLI
def _args(**kw):
    d = dict(orbit=None, frames=4, benchmark=False, vdb=None, gpus=1, export=None, animate=False, bricks=False, time_scale=1.0)
    d.update(kw)
    return argparse.Namespace(**d)


def test_cli_animate_argument_rules():
    from nrc_hpm_renderer_amd import cli
    seq = ["a.vdb", "b.vdb", "c.vdb"]
    assert cli.check_animate_args(_args()) is False
    assert cli.check_animate_args(argparse.Namespace(orbit=4, vdb=seq)) is False      # (a namespace without the flag)
    assert cli.check_animate_args(_args(orbit=4, vdb=seq, animate=True)) is True
    assert cli.check_orbit_args(_args(orbit=4, vdb=seq, animate=True)) == 4
    with pytest.raises(SystemExit, match="--orbit takes one volume, not a --vdb sequence"):      # without the flag: as before
        cli.check_orbit_args(_args(orbit=4, vdb=seq))
    for bad in (dict(animate=True), dict(animate=True, orbit=4), dict(animate=True, orbit=4, vdb=["a.vdb"]), dict(animate=True, vdb=seq),
                dict(animate=True, orbit=4, vdb=seq, bricks=True), dict(animate=True, orbit=4, vdb=seq, time_scale=-1.0),
                dict(animate=True, orbit=4, vdb=seq, time_scale=float("nan"))):
        with pytest.raises(SystemExit, match="SkyRenderer ERROR"):
            cli.check_animate_args(_args(**bad))
    # the parser: a bad combination ends the run before anything touches the GPU (or a file)
    for argv in (["--animate"], ["--animate", "--orbit", "4"], ["--animate", "--vdb", "a.vdb", "b.vdb"],
                 ["--animate", "--orbit", "4", "--vdb", "a.vdb", "b.vdb", "--bricks"], ["--orbit", "4", "--vdb", "a.vdb", "b.vdb"]):
        with pytest.raises(SystemExit, match="SkyRenderer ERROR"):
            cli.main(argv)


def test_cli_animate_times(sc):
    from nrc_hpm_renderer_amd import cli
    t = cli.animate_times(5, 3)
    assert t.dtype == np.float32 and np.array_equal(t, np.array([0, 0.5, 1, 1.5, 2], np.float32))
    assert np.array_equal(cli.animate_times(1, 3), np.array([0], np.float32))              # max(N - 1, 1)
    assert np.array_equal(cli.animate_times(3, 1), np.zeros(3, np.float32))                # one key: it stands still
    assert np.array_equal(cli.animate_times(5, 3, 0.5), np.array([0, 0.25, 0.5, 0.75, 1], np.float32))      # slow motion
    assert np.array_equal(cli.animate_times(5, 3, 2.0), np.array([0, 1, 2, 2, 2], np.float32))              # clamped at the last key
    for n_views, n_keys, scale in ((64, 8, 1.0), (7, 24, 3.7), (10, 2, 0.01)):
        for v in cli.animate_times(n_views, n_keys, scale):
            sc.key_of_time(v, n_keys)      # (every time is one the library accepts)
    assert math.isclose(float(cli.animate_times(64, 8)[-1]), 7.0)


# ---------------------------------------------------------------------------------------------------------------- the surface
NEW_SYMBOLS = ["nrc_renderer_set_volume_keys", "nrc_mc_renderer_set_volume_keys", "nrc_renderer_volume_key_count", "nrc_mc_renderer_volume_key_count",
               "nrc_renderer_set_volume_time", "nrc_mc_renderer_set_volume_time", "nrc_renderer_render_path_timed", "nrc_mc_renderer_render_path_timed"]


def test_new_symbols_are_in_the_header_and_both_mirrors(api):
    header = open(os.path.join(ROOT, "include", "nrc_hpm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    hpp = open(os.path.join(ROOT, "include", "nrc_hpm.hpp")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), s
        assert s + "(" in hpp, s
        assert s in api.ABI_SYMBOLS, s
        assert hasattr(api.load_library(), s), s
    assert re.search(r"int nrc_renderer_set_volume_keys\(nrc_renderer_t\* r, const void\* volumes, uint32_t n_keys, uint32_t nx, uint32_t ny, uint32_t nz, "
                     r"int format,\s*int on_device\);", code)
    assert re.search(r"int nrc_renderer_set_volume_time\(nrc_renderer_t\* r, float t\);", code)
    assert re.search(r"int nrc_renderer_render_path_timed\(nrc_renderer_t\* r, uint32_t n_cameras, const nrc_camera\* cameras, const float\* times,\s*"
                     r"uint32_t frames_per_camera, const float\* frame_randoms, int train, float\* d_frames\);", code)
    assert re.search(r"int nrc_mc_renderer_render_path_timed\(nrc_mc_renderer_t\* r, uint32_t n_cameras, const nrc_camera\* cameras, const float\* times,\s*"
                     r"uint32_t frames_per_camera, const float\* frame_randoms, float\* d_frames\);", code)
    # the specification is in the header's text: the weight's rounding and the integer in-between
    assert "(uint32)(w * 256.0f + 0.5f)" in header and "q = (a * (256 - W) + b * W + 128) >> 8" in header
    for cls in ("NrcHpmRenderer", "McHpmRenderer"):
        body = hpp.split("class %s {" % cls)[1].split("\n};")[0]
        for name in ("void SetVolumeKeys(", "VolumeKeyCount()", "void SetVolumeTime(float t)", "const float* times"):
            assert name in body, (cls, name)
        py = getattr(api, cls)
        for name in ("SetVolumeKeys", "VolumeKeyCount", "SetVolumeTime", "RenderPath"):
            assert callable(getattr(py, name)), (cls, name)

        class Probe(py):      # RenderPath's times keyword reaches the path with the other arguments in place
            def __init__(self):
                pass

            def _path(self, *a):
                return a
        assert Probe().RenderPath(["cam"], 2, times=[0.5]) == (["cam"], 2, None, False, None, [0.5])
        assert Probe().RenderPath(["cam"], 2, None, False, False, times=[1.0]) == (["cam"], 2, None, False, False, [1.0])
