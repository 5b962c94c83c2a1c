"""The view AOV ({alpha, tau, z_front, z_half} per pixel: include/nrc_hpm.h, csrc/nrc_view_aov.hpp), the parts that need no GPU: the fp64
reference (tests/view_aov_reference.py) against closed forms and against the CPU oracle's Monte-Carlo alpha, the fp32 host restatement
against the reference, nrc_expm1_negf against fp64, and the new surface.  tests/cpp/view_aov_main.cpp -- its own main, the device-free
headers alone, ASan + UBSan without recovery -- is built once and run directly; nothing is loaded into Python under a sanitizer."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import view_aov_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nrc-hpm-renderer_amd", "csrc")
COMPONENTS = (("alpha", 0), ("tau", 1), ("z_front", 2), ("z_half", 3))
CASES = ("blocks_v3", "blocks_v1", "cloud_v3", "blocks_inside")

_REF = {}


def reference(sc, name):
    """the fp64 reference of a case, computed once per session"""
    if name not in _REF:
        scene, cam = R.cases(sc)[name]
        _REF[name] = R.reference_view(scene, cam)
    return _REF[name]


@pytest.fixture(scope="module")
def program():
    build = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "view_aov_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "view_aov_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def run(*args):
        r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600, env=env)
        out = r.stdout + r.stderr
        assert r.returncode == 0, out[-4000:]
        assert "AddressSanitizer" not in out and "runtime error" not in out and "FAILED" not in out, out[-4000:]
        return out
    return run


def program_aov(program, tmp_path, scene, cam, w=R.W, h=R.H):
    """the program's plain voxel walk [h][w][4]; the program itself fails when its walk with occupancy jumps differs in any bit"""
    nx, ny, nz = scene["dims"]
    head = struct.pack("<8I", nx, ny, nz, w, h, 0, 1, 0)
    floats = np.concatenate([np.asarray(scene["size"], np.float32), [np.float32(scene["density_factor"])],
                             [np.float32(1.0) / np.float32(w), np.float32(1.0) / np.float32(h)],
                             np.asarray(cam["inv_proj_view"], np.float32).reshape(16), np.asarray(cam["pos"], np.float32)]).astype("<f4")
    src, dst = str(tmp_path / "scene.bin"), str(tmp_path / "aov.bin")
    with open(src, "wb") as f:
        f.write(head + floats.tobytes() + np.ascontiguousarray(scene["density"], np.uint8).tobytes())
    out = program("aov", src, dst)
    assert " 0 differ between the plain walk and the walk with jumps" in out, out
    return np.fromfile(dst, "<f4").reshape(h, w, 4)


# ---------------------------------------------------------------------------------------------------------------- 1. closed forms
def _chords(size, pos, dirs):
    """slab entry max(0, .) and exit of rays from pos through the box of `size` centred on the origin, fp64"""
    with np.errstate(divide="ignore"):
        ta, tb = (-0.5 * size - pos) / dirs, (0.5 * size - pos) / dirs
    t0 = np.maximum(np.minimum(ta, tb).max(axis=-1), 0.0)
    t1 = np.maximum(ta, tb).min(axis=-1)
    return t0, t1


def test_reference_equals_the_closed_form_of_a_full_volume(sc):
    """every voxel 255: tau = sigma * chord, z_front = t0, z_half = t0 + ln 2 / sigma"""
    scene = sc.make_scene(np.full((9, 5, 7), 255, np.uint8), scene_id=4)
    cam = R.orbit_view(sc, 3)
    size, sigma = scene["size"].astype(np.float64), float(np.float32(scene["density_factor"]))
    dirs, pos = R.ray_directions(cam, 24, 16)
    t0, t1 = _chords(size, pos, dirs)
    hit = 0
    for y in range(16):
        for x in range(24):
            tau, zf, zh, _, _, _ = R.reference_ray(scene["density"], size, sigma, pos, dirs[y, x])
            if not t0[y, x] < t1[y, x]:
                assert (tau, zf, zh) == (0.0, math.inf, math.inf)
                continue
            hit += 1
            want = sigma * (t1[y, x] - t0[y, x])
            assert abs(tau - want) <= 1e-12 * (1.0 + want)
            assert abs(zf - t0[y, x]) <= 1e-12 * t0[y, x]
            if want >= R.LN2:
                assert abs(zh - (t0[y, x] + R.LN2 / sigma)) <= 1e-9
            else:
                assert zh == math.inf
    assert hit > 40


def test_reference_equals_the_closed_form_of_two_slabs(sc):
    """x < 0: byte 60, x >= 0: byte 200 -- two homogeneous slabs, the chord split at the plane x = 0"""
    vol = np.zeros((6, 4, 10), np.uint8)
    vol[:, :, :5], vol[:, :, 5:] = 60, 200
    scene = sc.make_scene(vol, scene_id=4)
    size, rho = scene["size"].astype(np.float64), float(np.float32(scene["density_factor"]))
    cam = R.orbit_view(sc, 1)
    dirs, pos = R.ray_directions(cam, 24, 16)
    t0, t1 = _chords(size, pos, dirs)
    s_neg, s_pos = rho * 60 / 255.0, rho * 200 / 255.0
    hit = 0
    for y in range(16):
        for x in range(24):
            d = dirs[y, x]
            if not t0[y, x] < t1[y, x]:
                continue
            hit += 1
            tm = min(max(-pos[0] / d[0], t0[y, x]), t1[y, x])      # where the ray meets x = 0, clamped into the chord
            first, second = (s_pos, s_neg) if d[0] < 0 else (s_neg, s_pos)      # (a chord on one side only: tm is one of its ends)
            tau1 = first * (tm - t0[y, x])
            want = tau1 + second * (t1[y, x] - tm)
            tau, zf, zh, _, _, _ = R.reference_ray(vol, size, rho, pos, d)
            assert abs(tau - want) <= 1e-11 * (1.0 + want)
            assert abs(zf - t0[y, x]) <= 1e-12 * t0[y, x]
            if want >= R.LN2:
                z = t0[y, x] + R.LN2 / first if tau1 >= R.LN2 else tm + (R.LN2 - tau1) / second
                assert abs(zh - z) <= 1e-9
    assert hit > 40


# ---------------------------------------------------------------------------------------------------------------- 2. the oracle
def test_oracle_monte_carlo_alpha_estimates_the_reference_alpha(sc, orc):
    """Oracle.mc_render's alpha (the scatter flag of a path of length 1) averaged over 64 frames is an unbiased estimate of 1 - exp(-tau):
    chi^2 over the pixels with alpha in (0.05, 0.95) stays below n + 6 sqrt(2 n) (measured 143.1 over n = 140, bound 240), and a pixel
    whose alpha is 0 never scatters"""
    scene, cam = R.cases(sc)["blocks_v3"]
    ref = reference(sc, "blocks_v3")
    alpha = -np.expm1(-ref["tau"][..., 0])
    acc = np.zeros((R.H, R.W))
    for fr in sc.frame_randoms(64, seed=11):
        img, _, _ = orc.mc_render(scene, cam, R.W, R.H, 1, fr, blend=1.0, threads=8)
        acc += img[..., 3]
    a_mc = acc / 64.0
    chi2, n, bound = R.chi2_against_alpha(a_mc, alpha, 64)
    print("chi2 %.1f over n = %d (bound %.1f); mean alpha %.4f, mean a_mc %.4f" % (chi2, n, bound, alpha.mean(), a_mc.mean()))
    assert n >= 100
    assert chi2 <= bound
    assert (a_mc[alpha == 0.0] == 0.0).all()


# ---------------------------------------------------------------------------------------------------------------- 3. the host restatement
@pytest.mark.parametrize("name", CASES)
def test_at_most_five_percent_of_the_hit_pixels_are_unstable(sc, name):
    un, hit = R.unstable_share(reference(sc, name))
    print("%s: %d unstable of %d hit pixels" % (name, un, hit))
    assert hit > 250 and un <= R.UNSTABLE_CAP * hit


def _compare(got, ref, sigma_max):
    """per component: the largest error-to-bound ratio over the stable pixels (finiteness must agree there)"""
    tol = R.tolerances(ref, sigma_max)
    st = ref["stable"]
    ratios = {}
    for k, i in COMPONENTS:
        want = -np.expm1(-ref["tau"][..., 0]) if k == "alpha" else ref[k][..., 0]
        g = got[..., i].astype(np.float64)
        assert (np.isfinite(g) == np.isfinite(want))[st].all(), k
        m = st & np.isfinite(want)
        err, bound = np.abs(g[m] - want[m]), tol[k][m]
        ratios[k] = float(np.where(err > 0.0, err / np.maximum(bound, 1e-300), 0.0).max()) if m.any() else 0.0
    return ratios


@pytest.mark.parametrize("name", CASES)
def test_host_restatement_against_the_fp64_reference(sc, api, program, tmp_path, name):
    """The fp32 walk (the sanitized program's) against the fp64 reference along the fp32 inv_proj_view evaluated in fp64, on stable pixels:
        |d tau|     <= S_tau + 8 N sigma_max ulp32(t1) + N ulp32(tau)
        |d z_front| <= S_z + 8 ulp32(z)
        |d z_half|  <= S_z + tol_tau / sigma_cross + 8 ulp32(z)
        |d alpha|   <= tol_tau + 4 ulp32(1)
    (S: the reference's spread over the pixel's five rays, N: plane crossings), under the precondition that the fp32 ray direction lies
    within 5e-7 rad of the fp64 one, so that the 2e-6 perturbation brackets it.  Measured: 1.2e-7 rad on every view (the rounding of
    u, v and of 2u - 1; view_aov_camera_ray cancels the large terms before it rounds -- the frames' camera_ray, which does not, is
    2.2e-5 rad off on the orbit views and misses these bounds by a factor of up to 9.5).  Largest error-to-bound ratios: blocks V3
    tau 0.04, z_front 0.12, z_half 0.03, alpha 0.03;  blocks V1 0.01, 0.16, 0.02, 0.01;  cloud V3 0.01, 0.11, 0.003, 0.003;  inside
    0.03, 0.96, 0.03, 0.02 (z_front there is about 5 and 8 ulp32 of it are 4e-6: the plane parameters fma(i, k, c) with |c| near 60 are
    rounded to half an ulp32 of c)."""
    scene, cam = R.cases(sc)[name]
    got = program_aov(program, tmp_path, scene, cam)
    ref = reference(sc, name)
    d32 = R.ray_directions_f32(cam, R.W, R.H).astype(np.float64)
    angle = np.linalg.norm(np.cross(d32, ref["dirs"]), axis=-1) / np.linalg.norm(d32, axis=-1)
    ratios = _compare(got, ref, float(np.float32(scene["density_factor"])))
    print("%s: fp32 ray within %.2e rad of the fp64 one; largest error-to-bound ratios %s" % (name, angle.max(), ratios))
    assert angle.max() <= 5e-7
    assert max(ratios.values()) <= 1.0


def check_ranges(a):
    """the contract's range properties of an AOV image"""
    alpha, tau, zf, zh = (a[..., i] for i in range(4))
    assert not np.isnan(a).any()
    assert (alpha >= 0.0).all() and (alpha <= 1.0).all() and (tau >= 0.0).all() and np.isfinite(tau).all()
    assert ((tau > 0.0) == np.isfinite(zf)).all() and ((tau > 0.0) == (alpha > 0.0)).all()
    assert (np.isfinite(zh) == (tau >= np.float32(R.LN2))).all()
    assert (zf[np.isfinite(zf)] >= 0.0).all()
    both = np.isfinite(zf) & np.isfinite(zh)
    assert (zf[both] <= zh[both]).all()
    miss = tau == 0.0
    assert (alpha[miss] == 0.0).all() and np.isposinf(zf[miss]).all() and np.isposinf(zh[miss]).all()


@pytest.mark.parametrize("name", CASES + ("blocks_default", "cloud_default"))
def test_library_and_program_agree_bitwise_and_keep_the_ranges(sc, api, program, tmp_path, name):
    """nrc_test_view_aov_host (the library's host compiler) and the sanitized program (g++) run the same header: the same bits; the
    program has also walked every pixel with the occupancy jumps and found the same bits.  The default view -- its centre row and column
    run inside voxel faces -- is looked at for this and for the range properties only."""
    if name.endswith("_default"):
        vol = R.blocks_volume() if name.startswith("blocks") else R.cloud_volume()
        scene, cam = sc.make_scene(vol, scene_id=4), R.default_view(sc)
    else:
        scene, cam = R.cases(sc)[name]
    got = program_aov(program, tmp_path, scene, cam)
    lib = api.test_view_aov_host(scene, cam, R.W, R.H)
    assert R.same_bits(got, lib)
    check_ranges(got)
    assert (got[..., 1] > 0.0).sum() > 100


def test_ragged_and_sharded_frames_on_the_host(sc, api):
    """44 x 36 (no multiple of 8) keeps the ranges; three ranks' 8-column strips of a 72 x 32 frame are the whole frame's columns"""
    scene, _ = R.cases(sc)["blocks_v3"]
    check_ranges(api.test_view_aov_host(scene, R.orbit_view(sc, 3, aspect=44 / 36), 44, 36))
    cam = R.orbit_view(sc, 3, aspect=72 / 32)
    whole = api.test_view_aov_host(scene, cam, 72, 32)
    for rank in range(3):
        part = api.test_view_aov_host(scene, cam, 24, 32, tile=(rank, 3, 72, 32, 8))
        cols = [((rank + (lx >> 3) * 3) << 3) + (lx & 7) for lx in range(24)]
        assert R.same_bits(part, whole[:, cols])


def test_degenerate_cameras_give_no_nan(sc, api):
    """axis-parallel rays (zero direction components), a camera on a face plane, far outside, and looking away"""
    scene, _ = R.cases(sc)["blocks_v3"]
    half = scene["size"].astype(np.float64) / 2
    for pos, view in (((200.0, 0.0, 0.0), (-1.0, 0.0, 0.0)), ((0.0, 0.0, -90.0), (0.0, 0.0, 1.0)), ((half[0], 0.0, 0.0), (-1.0, 0.0, 0.0)),
                      ((0.0, half[1], 0.0), (0.0, -1.0, 0.0)), ((1e6, 3e5, -2e5), (-1.0, -0.3, 0.2)), ((64.0, 0.0, 0.0), (1.0, 0.0, 0.0))):
        up = (0.0, 0.0, 1.0) if view[1] != 0.0 else (0.0, 1.0, 0.0)
        check_ranges(api.test_view_aov_host(scene, sc.make_camera(pos=pos, view_dir=view, up=up, aspect=1.5), 16, 16))


# ---------------------------------------------------------------------------------------------------------------- 4. nrc_expm1_negf
def test_expm1_sweep_against_fp64(program, tmp_path):
    """nrc_expm1_negf(x) = 1 - exp(-x): 65 * 2^16 (> 2^22) arguments across [2^-60, 32) and 129 neighbours of every branch point (0,
    (n + 1/2) ln 2, NRC_EXPM1_ONE), within 4 ulp of the fp64 value's fp32 neighbourhood (measured: 0.88 ulp); 0 for x <= 0 and NaN, 1 at +inf"""
    dst = str(tmp_path / "expm1.bin")
    program("expm1", dst)
    a = np.fromfile(dst, "<f4").reshape(-1, 2)
    assert a.shape[0] >= 1 << 22
    x, y = a[:, 0].astype(np.float64), a[:, 1].astype(np.float64)
    pos = np.isfinite(x) & (x > 0.0)
    want = -np.expm1(-x[pos])
    err = np.abs(y[pos] - want) / R.ulp32(want)
    print("largest error %.3f ulp at x = %r" % (err.max(), x[pos][err.argmax()]))
    assert err.max() <= 4.0
    assert (y[pos] >= 0.0).all() and (y[pos] <= 1.0).all()
    assert (np.diff(y[pos][:65 << 16]) >= 0.0).all()      # (the sweep is in ascending order: monotone)
    assert (y[~pos & ~np.isposinf(x)] == 0.0).all() and (y[np.isposinf(x)] == 1.0).all()


# ---------------------------------------------------------------------------------------------------------------- 5. the surface
NEW_SYMBOLS = ("nrc_renderer_view_aov", "nrc_mc_renderer_view_aov", "nrc_renderer_set_path_aov_target", "nrc_mc_renderer_set_path_aov_target",
               "nrc_renderer_export_exr_aov", "nrc_mc_renderer_export_exr_aov", "nrc_test_view_aov_host")


def test_the_new_symbols_exist_in_the_library_the_header_and_the_mirrors(api):
    L = api.load_library()
    header = open(os.path.join(ROOT, "include", "nrc_hpm.h")).read()
    hpp = open(os.path.join(ROOT, "include", "nrc_hpm.hpp")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in api.ABI_SYMBOLS and s + "(" in header, s
    for cls in (api.NrcHpmRenderer, api.McHpmRenderer):
        assert callable(cls.ViewAov) and callable(cls.ExportImageWithAovToFile) and callable(cls.SetPathAovTarget)
    assert callable(api.test_view_aov_host)
    for name in ("GetViewAov", "SetPathAovTarget", "ExportOutputImageWithAovToFile"):
        assert hpp.count(name) >= 2, name


def test_the_header_is_device_free():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-include", "nrc_view_aov.hpp", "-x", "c++", os.devnull],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-4000:]
    code = open(os.path.join(CSRC, "nrc_view_aov.hpp")).read()
    assert "hip_runtime" not in code and "__global__" not in code and "threadIdx" not in code
    assert "nrc_view_aov.hpp" in open(os.path.join(CSRC, "Makefile")).read()


def test_exr_channels_round_trip(tmp_path):
    from nrc_hpm_renderer_amd import io_exr
    rng = np.random.default_rng(3)
    planes = {n: rng.random((19, 23), dtype=np.float32) for n in ("A", "B", "G", "R", "Z", "Zhalf", "tau")}
    planes["Z"][3, 4] = np.inf
    for comp in ("none", "zip"):
        path = str(tmp_path / ("c_%s.exr" % comp))
        io_exr.write_exr_channels(path, planes, compression=comp)
        back = io_exr.read_exr_channels(path)
        assert sorted(back) == sorted(planes)
        for n in planes:
            assert R.same_bits(back[n], planes[n]), n
        rgba = io_exr.read_exr(path)
        for i, n in enumerate("RGBA"):
            assert R.same_bits(rgba[..., i], planes[n])


def test_cli_aov_argument_rules():
    import argparse
    from nrc_hpm_renderer_amd import cli
    cli.check_aov_args(argparse.Namespace(export=None, gpus=1))                  # (a namespace without the flag)
    cli.check_aov_args(argparse.Namespace(aov=False, export=None, gpus=4))
    cli.check_aov_args(argparse.Namespace(aov=True, export="out_%04d.exr", gpus=1))
    for bad in (dict(aov=True, export=None, gpus=1), dict(aov=True, export="a.exr", gpus=2)):
        with pytest.raises(SystemExit):
            cli.check_aov_args(argparse.Namespace(**bad))
    rgba, aov = np.arange(24, dtype=np.float32).reshape(2, 3, 4), -np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    planes = cli.aov_planes(rgba, aov)
    assert sorted(planes) == ["A", "B", "G", "R", "Z", "Zhalf", "tau"]
    assert planes["A"][1, 2] == aov[1, 2, 0] and planes["tau"][1, 2] == aov[1, 2, 1] and planes["Z"][0, 1] == aov[0, 1, 2] \
        and planes["Zhalf"][0, 0] == aov[0, 0, 3] and planes["B"][1, 0] == rgba[1, 0, 2]
