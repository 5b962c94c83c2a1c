"""The ray AOV ({alpha, tau, z_front, z_half} over caller-supplied ray segments: include/nrc_hpm.h "Ray AOV", csrc/nrc_view_aov.hpp
view_aov_walk_range), the parts that need no GPU: the bit contract of the range walk, its degenerate inputs, the split check, the fp32
host restatement against an fp64 reference of the range (tests/ray_aov_reference.py), and the new surface.
tests/cpp/ray_aov_main.cpp -- its own main, the device-free headers alone, ASan + UBSan without recovery -- is built once and run
directly; nothing is loaded into Python under a sanitizer."""
import argparse
import os
import struct
import subprocess

import numpy as np
import pytest

import ray_aov_reference as Q
import view_aov_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nrc-hpm-renderer_amd", "csrc")
COMPONENTS = (("alpha", 0), ("tau", 1), ("z_front", 2), ("z_half", 3))
VIEWS = ("blocks_v3", "blocks_v1", "cloud_v3", "blocks_inside")
LIGHTS = (("blocks", None), ("cloud", None), ("blocks", Q.OTHER_LIGHT), ("cloud", Q.OTHER_LIGHT))


@pytest.fixture(scope="module")
def program():
    build = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "ray_aov_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "ray_aov_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def run(*args):
        r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600, env=env)
        out = r.stdout + r.stderr
        assert r.returncode == 0, out[-4000:]
        assert "AddressSanitizer" not in out and "runtime error" not in out and "FAILED" not in out, out[-4000:]
        return out
    return run


def program_rays(program, tmp_path, scene, rays):
    """the program's plain range walk [...][4]; the program itself fails when its walk with jumps, or view_aov_walk on a whole ray, differs"""
    nx, ny, nz = scene["dims"]
    recs = np.ascontiguousarray(rays, np.float32)
    n = recs.size // 8
    head = struct.pack("<4I", nx, ny, nz, n)
    floats = np.concatenate([np.asarray(scene["size"], np.float32), [np.float32(scene["density_factor"])]]).astype("<f4")
    src, rs, dst = str(tmp_path / "scene.bin"), str(tmp_path / "rays.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(head + floats.tobytes() + np.ascontiguousarray(scene["density"], np.uint8).tobytes())
    recs.astype("<f4").tofile(rs)
    out = program("rays", src, rs, dst)
    assert " 0 differ between the plain walk and the walk with jumps" in out and " 0 differ from view_aov_walk" in out, out
    return np.fromfile(dst, "<f4").reshape(recs.shape[:-1] + (4,))


def ray_sets(api, sc):
    """{name: (scene, records)}: every set of the issue, for the bitwise checks"""
    sets = {}
    for name in VIEWS:
        scene, _, _, rays = Q.holdout_rays(api, sc, name)
        sets["holdout_" + name] = (scene, rays)
    for volume, light in LIGHTS:
        scene, _, rays = Q.light_rays(api, sc, volume, light)
        sets["light_%s_%s" % (volume, "scene" if light is None else "other")] = (scene, rays)
    for volume in ("blocks", "cloud"):
        scene = Q.volume_scene(sc, volume)
        sets["random_" + volume] = (scene, Q.random_segments(scene))
    return sets


SET_NAMES = tuple("holdout_" + v for v in VIEWS) + tuple("light_%s_%s" % (v, "scene" if l is None else "other") for v, l in LIGHTS) + \
    ("random_blocks", "random_cloud")
ACCURACY_SETS = SET_NAMES[:-1]      # (the cloud's random list is over the unstable cap: bitwise checks only)
_REF = {}


def reference(api, sc, name):
    """the fp64 reference of a ray set, computed once per session"""
    if name not in _REF:
        scene, rays = ray_sets(api, sc)[name]
        _REF[name] = Q.reference_rays(scene, rays)
    return _REF[name]


def check_ranges(a):
    """no NaN; alpha, tau and the depths in their ranges; a record that saw nothing is the empty result, bit for bit"""
    a = np.asarray(a, np.float32).reshape(-1, 4)
    alpha, tau, zf, zh = (a[:, i] for i in range(4))
    assert not np.isnan(a).any()
    assert (alpha >= 0.0).all() and (alpha <= 1.0).all() and (tau >= 0.0).all() and np.isfinite(tau).all()
    assert ((tau > 0.0) == np.isfinite(zf)).all() and ((tau > 0.0) == (alpha > 0.0)).all()
    assert (np.isfinite(zh) == (tau >= np.float32(R.LN2))).all()
    both = np.isfinite(zf) & np.isfinite(zh)
    assert (zf[both] <= zh[both]).all() and (zf[np.isfinite(zf)] >= 0.0).all()
    assert Q.is_empty(a[tau == 0.0]).all()


# ---------------------------------------------------------------------------------------------------------------- 1. the bit contract
@pytest.mark.parametrize("name", SET_NAMES)
def test_library_and_program_agree_bitwise_and_both_walks_agree(sc, api, program, tmp_path, name):
    """nrc_test_ray_aov_host (the library's host compiler) and the sanitized program (g++) run the same header: the same bits; the
    program has also walked every record with the occupancy jumps and found the same bits in all four components"""
    scene, rays = ray_sets(api, sc)[name]
    got = program_rays(program, tmp_path, scene, rays)
    lib = api.test_ray_aov_host(scene, rays)
    assert R.same_bits(got, lib)
    check_ranges(got)
    assert (got[..., 1] > 0.0).sum() > 100


@pytest.mark.parametrize("name", VIEWS + ("blocks_default", "cloud_default"))
def test_whole_camera_rays_equal_the_view_aov(sc, api, program, tmp_path, name):
    """the records nrc_camera_rays writes, walked whole, are nrc_test_view_aov_host's image bit for bit (the program compares the
    range walk with view_aov_walk itself, plain and with jumps); t_min < 0 behaves as 0"""
    if name.endswith("_default"):
        scene, cam = Q.volume_scene(sc, name.split("_")[0]), R.default_view(sc)
    else:
        scene, cam = R.cases(sc)[name]
    rays = api.camera_rays(cam, Q.W, Q.H)
    assert (rays[..., 3] == 0.0).all() and np.isposinf(rays[..., 7]).all()
    want = api.test_view_aov_host(scene, cam, Q.W, Q.H)
    assert R.same_bits(program_rays(program, tmp_path, scene, rays), want)
    for t_min in (-0.0, -3.5, -np.inf):
        neg = rays.copy()
        neg[..., 3] = t_min
        assert R.same_bits(api.test_ray_aov_host(scene, neg), want)


def test_camera_rays_of_a_sharded_frame_are_the_whole_frames_columns(sc, api):
    cam = R.orbit_view(sc, 3, aspect=72 / 32)
    whole = api.camera_rays(cam, 72, 32)
    for rank in range(3):
        part = api.camera_rays(cam, 24, 32, tile=(rank, 3, 72, 32, 8))
        cols = [((rank + (lx >> 3) * 3) << 3) + (lx & 7) for lx in range(24)]
        assert R.same_bits(part, whole[:, cols])


def _cut_points(whole, rng):
    """per record a cut T inside the medium's part of the ray: between z_front and z_front + 30 (beyond every fixture's thickness at times)"""
    zf = whole[..., 2].astype(np.float64)
    T = np.where(np.isfinite(zf), zf, 50.0) + rng.random(zf.shape) * 30.0 - 2.0
    return np.maximum(T, 0.5).astype(np.float32)


@pytest.mark.parametrize("name", ("holdout_blocks_v3", "holdout_cloud_v3", "holdout_blocks_inside", "light_cloud_other", "random_blocks", "random_cloud"))
def test_a_cut_ray_keeps_z_front_and_finite_z_half_of_the_whole_ray(sc, api, name):
    """cut at t_max = T: z_front where the cut ray has one, and z_half where the cut ray has one, carry the whole ray's bits; tau does not
    grow beyond the whole ray's; a cut that lies in front of the medium gives the empty result"""
    scene, rays = ray_sets(api, sc)[name]
    whole_rays = rays.copy()
    whole_rays[..., 7] = np.inf
    whole = api.test_ray_aov_host(scene, whole_rays)
    cut_rays = whole_rays.copy()
    cut_rays[..., 7] = _cut_points(whole, np.random.default_rng(5))
    cut = api.test_ray_aov_host(scene, cut_rays)
    check_ranges(cut)
    hit = cut[..., 1] > 0.0
    assert hit.sum() > 100 and np.isfinite(cut[..., 3]).sum() > 20
    assert R.same_bits(cut[..., 2][hit], whole[..., 2][hit])
    half = np.isfinite(cut[..., 3])
    assert R.same_bits(cut[..., 3][half], whole[..., 3][half])
    assert (cut[..., 1] <= whole[..., 1]).all()
    assert (cut[..., 1] < whole[..., 1]).sum() > 50      # (the cuts do cut)
    in_front = cut_rays[..., 7] <= whole[..., 2]
    assert Q.is_empty(cut[in_front]).all()


def test_a_permuted_list_gives_the_permuted_results(sc, api):
    scene = Q.volume_scene(sc, "cloud")
    rays = Q.random_segments(scene)
    perm = np.random.default_rng(2).permutation(rays.shape[0])
    assert R.same_bits(api.test_ray_aov_host(scene, rays[perm]), api.test_ray_aov_host(scene, rays)[perm])


def test_every_degenerate_record_gives_the_empty_result(sc, api, program, tmp_path):
    """t_max <= max(t_min, 0), a NaN in any of the eight numbers, a zero or non-finite direction, a non-finite origin, a range that holds
    no medium: {0, 0, +inf, +inf} and no NaN, from the library and from the sanitized program, on both volumes"""
    recs, what = Q.degenerate_records()
    for volume in ("blocks", "cloud"):
        scene = Q.volume_scene(sc, volume)
        lib = api.test_ray_aov_host(scene, recs)
        assert R.same_bits(lib, program_rays(program, tmp_path, scene, recs))
        bad = [w for w, e in zip(what, Q.is_empty(lib)) if not e]
        assert not bad, bad
    good = np.array([[60.0, 3.0, -2.0, 0.0, -1.0, 0.0, 0.0, np.inf]], np.float32)
    assert api.test_ray_aov_host(Q.volume_scene(sc, "cloud"), good)[0, 1] > 0.0      # (the record the degenerate ones are made from sees the cloud)
    assert api.test_ray_aov_host(Q.volume_scene(sc, "cloud"), np.zeros((0, 8), np.float32)).shape == (0, 4)


def test_a_direction_that_is_not_normalised_scales_the_parameter(sc, api):
    """rd is used as given: doubling it halves t, and every step of the arithmetic with it, exactly -- z_front halves and tau, integrated
    against t, halves too, bit for bit"""
    scene = Q.volume_scene(sc, "blocks")
    rays = Q.random_segments(scene).copy()
    rays[:, 3], rays[:, 7] = 0.0, np.inf
    one = api.test_ray_aov_host(scene, rays)
    rays[:, 4:7] *= 2.0
    two = api.test_ray_aov_host(scene, rays)
    hit = one[:, 1] > 0.0
    assert hit.sum() > 100
    assert R.same_bits(two[hit][:, 2], one[hit][:, 2] * np.float32(0.5))
    assert R.same_bits(two[hit][:, 1], one[hit][:, 1] * np.float32(0.5))


# ---------------------------------------------------------------------------------------------------------------- 2. the split check
@pytest.mark.parametrize("name", ("holdout_blocks_v3", "holdout_cloud_v3", "random_blocks"))
def test_tau_of_two_halves_adds_up_to_the_whole(sc, api, name):
    """tau[0, T] + tau[T, inf] against tau[0, inf]: within N ulp32(tau) + 8 N sigma_max ulp32(t1) -- view_aov_reference.tolerances' bound of
    one walk's rounding (N: plane crossings of the whole ray, t1: its end; no spread: the three walks follow the same fp32 ray)"""
    scene, rays = ray_sets(api, sc)[name]
    whole_rays = rays.copy()
    whole_rays[..., 3], whole_rays[..., 7] = 0.0, np.inf
    whole = api.test_ray_aov_host(scene, whole_rays)
    T = _cut_points(whole, np.random.default_rng(9))
    front, back = whole_rays.copy(), whole_rays.copy()
    front[..., 7], back[..., 3] = T, T
    a, b = api.test_ray_aov_host(scene, front), api.test_ray_aov_host(scene, back)
    ref = Q.reference_rays(scene, whole_rays, centre_only=True)
    sigma_max = float(np.float32(scene["density_factor"]))
    N = ref["crossings"].astype(np.float64)
    tau = whole[..., 1].astype(np.float64)
    bound = N * R.ulp32(tau) + 8.0 * N * sigma_max * R.ulp32(ref["t1"])
    err = np.abs(a[..., 1].astype(np.float64) + b[..., 1].astype(np.float64) - tau)
    hit = tau > 0.0
    both = (a[..., 1] > 0.0) & (b[..., 1] > 0.0)
    print("%s: %d rays split inside the medium; largest error-to-bound ratio %.3f" % (name, both.sum(), (err[hit] / bound[hit]).max()))
    assert both.sum() > 50
    assert (err[hit] <= bound[hit]).all()
    assert (err[~hit] == 0.0).all()


# ---------------------------------------------------------------------------------------------------------------- 3. the fp64 reference
@pytest.mark.parametrize("name", ACCURACY_SETS)
def test_at_most_five_percent_of_the_hit_rays_are_unstable(sc, api, name):
    un, hit = R.unstable_share(reference(api, sc, name))
    print("%s: %d unstable of %d hit rays" % (name, un, hit))
    assert hit > 100 and un <= R.UNSTABLE_CAP * hit


def _compare(got, ref, sigma_max):
    """per component: the largest error-to-bound ratio over the stable rays (finiteness must agree there)"""
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


@pytest.mark.parametrize("name", ACCURACY_SETS)
def test_host_restatement_against_the_fp64_reference_of_the_range(sc, api, name):
    """The fp32 range walk against the fp64 reference of the same fp32 record, on stable rays, within view_aov_reference.tolerances with t1
    the range's end:
        |d tau|     <= S_tau + 8 N sigma_max ulp32(t1) + N ulp32(tau)
        |d z_front| <= S_z + 8 ulp32(z)
        |d z_half|  <= S_z + tol_tau / sigma_cross + 8 ulp32(z)
        |d alpha|   <= tol_tau + 4 ulp32(1)
    (S: the reference's spread over the record's five rays, N: plane crossings inside the range).  Where a range starts or ends inside a
    voxel, z_front = t0 and the last segment's end are the record's own fp32 numbers: exact."""
    scene, rays = ray_sets(api, sc)[name]
    got = api.test_ray_aov_host(scene, rays)
    ratios = _compare(got, reference(api, sc, name), float(np.float32(scene["density_factor"])))
    print("%s: largest error-to-bound ratios %s" % (name, ratios))
    assert max(ratios.values()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 4. the ray generators
def test_light_view_is_the_documented_frame(sc):
    scene = Q.volume_scene(sc, "blocks")
    for light, margin in ((None, 1.0), (Q.OTHER_LIGHT, 1.0), ((0.0, -1.0, 0.0), 1.25), ((0.1, 0.95, 0.0), 1.0)):
        v = sc.light_view(scene, 8, 8, light_dir=light, margin=margin)
        l = np.asarray(scene["dir_light_dir"] if light is None else light, np.float64)
        l = l / np.linalg.norm(l)
        a = np.cross(l, (1.0, 0.0, 0.0) if abs(l[1]) > 0.9 else (0.0, 1.0, 0.0))
        a /= np.linalg.norm(a)
        b = np.cross(l, a)
        rad = 0.5 * Q.scene_diagonal(scene) * margin
        assert all(v[k].dtype == np.float32 and v[k].shape == (3,) for k in ("origin", "du", "dv", "dir"))
        np.testing.assert_array_equal(v["dir"], l.astype(np.float32))
        np.testing.assert_array_equal(v["origin"], (-rad * (l + a + b)).astype(np.float32))
        np.testing.assert_array_equal(v["du"], (2 * rad * a).astype(np.float32))
        np.testing.assert_array_equal(v["dv"], (2 * rad * b).astype(np.float32))
        # the square faces the light, contains the box's bounding sphere in projection, and starts in front of the box
        assert abs(np.dot(a, l)) < 1e-12 and abs(np.dot(b, l)) < 1e-12 and abs(np.dot(a, b)) < 1e-12
        assert np.dot(v["origin"].astype(np.float64), l) <= -0.5 * Q.scene_diagonal(scene) * (1 - 1e-6)
    with pytest.raises(ValueError):
        sc.light_view(scene, 8, 8, light_dir=(0.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        sc.light_view(scene, 0, 8)


def test_ortho_rays_are_the_documented_fma_chain(sc, api):
    """o_k = fma(su, du_k, fma(sv, dv_k, origin_k)) with su = (i + 0.5) / w, sv = (j + 0.5) / h in fp32; the direction as given"""
    scene = Q.volume_scene(sc, "cloud")
    view = sc.light_view(scene, 20, 12, light_dir=Q.OTHER_LIGHT)
    rays = api.ortho_rays(view, 20, 12)
    f32 = np.float32
    su = ((np.arange(20, dtype=f32) + f32(0.5)) / f32(20)).astype(f32)
    sv = ((np.arange(12, dtype=f32) + f32(0.5)) / f32(12)).astype(f32)
    SU, SV = np.meshgrid(su.astype(np.float64), sv.astype(np.float64))
    for k in range(3):      # (an fp32 product is exact in fp64; the one fp64 sum is rounded to fp32 once more: within half an ulp of the fma's)
        inner = (SV * float(view["dv"][k]) + float(view["origin"][k])).astype(f32)
        want = (SU * float(view["du"][k]) + inner.astype(np.float64)).astype(f32)
        assert np.abs(rays[..., k].astype(np.float64) - want) .max() <= np.spacing(np.abs(want).max())
        assert (rays[..., 4 + k] == view["dir"][k]).all()
    assert (rays[..., 3] == 0.0).all() and np.isposinf(rays[..., 7]).all()


# ---------------------------------------------------------------------------------------------------------------- 5. the surface
NEW_SYMBOLS = ("nrc_renderer_ray_aov", "nrc_mc_renderer_ray_aov", "nrc_renderer_view_aov_to_depth", "nrc_mc_renderer_view_aov_to_depth",
               "nrc_renderer_ortho_aov", "nrc_mc_renderer_ortho_aov", "nrc_renderer_set_path_aov_depths", "nrc_mc_renderer_set_path_aov_depths",
               "nrc_camera_rays", "nrc_ortho_rays", "nrc_test_ray_aov_host")


def test_the_new_symbols_exist_in_the_library_the_header_and_the_mirrors(api):
    import inspect
    L = api.load_library()
    header = open(os.path.join(ROOT, "include", "nrc_hpm.h")).read()
    hpp = open(os.path.join(ROOT, "include", "nrc_hpm.hpp")).read()
    assert "Ray AOV" in header and "typedef struct nrc_ortho_view" in header
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in api.ABI_SYMBOLS and s + "(" in header, s
    for cls in (api.NrcHpmRenderer, api.McHpmRenderer):
        assert callable(cls.RayAov) and callable(cls.ViewAovToDepth) and callable(cls.OrthoAov) and callable(cls.SetPathAovDepths)
    assert callable(api.camera_rays) and callable(api.ortho_rays) and callable(api.test_ray_aov_host)
    assert "aov_depths" in inspect.getsource(api._times_keyword)
    for name in ("RayAov", "ViewAovToDepth", "OrthoAov", "SetPathAovDepths"):
        assert hpp.count(name) >= 2, name
    for s in ("nrc_camera_rays", "nrc_ortho_rays"):
        assert s in hpp, s


def test_null_arguments_are_refused_and_no_rays_are_no_work(api):
    L = api.load_library()
    out = np.zeros(8, np.float32)
    assert L.nrc_camera_rays(None, 4, 4, None, out.ctypes.data) != 0
    assert L.nrc_ortho_rays(None, 4, 4, out.ctypes.data) != 0
    assert L.nrc_test_ray_aov_host(None, 1, out.ctypes.data, out.ctypes.data) != 0
    assert L.nrc_renderer_ray_aov(None, 0, None, None) != 0 and L.nrc_mc_renderer_ray_aov(None, 1, None, None) != 0


def test_the_header_is_device_free_and_states_the_range_walk_once():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-include", "nrc_view_aov.hpp", "-x", "c++", os.devnull],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-4000:]
    code = open(os.path.join(CSRC, "nrc_view_aov.hpp")).read()
    assert "hip_runtime" not in code and "__global__" not in code and "threadIdx" not in code
    assert code.count("view_aov_walk_range(") == 1 and code.count("ray_aov_ortho_ray(") == 1
    kernels = open(os.path.join(CSRC, "nrc_integrator.hip")).read()
    assert "k_ray_aov" in kernels and "view_aov_walk_range(" in kernels


def test_cli_shadow_map_and_holdout_argument_rules():
    from nrc_hpm_renderer_amd import cli
    ok = dict(aov=True, export="out_%04d.exr", gpus=1, shadow_map=None, shadow_size=512, holdout_sphere=None)
    cli.check_ray_aov_args(argparse.Namespace(export=None, gpus=1))                  # (a namespace without the flags)
    cli.check_ray_aov_args(argparse.Namespace(**ok))
    cli.check_ray_aov_args(argparse.Namespace(**dict(ok, holdout_sphere=12.5)))
    cli.check_ray_aov_args(argparse.Namespace(**dict(ok, aov=False, export=None, shadow_map="shadow.exr", gpus=4)))
    for bad in (dict(ok, aov=False, holdout_sphere=10.0), dict(ok, holdout_sphere=0.0), dict(ok, holdout_sphere=-1.0),
                dict(ok, holdout_sphere=float("nan")), dict(ok, shadow_map="s.exr", shadow_size=0), dict(ok, shadow_map="")):
        with pytest.raises(SystemExit):
            cli.check_ray_aov_args(argparse.Namespace(**bad))
    aov = -np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    planes = cli.shadow_planes(aov)
    assert sorted(planes) == ["A", "Z", "Zhalf", "tau"]
    assert planes["A"][1, 2] == aov[1, 2, 0] and planes["tau"][1, 2] == aov[1, 2, 1] and planes["Z"][0, 1] == aov[0, 1, 2] \
        and planes["Zhalf"][0, 0] == aov[0, 0, 3]
    # the analytic depth image of --holdout-sphere: the near root along unit camera rays, +inf beside the sphere
    rays = np.zeros((1, 3, 8), np.float32)
    rays[..., 0], rays[..., 4] = 50.0, -1.0
    rays[0, 1, 1] = 5.0                       # passes the centre at distance 5
    rays[0, 2, 1] = 20.0                      # misses a sphere of radius 10
    d = cli.sphere_depth(rays, 10.0)
    assert d.dtype == np.float32 and d.shape == (1, 3)
    assert d[0, 0] == 40.0 and abs(d[0, 1] - (50.0 - np.sqrt(75.0))) < 1e-4 and np.isposinf(d[0, 2])
