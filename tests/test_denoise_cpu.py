"""The denoise filter (include/nrc_hpm.h, "Denoise"; csrc/nrc_denoise.hpp), the parts that need no GPU: the host restatement
(nrc_test_denoise_host) against the fp64 statement per pass, the pass-through rules, and what the filter buys on the CPU oracle's Monte-Carlo
frames.  tests/cpp/denoise_main.cpp -- its own main, the device-free header alone, ASan + UBSan without recovery -- is built once and run
directly; nothing is loaded into Python under a sanitizer."""
import argparse
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import denoise_reference as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nrc-hpm-renderer_amd", "csrc")

_RENDERED = {}


def rendered(sc, orc, name):
    """what the tests of a rendered case share, computed once per session: the guide, the running blends of 16 frames per seed (the
    renderers' blend: frame k enters with weight 1 / k) and the 1024-frame truth"""
    if name not in _RENDERED:
        scene, cam = D.V.cases(sc)[name]
        blends = {}
        for seed in D.QUALITY_SEEDS:
            acc = np.zeros((D.H, D.W, 4), np.float32)
            for k, fr in enumerate(sc.frame_randoms(max(D.QUALITY_FRAMES), seed=seed), 1):
                orc.mc_render(scene, cam, D.W, D.H, D.PATH_LENGTH, fr, blend=1.0 / k, out=acc, threads=8)
                if k in D.QUALITY_FRAMES:
                    blends[seed, k] = acc.copy()
        truth = np.zeros((D.H, D.W, 4), np.float64)
        for fr in sc.frame_randoms(D.TRUTH_FRAMES, seed=D.TRUTH_SEED):
            truth += orc.mc_render(scene, cam, D.W, D.H, D.PATH_LENGTH, fr, blend=1.0, threads=8)[0]
        _RENDERED[name] = dict(guide=D.reference_guide(sc, name), blends=blends, truth=truth / D.TRUTH_FRAMES)
    return _RENDERED[name]


@pytest.fixture(scope="module")
def program():
    build = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "denoise_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "denoise_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def run(tmp_path, rgba, aov, p):
        h, w = rgba.shape[:2]
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<3I4f", w, h, p["passes"], p["sigma_alpha"], p["sigma_depth"], p["sigma_color"], p["color_decay"]))
            f.write(np.ascontiguousarray(rgba, "<f4").tobytes() + np.ascontiguousarray(aov, "<f4").tobytes())
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600, env=env)
        out = r.stdout + r.stderr
        assert r.returncode == 0, out[-4000:]
        assert "AddressSanitizer" not in out and "runtime error" not in out and "FAILED" not in out, out[-4000:]
        return np.fromfile(dst, "<f4").reshape(h, w, 4)
    return run


COLOUR_ON = dict(sigma_color=1.5, color_decay=0.5)


# ---------------------------------------------------------------------------------------------------------------- 1. program == library
@pytest.mark.parametrize("w,h", D.SYNTHETIC_SIZES)
def test_library_and_program_agree_bitwise_on_the_synthetic_images(api, program, tmp_path, w, h):
    """nrc_test_denoise_host (the library's host compiler) and the sanitized program (g++) run the same header: the same bits, for 1 .. 6
    passes and with the colour term on"""
    rgba, aov = D.synthetic(w, h)
    for p in [D.params(passes=n) for n in range(1, 7)] + [D.params(passes=3, **COLOUR_ON)]:
        assert D.same_bits(program(tmp_path, rgba, aov, p), api.test_denoise_host(rgba, aov, p)), p


@pytest.mark.parametrize("name", D.RENDERED)
def test_library_and_program_agree_bitwise_on_rendered_frames(sc, orc, api, program, tmp_path, name):
    r = rendered(sc, orc, name)
    for key in ((3, 1), (4, 4)):
        for p in (D.params(), D.params(passes=2, **COLOUR_ON)):
            assert D.same_bits(program(tmp_path, r["blends"][key], r["guide"], p), api.test_denoise_host(r["blends"][key], r["guide"], p))


# ---------------------------------------------------------------------------------------------------------------- 2. host against fp64
def per_pass_ratio(api, rgba, aov, p, terms=("alpha", "depth", "color")):
    """the largest error-to-bound ratio of the host's passes, each against the fp64 pass on the host's OWN input of that pass"""
    worst = 0.0
    cur = np.asarray(rgba, np.float32)
    for k in range(p["passes"]):
        nxt = api.test_denoise_host(rgba, aov, dict(p, passes=k + 1))
        s, inv_sa, inv_sz, inv_sc = D.pass_constants(p, k)
        want, aux = D.pass_fp64(cur, aov, s, inv_sa, inv_sz, inv_sc, terms)
        bound = D.pass_bound(aux, inv_sc)[..., None]
        f = aux["filtered"]
        with np.errstate(invalid="ignore", divide="ignore"):      # (the copied non-finite pixels)
            err = np.abs(nxt[..., :3].astype(np.float64) - want[..., :3])
            ratio = np.where(err > 0.0, err / bound, 0.0)
        assert np.isfinite(err[f]).all()
        worst = max(worst, float(ratio[f].max()))
        cur = nxt
    return worst


def test_host_restatement_against_fp64_per_pass(sc, orc, api):
    """Every pass of the host restatement against the fp64 pass (denoise_reference.pass_fp64) on the host's own input of that pass, so that
    errors do not compound.  The bound, from the arithmetic alone (u = 2^-24, first order in u; the colours here are non-negative):
      per kept tap   d: one product and two fma, |dd| <= 3 u d, plus the luminances' three roundings each through the colour term,
                     <= 6 u L inv_sc (L: the largest |lum| among the taps); through exp(-d): <= e^-d (3 u d + 6 u L inv_sc) <= 1.2 u + 6 u L inv_sc;
                     nrc_expm1_negf: 4 ulp of a number below 1, <= 4 u;  1 - e: <= u;  the product with k: <= u.
                     |dw| <= k (8 u + 6 u L inv_sc), and the k sum to at most 1:  E_w = sum |dw| <= 8 u + 6 u L inv_sc.
      numerator      the mean is formed around the centre: 25 differences c_Q - c_P (|.| <= C for non-negative colours, C the largest
                     component among the taps; a rounding each) and 25 fma: |dN| <= C E_w + u C D + 25 u C D   (D: the sum of the weights)
      denominator    25 sums: |dD| <= E_w + 25 u D
      one division   q = N / D, |q| <= C:  |dq| <= |dN| / D + |q| |dD| / D + u |q| <= u C ((16 + 12 L inv_sc) / D + 52)
      one sum        out = c_P + q: one more rounding, <= u C:   |d out| <= u C ((16 + 12 L inv_sc) / D + 53).
    Largest error-to-bound ratios measured: synthetic 48 x 32 default 0.035, colour term on 0.019, six passes 0.035; 97 x 41 0.041;
    cloud_v3 0.031, blocks_v3 0.027."""
    ratios = {}
    rgba, aov = D.synthetic(48, 32)
    ratios["synthetic default"] = per_pass_ratio(api, rgba, aov, D.params())
    ratios["synthetic colour"] = per_pass_ratio(api, rgba, aov, D.params(**COLOUR_ON))
    ratios["synthetic six passes"] = per_pass_ratio(api, rgba, aov, D.params(passes=6))
    ratios["synthetic 97x41"] = per_pass_ratio(api, *D.synthetic(97, 41), D.params())
    for name in D.RENDERED:
        r = rendered(sc, orc, name)
        ratios[name] = per_pass_ratio(api, r["blends"][3, 4], r["guide"], D.params())
    print("largest error-to-bound ratios: %s" % ratios)
    assert max(ratios.values()) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 3. the rules
@pytest.mark.parametrize("p", [D.params(), D.params(passes=6), D.params(passes=2, **COLOUR_ON)], ids=["default", "six", "colour"])
def test_pass_through_rules_are_bitwise(api, p):
    """alpha == 0 pixels, non-finite pixels and the alpha channel come through bit for bit; every other pixel is finite"""
    rgba, aov = D.synthetic(44, 36)
    out = api.test_denoise_host(rgba, aov, p)
    sky = aov[..., 0] == 0.0
    bad = ~np.isfinite(rgba[..., :3]).all(axis=-1)
    assert sky.sum() > 100 and bad.sum() == 2
    assert D.same_bits(out[sky], rgba[sky])
    assert D.same_bits(out[bad], rgba[bad])
    assert D.same_bits(out[..., 3], rgba[..., 3])
    assert np.isfinite(out[~sky & ~bad]).all()
    changed = (out[..., :3].view(np.uint32) != rgba[..., :3].view(np.uint32)).any(axis=-1)
    assert changed[~sky & ~bad].mean() > 0.9 and not changed[sky | bad].any()


def test_one_nan_pixel_changes_no_other_pixel(api):
    """the image with its NaN pixel against the same image with that pixel finite but skipped (its guide alpha 0): every other pixel has
    the same bits, after every number of passes"""
    rgba, aov = D.synthetic(48, 32)
    y, x = [tuple(q) for q in D.nonfinite_pixels(rgba) if np.isnan(rgba[q[0], q[1]]).any()][0]
    rgba2, aov2 = rgba.copy(), aov.copy()
    rgba2[y, x, :3] = 1.0
    aov2[y, x] = (0.0, 0.0, np.inf, np.inf)
    others = np.ones(rgba.shape[:2], bool)
    others[y, x] = False
    for n in (1, 3, 6):
        a, b = api.test_denoise_host(rgba, aov, D.params(passes=n)), api.test_denoise_host(rgba2, aov2, D.params(passes=n))
        assert D.same_bits(a[others], b[others]), n
        assert np.isnan(a[y, x, 1]) and D.same_bits(b[y, x], rgba2[y, x])


def test_a_constant_colour_over_a_constant_guide_stays_within_one_ulp(api):
    """The filtered image of a constant colour over a constant guide against the colour: within 1 ulp -- and, because the mean is formed
    around the centre pixel (every difference c_Q - c_P is an exact 0, so out = c_P + 0 / acc_w), bit for bit, at the image's edges too, after
    any number of passes and with the colour term on.  (Summing wgt c_Q itself gave 2 ulp after one pass, 4 after six and 5 after three
    with the colour term on for this colour, which is no power of two.)"""
    rgba = np.empty((23, 37, 4), np.float32)
    rgba[...] = (0.7371, 2.913, 0.01234, 0.5)
    aov = np.empty_like(rgba)
    aov[...] = (0.6, 0.9163, 55.0, 56.0)
    worst = {}
    for name, p in (("one pass", D.params(passes=1)), ("six passes", D.params(passes=6)), ("colour on", D.params(passes=3, **COLOUR_ON))):
        out = api.test_denoise_host(rgba, aov, p)
        ulps = np.abs(out[..., :3].view(np.int32).astype(np.int64) - rgba[..., :3].view(np.int32).astype(np.int64))
        worst[name] = int(ulps.max())
        print("%s: components by ulp %s" % (name, np.bincount(ulps.ravel())))
        assert D.same_bits(out[..., 3], rgba[..., 3])
    assert max(worst.values()) <= 1, worst
    assert max(worst.values()) == 0, worst


def test_infinite_sigmas_give_exact_zero_terms(api):
    """sigma = +inf: the result is that of the formula without the term.  Depth and alpha: bit for bit the result over a guide whose z_front
    (alpha) is constant where defined, where the term is an exact 0 by itself.  Colour (the default): within the per-pass bound of the
    fp64 statement that never forms the term."""
    rgba, aov = D.synthetic(48, 32)
    solid = aov[..., 0] != 0.0
    flat_z, flat_a = aov.copy(), aov.copy()
    flat_z[solid, 2] = 60.0
    flat_a[solid, 0] = 0.5
    inf = math.inf
    assert D.same_bits(api.test_denoise_host(rgba, aov, D.params(sigma_depth=inf)), api.test_denoise_host(rgba, flat_z, D.params()))
    assert D.same_bits(api.test_denoise_host(rgba, aov, D.params(sigma_alpha=inf)), api.test_denoise_host(rgba, flat_a, D.params()))
    assert not D.same_bits(api.test_denoise_host(rgba, aov, D.params()), api.test_denoise_host(rgba, flat_z, D.params()))
    assert per_pass_ratio(api, rgba, aov, D.params(), terms=("alpha", "depth")) <= 1.0
    # (and with all three off the filter is the plain a-trous kernel over the usable pixels)
    assert per_pass_ratio(api, rgba, aov, D.params(sigma_alpha=inf, sigma_depth=inf), terms=()) <= 1.0


def test_strides_beyond_the_image(api, program, tmp_path):
    """6 passes on 9 x 7: from stride 4 on most taps, from stride 16 on all but the centre, lie outside"""
    rgba, aov = D.synthetic(48, 32)
    rgba, aov = np.ascontiguousarray(rgba[10:17, 20:29]), np.ascontiguousarray(aov[10:17, 20:29])
    rgba[...] = np.where(np.isfinite(rgba), rgba, 1.0)
    assert (aov[..., 0] != 0.0).sum() > 40
    p = D.params(passes=6)
    out = api.test_denoise_host(rgba, aov, p)
    assert np.isfinite(out).all()
    assert D.same_bits(out, program(tmp_path, rgba, aov, p))
    assert per_pass_ratio(api, rgba, aov, p) <= 1.0
    five, six = api.test_denoise_host(rgba, aov, D.params(passes=5)), out      # (stride 32: the centre tap alone, w c / w)
    ulps = np.abs(six[..., :3].view(np.int32).astype(np.int64) - five[..., :3].view(np.int32).astype(np.int64))
    assert ulps.max() <= 1


# ---------------------------------------------------------------------------------------------------------------- 4. quality
@pytest.mark.parametrize("name", D.RENDERED)
def test_quality_on_oracle_frames(sc, orc, api, name):
    """MSE(denoised) / MSE(raw) against the mean of 1024 frames (seed 99), default parameters, for blends of 1, 4 and 16 oracle frames of
    seeds 3 and 4: every ratio <= 0.5.  The fp64 statement gave at most 0.230 on these inputs; the bound has a factor 2 of room and is a
    condition on these inputs, not a general claim."""
    r = rendered(sc, orc, name)
    ratios = {}
    for key, img in sorted(r["blends"].items()):
        ratios[key] = D.mse(api.test_denoise_host(img, r["guide"], D.params()), r["truth"]) / D.mse(img, r["truth"])
    bias = D.mse(api.test_denoise_host(r["truth"].astype(np.float32), r["guide"], D.params()), r["truth"])
    print("%s: MSE ratios (seed, frames) %s; MSE(filter(truth), truth) %.2e" % (name, {k: round(v, 3) for k, v in ratios.items()}, bias))
    assert len(ratios) == 6
    assert max(ratios.values()) <= D.QUALITY_BOUND
    sky = r["guide"][..., 0] == 0.0
    assert sky.sum() > 50
    for img in r["blends"].values():
        assert D.same_bits(api.test_denoise_host(img, r["guide"], D.params())[sky], img[sky])


# ---------------------------------------------------------------------------------------------------------------- 5. the surface
NEW_SYMBOLS = ("nrc_denoise_params_default", "nrc_denoise_scratch_bytes", "nrc_denoise", "nrc_test_denoise_host", "nrc_renderer_denoised_frame",
               "nrc_mc_renderer_denoised_frame", "nrc_renderer_set_path_denoise_target", "nrc_mc_renderer_set_path_denoise_target",
               "nrc_renderer_export_exr_denoised", "nrc_mc_renderer_export_exr_denoised")


def test_the_new_symbols_exist_in_the_library_the_header_and_the_mirrors(api, sc):
    L = api.load_library()
    header = open(os.path.join(ROOT, "include", "nrc_hpm.h")).read()
    hpp = open(os.path.join(ROOT, "include", "nrc_hpm.hpp")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in api.ABI_SYMBOLS and s + "(" in header, s
    for cls in (api.NrcHpmRenderer, api.McHpmRenderer):
        assert callable(cls.DenoisedFrame) and callable(cls.SetPathDenoiseTarget) and callable(cls.ExportDenoisedImageToFile)
    assert callable(api.Denoise) and callable(api.test_denoise_host) and callable(sc.denoise_params)
    for name in ("DenoisedFrame", "ExportDenoisedImageToFile", "SetPathDenoiseTarget"):
        assert hpp.count(name) >= 2, name
    assert "inline void Denoise(" in hpp


def test_the_header_is_device_free_and_in_the_build_id():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-include", "nrc_denoise.hpp", "-x", "c++", os.devnull],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-4000:]
    code = open(os.path.join(CSRC, "nrc_denoise.hpp")).read()
    assert "hip_runtime" not in code and "__global__" not in code and "threadIdx" not in code
    make = open(os.path.join(CSRC, "Makefile")).read()
    srcs = make[make.index("SRCS ="):make.index("HIPCC_VERSION")]
    assert "DENOISE_HDRS = nrc_denoise.hpp" in make and "$(DENOISE_HDRS)" in srcs
    for obj in ("nrc_integrator.o:", "nrc_api.o:"):
        line = [l for l in make.splitlines() if obj in l][0]
        assert "$(DENOISE_HDRS)" in line, obj


def test_the_defaults_and_parameter_validation(api, sc):
    p = api.make_c_denoise_params()
    assert (p.passes, p.sigma_alpha, p.sigma_depth, p.color_decay) == (3, np.float32(0.1), 4.0, 0.5) and math.isinf(p.sigma_color) and p.sigma_color > 0
    assert sc.denoise_params() == D.DEFAULTS and sc.denoise_params(passes=5, sigma_color=2.0)["sigma_color"] == 2.0
    L = api.load_library()
    rgba, aov = D.synthetic(48, 32)
    nan = math.nan
    bad = [dict(passes=0), dict(passes=7), dict(sigma_alpha=0.0), dict(sigma_alpha=-1.0), dict(sigma_alpha=nan), dict(sigma_depth=0.0),
           dict(sigma_depth=nan), dict(sigma_depth=-math.inf), dict(sigma_color=0.0), dict(sigma_color=nan), dict(color_decay=0.0),
           dict(color_decay=1.5), dict(color_decay=nan), dict(sigma_alpha=1e-42), dict(passes=6, sigma_color=1e-37, color_decay=0.01)]
    for kw in bad:
        with pytest.raises(RuntimeError, match="denoise"):
            api.test_denoise_host(rgba, aov, D.params(**kw))
        assert L.nrc_denoise_scratch_bytes(48, 32, api.C.byref(api.make_c_denoise_params(D.params(**kw)))) == 0, kw
    for kw in bad[:-2]:      # (the last two are refused for an inverse that fp32 cannot hold: the library's check alone)
        with pytest.raises(ValueError):
            sc.denoise_params(**kw)
    for kw in (dict(sigma_alpha=math.inf, sigma_depth=math.inf), dict(color_decay=1.0, sigma_color=3.0), dict(passes=6), dict(passes=1)):
        api.test_denoise_host(rgba, aov, D.params(**kw))
    px = 48 * 32
    for n, want in ((1, 8 * px), (2, 24 * px), (3, 40 * px), (6, 40 * px)):
        assert L.nrc_denoise_scratch_bytes(48, 32, api.C.byref(api.make_c_denoise_params(dict(passes=n)))) == want
    assert L.nrc_denoise_scratch_bytes(0, 32, api.C.byref(p)) == 0
    c = np.ascontiguousarray(rgba)
    assert L.nrc_test_denoise_host(c.ctypes.data, np.ascontiguousarray(aov).ctypes.data, 48, 32, api.C.byref(p), c.ctypes.data) == -1      # in place
    assert b"in-place" in L.nrc_last_error()
    assert L.nrc_denoise(None, None, 48, 32, api.C.byref(p), None, None, None) == -1
    with pytest.raises(ValueError):
        api.make_c_denoise_params(dict(sigma=1.0))


def test_cli_denoise_argument_rules():
    from nrc_hpm_renderer_amd import cli
    ns = argparse.Namespace
    cli.check_denoise_args(ns(export=None, gpus=1))                                  # (a namespace without the flag)
    cli.check_denoise_args(ns(denoise=None, export=None, gpus=4, holdout_sphere=None))
    cli.check_denoise_args(ns(denoise=3, export="out_%04d.exr", gpus=1, holdout_sphere=None, aov=True))
    cli.check_denoise_args(ns(denoise=6, export="a.exr", gpus=1, holdout_sphere=None, aov=False))
    for bad in (dict(denoise=3, export=None, gpus=1, holdout_sphere=None), dict(denoise=3, export="a.exr", gpus=2, holdout_sphere=None),
                dict(denoise=3, export="a.exr", gpus=1, holdout_sphere=8.0), dict(denoise=0, export="a.exr", gpus=1, holdout_sphere=None),
                dict(denoise=7, export="a.exr", gpus=1, holdout_sphere=None)):
        with pytest.raises(SystemExit):
            cli.check_denoise_args(ns(**bad))
