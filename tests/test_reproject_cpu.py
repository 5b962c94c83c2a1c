"""Reprojection (include/nrc_hpm.h, "Reproject"; csrc/nrc_reproject.hpp), the parts that need no GPU: the host restatement
(nrc_test_reproject_host) against the sanitized program and against the fp64 statement, the exact rules, and what carrying the accumulated
frame from view to view buys on the CPU oracle's Monte-Carlo frames.  tests/cpp/reproject_main.cpp -- its own main, the device-free header
alone, ASan + UBSan without recovery -- is built once and run directly; nothing is loaded into Python under a sanitizer."""
import argparse
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import reproject_reference as R

V = R.V
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nrc-hpm-renderer_amd", "csrc")
FRAMES = 4.0

_RENDERED = {}


def rendered(sc, orc, api, name):
    """what the tests of a rendered case share, computed once per session: the orbit's cameras, every view's guide (the library's host walk of
    the view AOV), its blend of 4 oracle frames per seed (the renderers' blend: frame k enters with weight 1 / k) and its 1024-frame truth"""
    if name not in _RENDERED:
        scene, cam0 = V.cases(sc)[name]
        cams = R.orbit(sc)
        assert np.array_equal(cams[0]["inv_proj_view"], cam0["inv_proj_view"])      # (the orbit starts at the case's own view)
        guides = [api.test_view_aov_host(scene, c, R.W, R.H) for c in cams]
        blends = {}
        for seed in R.QUALITY_SEEDS:
            rnd = sc.frame_randoms(R.ORBIT_VIEWS * R.ORBIT_FRAMES, seed=seed)
            blends[seed] = []
            for i, c in enumerate(cams):
                acc = np.zeros((R.H, R.W, 4), np.float32)
                for k in range(R.ORBIT_FRAMES):
                    orc.mc_render(scene, c, R.W, R.H, R.PATH_LENGTH, rnd[i * R.ORBIT_FRAMES + k], blend=1.0 / (k + 1), out=acc, threads=8)
                blends[seed].append(acc.copy())
        truths = []
        for c in cams:
            t = np.zeros((R.H, R.W, 4), np.float64)
            for fr in sc.frame_randoms(R.TRUTH_FRAMES, seed=R.TRUTH_SEED):
                t += orc.mc_render(scene, c, R.W, R.H, R.PATH_LENGTH, fr, blend=1.0, threads=8)[0]
            truths.append(t / R.TRUTH_FRAMES)
        _RENDERED[name] = dict(cams=cams, guides=guides, blends=blends, truths=truths)
    return _RENDERED[name]


def camera_floats(cam):
    return [float(x) for x in np.asarray(cam["inv_proj_view"], np.float32).reshape(16)] + [float(x) for x in np.asarray(cam["pos"], np.float32)]


@pytest.fixture(scope="module")
def program():
    build = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "reproject_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "reproject_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def run(tmp_path, hist, rgba, frames, aov, cam, p):
        h, w = rgba.shape[:2]
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<3I4f", w, h, 1 if hist is not None else 0, p["max_history"], p["sigma_alpha"], p["sigma_depth"], frames))
            f.write(struct.pack("<38f", *(camera_floats(cam) + camera_floats(hist[3] if hist is not None else cam))))
            f.write(np.ascontiguousarray(rgba, "<f4").tobytes() + np.ascontiguousarray(aov, "<f4").tobytes())
            if hist is not None:
                f.write(np.ascontiguousarray(hist[0], "<f4").tobytes() + np.ascontiguousarray(hist[1], "<f4").tobytes() +
                        np.ascontiguousarray(hist[2], "<f4").tobytes())
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600, env=env)
        out = r.stdout + r.stderr
        assert r.returncode == 0, out[-4000:]
        assert "AddressSanitizer" not in out and "runtime error" not in out and "FAILED" not in out, out[-4000:]
        both = np.fromfile(dst, "<f4")
        return both[:h * w * 4].reshape(h, w, 4), both[h * w * 4:].reshape(h, w)
    return run


def small_images():
    """the 9 x 7 cut of the 48 x 32 synthetic images, non-finite colours made finite"""
    cut = [np.ascontiguousarray(a[10:17, 20:29]) for a in R.synthetic(48, 32)]
    cut[0] = np.where(np.isfinite(cut[0]), cut[0], np.float32(1.0))
    return tuple(cut)


def pair_same(a, b):
    return R.same_bits(a[0], b[0]) and R.same_bits(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------- 1. program == library
@pytest.mark.parametrize("w,h", R.SYNTHETIC_SIZES)
def test_library_and_program_agree_bitwise_on_the_synthetic_images(api, sc, program, tmp_path, w, h):
    """nrc_test_reproject_host (the library's host compiler) and the sanitized program (g++) run the same header: the same bits, for every
    camera pair, with a max_history that bites, and without history"""
    rgba, aov, hr, hn, ha = R.synthetic(w, h)
    for name, (hcam, cam) in R.camera_pairs(sc, w, h).items():
        for p in (R.params(), R.params(max_history=8.0, sigma_depth=1.5)):
            hist = (hr, hn, ha, hcam)
            assert pair_same(program(tmp_path, hist, rgba, FRAMES, aov, cam, p), api.test_reproject_host(hist, rgba, FRAMES, aov, cam, p)), (name, p)
    cam = R.camera_pairs(sc, w, h)["orbit2"][1]
    assert pair_same(program(tmp_path, None, rgba, FRAMES, aov, cam, R.params()), api.test_reproject_host(None, rgba, FRAMES, aov, cam, R.params()))


@pytest.mark.parametrize("name", R.RENDERED)
def test_library_and_program_agree_bitwise_on_rendered_frames(sc, orc, api, program, tmp_path, name):
    r = rendered(sc, orc, api, name)
    hist = None
    for i in range(3):      # (chained: view 1's history is view 0's output, view 2's is view 1's)
        got = api.test_reproject_host(hist, r["blends"][3][i], FRAMES, r["guides"][i], r["cams"][i], R.params())
        assert pair_same(program(tmp_path, hist, r["blends"][3][i], FRAMES, r["guides"][i], r["cams"][i], R.params()), got), i
        hist = (got[0], got[1], r["guides"][i], r["cams"][i])


# ---------------------------------------------------------------------------------------------------------------- 2. host against fp64
def solve_errors(cam, hcam, aov, w, h):
    """(position error in pixels, distance error) of the fp32 solve against the fp64 solve, the largest over the medium's pixels"""
    g = np.asarray(aov, np.float64)
    medium = g[..., 0] != 0.0
    z = np.where(medium, R.representative_depth(g), 0.0)
    a, b = R.solve_f64(cam, hcam, z, w, h), R.solve_f32(cam, hcam, z, w, h)
    assert (a["front"] == b["front"])[medium].all()
    pos = max(float(np.abs(a["fx"] - b["fx"])[medium].max()), float(np.abs(a["fy"] - b["fy"])[medium].max()))
    assert float(np.linalg.norm(np.asarray(cam["pos"], np.float64)) + z.max()) <= R.SCALE      # (L = |ro| + z of the derivation)
    return pos, float(np.abs(a["dist"] - b["dist"])[medium].max())


def error_ratios(api, hist, rgba, frames, aov, cam, p, terms=("alpha", "depth")):
    """the largest error-to-bound ratios (colour, count) of the host against the fp64 statement; no pixel is excluded"""
    out, cnt = api.test_reproject_host(hist, rgba, frames, aov, cam, p)
    want, want_n, aux = R.reproject_fp64(hist, rgba, frames, aov, cam, p, terms)
    bc, bn = R.bounds(aux, frames, p)
    fin = np.isfinite(np.asarray(rgba)[..., :3]).all(axis=-1)
    assert R.same_bits(out[~fin], np.asarray(rgba, np.float32)[~fin])
    err = np.abs(out[..., :3].astype(np.float64)[fin] - want[..., :3][fin]).max(axis=-1)
    err_n = np.abs(cnt.astype(np.float64) - want_n)
    assert np.isfinite(err).all() and np.isfinite(err_n).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        rc = np.where(err > 0.0, err / bc[fin], 0.0)
        rn = np.where(err_n > 0.0, err_n / bn, 0.0)
    return float(rc.max()), float(rn.max())


def test_host_restatement_against_fp64(sc, orc, api):
    """The host restatement against the fp64 statement (reproject_reference.reproject_fp64), every pixel.  The bound, from the arithmetic
    (u = 2^-24, first order in u):
      position      the fp32 solve.  X = fma(z, rd, ro): rd within 3 u per component of the exact ray (view_aov_camera_ray's 1e-7 rad and
                    the fp32 u, v), so |dX| <= 4 u z + u |X| <= 5 u L with L = |ro| + z <= SCALE; D = X - pos_hist one more rounding; the
                    chain of q_k rounds three times and N's entries are fp32 numbers (the library's own fp64 inverse may round an entry the
                    other way: one more u): |dq_k| <= 9 u |N_k| L.  sx = q_0 / q_2: |dsx| <= (|dq_0| + |sx| |dq_2|) / |q_2| + u |sx|
                    <= 9 u kappa (1 + |sx|) with kappa = |N_k| L / |q_2| <= 5 for these cameras (the medium lies in front of the history
                    camera at a third of L or more) and |sx| <= 1 inside the image: |dsx| <= 90 u, and fx = (sx + 1) w / 2 moves by
                    eps_pos = 45 u max(w, h) pixels.  dist = |D|: |d dist| <= |dD| + 3 u |D| <= EPS_DIST = 9 u SCALE.
                    Both are MEASURED below (solve_f32: the header's chain operation for operation in numpy float32, against solve_f64) and
                    asserted: largest position error 2.3e-5 pixels against eps_pos = 2.6e-4 at 97 x 41, largest distance error 1.7e-5
                    against 1.1e-4.
      weights       the bilinear weights are products of per-axis hat functions of the position, which are 1-Lipschitz and sum to 1 along
                    each axis: over all taps sum |db| <= 2 eps_pos + 2 eps_pos -- also where floor(fx) differs between the two codes, the
                    taps that come or go having b <= eps_pos on each side (this is the rule's continuity; no pixel is excluded).  Per tap
                    d: |dd| <= EPS_DIST inv_sz + 4 u d, through exp(-d) (d e^-d <= 0.37) <= EPS_DIST inv_sz + 1.5 u; nrc_expm1_negf 4 u (an
                    exact 1 from 17.5 on, where e^-d < u); 1 - e and the product with b one u each, twice for the taps of two sets:
                    E_w = sum |dwgt| <= 4 eps_pos + EPS_DIST inv_sz + 48 u.
      the mean      around the centre: |d acc_c| <= E_w Cd + 2 u C W + 4 u Cd W (Cd: the largest |c_Q - c_P|, C: the largest component,
                    W = acc_w), |dW| <= E_w + 4 u W; q = acc_c / acc_w, |q| <= Cd: |dq| <= 2 E_w Cd / W + 2 u C + 9 u Cd.
      the count     |d acc_n| <= Nmax (E_w + 5 u W); min(., max_history) is 1-Lipschitz; a = n_h / (n_h + n): |da| <= |dn_h| / n + 2 u, and
                    a <= min(1, Nmax W / n) -- a poorly matched history (small W) has a small a, which cancels the 1 / W of dq.
      out           fma(a, q, c_P): |d out| <= a |dq| + |q| |da| + u (|a q| + |c_P|)
                        <= E_w Cd (2 min(1 / W, Nmax / n) + Nmax / n) + u (3 C + 12 Cd + 5 Cd Nmax W / n)
                    out_n = n_h + n: |d out_n| <= Nmax (E_w + 5 u W) + u (max_history + n).
    Cd, C and Nmax are taken over the usable history pixels of the 4 x 4 window around the fp64 position: every tap of either code.
    Largest error-to-bound ratios measured: colour 2.6e-3, count 1.3e-2 (the solve: 0.088 of eps_pos, 0.16 of EPS_DIST): the position
    term is a worst case over the roundings of the solve, which measure a tenth of it, and the typical tap has a contrast well below Cd."""
    ratios, solve = {}, {}
    for w, h in R.SYNTHETIC_SIZES + (R.SMALL,):
        rgba, aov, hr, hn, ha = small_images() if (w, h) == R.SMALL else R.synthetic(w, h)
        for name, (hcam, cam) in R.camera_pairs(sc, w, h).items():
            pos, dist = solve_errors(cam, hcam, aov, w, h)
            solve[w, h, name] = (pos / R.eps_pos(w, h), dist / R.EPS_DIST)
            for tag, p in (("default", R.params()), ("cap 8", R.params(max_history=8.0, sigma_depth=1.5))):
                ratios[w, h, name, tag] = error_ratios(api, (hr, hn, ha, hcam), rgba, FRAMES, aov, cam, p)
    for name in R.RENDERED:
        r = rendered(sc, orc, api, name)
        hist = None
        for i in range(R.ORBIT_VIEWS):
            if i > 0:
                pos, dist = solve_errors(r["cams"][i], r["cams"][i - 1], r["guides"][i], R.W, R.H)
                solve[name, i] = (pos / R.eps_pos(R.W, R.H), dist / R.EPS_DIST)
            ratios[name, i] = error_ratios(api, hist, r["blends"][4][i], FRAMES, r["guides"][i], r["cams"][i], R.params())
            out, cnt = api.test_reproject_host(hist, r["blends"][4][i], FRAMES, r["guides"][i], r["cams"][i], R.params())
            hist = (out, cnt, r["guides"][i], r["cams"][i])
    worst_solve = (max(v[0] for v in solve.values()), max(v[1] for v in solve.values()))
    worst = (max(v[0] for v in ratios.values()), max(v[1] for v in ratios.values()))
    print("fp32 solve against fp64, largest (position / eps_pos, distance / EPS_DIST): %.3f %.3f" % worst_solve)
    print("largest error-to-bound ratios (colour, count): %.2e %.2e" % worst)
    assert max(worst_solve) <= 1.0
    assert max(worst) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 3. the rules
def test_without_history_the_frame_comes_back(api, sc):
    rgba, aov, _, _, _ = R.synthetic(44, 36)
    out, cnt = api.test_reproject_host(None, rgba, 3.0, aov, V.orbit_view(sc, 3, aspect=44 / 36))
    assert R.same_bits(out, rgba) and (cnt == np.float32(3.0)).all()


def test_pass_through_rules_are_bitwise(api, sc):
    """sky and non-finite current pixels, a history that is all sky, a history camera that looks away and a history displaced in depth by
    17.5 sigma_depth or more: out is the current frame bit for bit, the count is `frames`"""
    rgba, aov, hr, hn, ha = R.synthetic(44, 36)
    pairs = R.camera_pairs(sc, 44, 36)
    sky = aov[..., 0] == 0.0
    bad = ~np.isfinite(rgba[..., :3]).all(axis=-1)
    assert sky.sum() > 100 and bad.sum() == 2
    for name, (hcam, cam) in pairs.items():
        out, cnt = api.test_reproject_host((hr, hn, ha, hcam), rgba, FRAMES, aov, cam)
        through = sky | bad
        assert R.same_bits(out[through], rgba[through]) and (cnt[through] == np.float32(FRAMES)).all(), name
        assert R.same_bits(out[..., 3], rgba[..., 3])
        assert np.isfinite(out[~through]).all() and np.isfinite(cnt).all()
        changed = (out[..., :3].view(np.uint32) != rgba[..., :3].view(np.uint32)).any(axis=-1)
        assert changed[~through].mean() > 0.8 and (cnt[~through] > FRAMES).mean() > 0.8, name
    hcam, cam = pairs["orbit2"]

    def comes_back(hist):
        out, cnt = api.test_reproject_host(hist, rgba, FRAMES, aov, cam)
        return R.same_bits(out, rgba) and bool((cnt == np.float32(FRAMES)).all())
    all_sky = np.empty_like(ha)
    all_sky[...] = (0.0, 0.0, np.inf, np.inf)
    assert comes_back((hr, hn, all_sky, hcam))
    pos = np.asarray(hcam["pos"], np.float64)
    away = sc.make_camera(pos=pos, view_dir=pos, aspect=44 / 36)      # (its back to the medium: q_2 ww <= 0 for every point of it)
    assert comes_back((hr, hn, ha, away))
    far = ha.copy()
    far[..., 2:] += np.float32(200.0)      # (|z_Q - dist| >= 17.5 * 4 for every pair of pixels: every weight is an exact 0)
    assert comes_back((hr, hn, far, hcam))
    assert not comes_back((hr, hn, ha, hcam))


def test_a_constant_colour_comes_back_bit_for_bit(api, sc):
    """a constant colour in history and current, any camera pair, any counts: every difference c_Q - c_P is an exact 0"""
    _, aov, _, hn, ha = R.synthetic(97, 41)
    rgba = np.empty((41, 97, 4), np.float32)
    rgba[...] = (0.7371, 2.913, 0.01234, 0.5)
    for name, (hcam, cam) in R.camera_pairs(sc, 97, 41).items():
        for p in (R.params(), R.params(max_history=8.0)):
            out, cnt = api.test_reproject_host((rgba, hn, ha, hcam), rgba, FRAMES, aov, cam, p)
            assert R.same_bits(out, rgba), name
            assert (cnt > FRAMES).mean() > 0.7


def test_one_nan_history_pixel_stays_local(api, sc):
    """the history with its NaN pixel against the same history with that pixel finite but skipped (its guide alpha 0): the same bits
    everywhere; against the history with the pixel finite and used: only pixels whose taps can include it differ; no NaN comes out"""
    rgba, aov, hr, hn, ha = R.synthetic(48, 32)
    rgba = np.where(np.isfinite(rgba), rgba, np.float32(1.0))
    y, x = [tuple(q) for q in R.D.nonfinite_pixels(hr) if np.isnan(hr[q[0], q[1]]).any()][0]
    skipped_c, skipped_g, used = hr.copy(), ha.copy(), hr.copy()
    skipped_c[y, x, :3] = 1.0
    skipped_g[y, x] = (0.0, 0.0, np.inf, np.inf)
    used[y, x, :3] = 1.0
    for name, (hcam, cam) in R.camera_pairs(sc, 48, 32).items():
        a = api.test_reproject_host((hr, hn, ha, hcam), rgba, FRAMES, aov, cam)
        assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
        assert pair_same(a, api.test_reproject_host((skipped_c, hn, skipped_g, hcam), rgba, FRAMES, aov, cam)), name
        b = api.test_reproject_host((used, hn, ha, hcam), rgba, FRAMES, aov, cam)
        differs = (a[0].view(np.uint32) != b[0].view(np.uint32)).any(axis=-1) | (a[1].view(np.uint32) != b[1].view(np.uint32))
        s = R.solve_f32(cam, hcam, np.where(aov[..., 0] != 0.0, R.representative_depth(aov.astype(np.float64)), 0.0), 48, 32)
        with np.errstate(invalid="ignore"):
            near = (np.floor(s["fx"]) <= x) & (x <= np.floor(s["fx"]) + 1) & (np.floor(s["fy"]) <= y) & (y <= np.floor(s["fy"]) + 1)
        assert differs.sum() >= 1 and not (differs & ~near).any(), name


def test_the_count_is_capped(api, sc):
    rgba, aov, hr, hn, ha = R.synthetic(48, 32)
    for name, (hcam, cam) in R.camera_pairs(sc, 48, 32).items():
        for cap in (8.0, 64.0):
            _, cnt = api.test_reproject_host((hr, hn, ha, hcam), rgba, FRAMES, aov, cam, R.params(max_history=cap))
            assert cnt.max() <= np.float32(cap) + np.float32(FRAMES) and cnt.min() >= np.float32(FRAMES)
        _, cnt = api.test_reproject_host((hr, hn, ha, hcam), rgba, FRAMES, aov, cam, R.params(max_history=8.0))
        if name == "same":      # (the cap bites: the counts run up to 40, and with equal cameras most pixels find their own history pixel)
            assert (cnt == np.float32(12.0)).mean() > 0.3


def test_infinite_sigmas_give_exact_zero_terms(api, sc):
    """sigma = +inf: the term is an exact 0 whatever the guides say -- the same bits over a history guide whose depths (alphas) are others --
    and the result is the fp64 statement's that never forms the term"""
    rgba, aov, hr, hn, ha = R.synthetic(48, 32)
    hcam, cam = R.camera_pairs(sc, 48, 32)["orbit2"]
    solid = ha[..., 0] != 0.0
    other_z, other_a = ha.copy(), ha.copy()
    other_z[solid, 2:] += np.float32(7.25)
    other_a[solid, 0] = 0.5
    inf = math.inf
    for other, key, terms in ((other_z, "sigma_depth", ("alpha",)), (other_a, "sigma_alpha", ("depth",))):
        off = R.params(**{key: inf})
        assert pair_same(api.test_reproject_host((hr, hn, ha, hcam), rgba, FRAMES, aov, cam, off),
                         api.test_reproject_host((hr, hn, other, hcam), rgba, FRAMES, aov, cam, off)), key
        assert not pair_same(api.test_reproject_host((hr, hn, ha, hcam), rgba, FRAMES, aov, cam),
                             api.test_reproject_host((hr, hn, other, hcam), rgba, FRAMES, aov, cam)), key
        assert max(error_ratios(api, (hr, hn, ha, hcam), rgba, FRAMES, aov, cam, off, terms=terms)) <= 1.0
    both = R.params(sigma_alpha=inf, sigma_depth=inf)
    assert max(error_ratios(api, (hr, hn, ha, hcam), rgba, FRAMES, aov, cam, both, terms=())) <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 4. the mean
@pytest.mark.parametrize("cap", [64.0, 8.0])
def test_equal_cameras_and_guides_give_the_count_weighted_mean(api, sc, cap):
    """history and current seen by one camera over one guide: every pixel projects onto itself, so out = (n_h c_h + n c) / (n_h + n) with
    n_h = min(history count, max_history) and out_n = n_h + n -- within the bound of the host against the fp64 statement (relative, for
    the count).  Where the history pixel itself cannot be used the mean is the current pixel (n_h = 0), within the same bound: the fp32
    position is a rounding beside the pixel's centre, and a neighbour enters with a weight of that size.  Sky and non-finite current pixels
    come through bit for bit."""
    w, h = 97, 41
    rgba, aov, hr, hn, _ = R.synthetic(w, h)
    cam = V.orbit_view(sc, 3, aspect=w / h)
    p = R.params(max_history=cap)
    out, cnt = api.test_reproject_host((hr, hn, aov, cam), rgba, FRAMES, aov, cam, p)
    _, _, aux = R.reproject_fp64((hr, hn, aov, cam), rgba, FRAMES, aov, cam, p)
    bc, bn = R.bounds(aux, FRAMES, p)
    use = (aov[..., 0] != 0.0) & np.isfinite(rgba[..., :3]).all(axis=-1)
    n_h = np.where(np.isfinite(hr[..., :3]).all(axis=-1), np.minimum(hn.astype(np.float64), cap), 0.0)
    mean = (n_h[..., None] * np.where(np.isfinite(hr[..., :3]), hr[..., :3], np.float32(0.0)).astype(np.float64) + FRAMES * rgba[..., :3].astype(np.float64)) / (n_h + FRAMES)[..., None]
    err = np.abs(out[..., :3].astype(np.float64)[use] - mean[use]).max(axis=-1)
    err_n = np.abs(cnt.astype(np.float64) - (n_h + FRAMES))[use]
    print("equal cameras, cap %g: largest error-to-bound ratios %.2e (colour) %.2e (count)" % (cap, (err / bc[use]).max(), (err_n / bn[use]).max()))
    assert use.sum() > 0.8 * w * h
    assert (err <= bc[use] + 1e-12).all() and (err_n <= bn[use] + 1e-12).all()
    assert (err_n / (n_h + FRAMES)[use]).max() <= (bn[use] / (n_h + FRAMES)[use]).max()
    assert R.same_bits(out[~use], rgba[~use]) and (cnt[~use] == np.float32(FRAMES)).all()


# ---------------------------------------------------------------------------------------------------------------- 5. quality
@pytest.mark.parametrize("name", R.RENDERED)
def test_quality_on_an_orbit_of_oracle_frames(sc, orc, api, name):
    """An orbit of 8 views 2 degrees apart, 4 oracle frames per view (48 x 32, path length 32), carried from view to view through
    nrc_test_reproject_host with the default parameters: MSE(accumulated) / MSE(raw 4-frame image) at the last view, against the mean of
    1024 frames (seed 99) of that view.  Measured with the fp64 statement (reproject_reference.step_fp64) chained the same way:
        cloud_v3   seed 3  0.162   seed 4  0.106        blocks_v3  seed 3  0.229   seed 4  0.371
    (the host restatement gives the same figures to four digits).  Asserted: every ratio <= 1.5 x the largest = 0.557 -- a condition on
    these inputs, not a general claim -- and at most 2 % of the medium's pixels of the last view without history (measured: 0.25 % and
    0 %).  The bias, MSE(reproject(truth chain), truth): cloud_v3 2.2e-4, blocks_v3 2.7e-4, against a raw 4-frame MSE of 8.9e-3 and
    7.9e-3."""
    r = rendered(sc, orc, api, name)
    truth = r["truths"][-1]
    medium = r["guides"][-1][..., 0] != 0.0
    assert medium.sum() > 200
    ratios, shares = {}, {}
    for seed in R.QUALITY_SEEDS:
        acc, cnt = R.chain(api.test_reproject_host, r["blends"][seed], r["guides"], r["cams"], FRAMES, R.params())
        ratios[seed] = R.mse(acc, truth) / R.mse(r["blends"][seed][-1], truth)
        shares[seed] = float((cnt[medium] == np.float32(FRAMES)).mean())
        assert R.same_bits(acc[~medium], r["blends"][seed][-1][~medium])
        assert cnt.max() <= R.ORBIT_VIEWS * FRAMES * (1.0 + 1e-5)      # (never more frames than were rendered)
        acc64, _ = R.chain(R.step_fp64, r["blends"][seed], r["guides"], r["cams"], FRAMES, R.params())
        assert abs(R.mse(acc64, truth) / R.mse(r["blends"][seed][-1], truth) - ratios[seed]) < 1e-3
    bias, _ = R.chain(api.test_reproject_host, [t.astype(np.float32) for t in r["truths"]], r["guides"], r["cams"], FRAMES, R.params())
    print("%s: MSE ratios by seed %s; medium pixels without history %s; MSE(reproject(truth chain), truth) %.2e" %
          (name, {k: round(v, 3) for k, v in ratios.items()}, shares, R.mse(bias, truth)))
    for seed in R.QUALITY_SEEDS:
        assert abs(ratios[seed] - R.MEASURED_RATIOS[name, seed]) < 2e-3      # (the figures the bound was made from)
    assert max(ratios.values()) <= R.QUALITY_BOUND < 0.6
    assert max(shares.values()) <= R.NO_HISTORY_CAP


# ---------------------------------------------------------------------------------------------------------------- 6. the surface
NEW_SYMBOLS = ("nrc_reproject_params_default", "nrc_reproject", "nrc_test_reproject_host", "nrc_renderer_set_path_reproject_target",
               "nrc_mc_renderer_set_path_reproject_target")


def test_the_new_symbols_exist_in_the_library_the_header_and_the_mirrors(api, sc):
    L = api.load_library()
    header = open(os.path.join(ROOT, "include", "nrc_hpm.h")).read()
    hpp = open(os.path.join(ROOT, "include", "nrc_hpm.hpp")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s) and s in api.ABI_SYMBOLS and s + "(" in header, s
        assert s + "(" in hpp or s.startswith("nrc_test_"), s
    for cls in (api.NrcHpmRenderer, api.McHpmRenderer):
        assert callable(cls.SetPathReprojectTarget)
    assert callable(api.Reproject) and callable(api.test_reproject_host) and callable(sc.reproject_params)
    assert hpp.count("SetPathReprojectTarget") >= 2 and "inline void Reproject(" in hpp


def test_the_header_is_device_free_and_in_the_build_id():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-include", "nrc_reproject.hpp", "-x", "c++", os.devnull],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-4000:]
    code = open(os.path.join(CSRC, "nrc_reproject.hpp")).read()
    assert "hip_runtime" not in code and "__global__" not in code and "threadIdx" not in code
    make = open(os.path.join(CSRC, "Makefile")).read()
    srcs = make[make.index("SRCS ="):make.index("HIPCC_VERSION")]
    assert "REPROJECT_HDRS = nrc_reproject.hpp" in make and "$(REPROJECT_HDRS)" in srcs
    for obj in ("nrc_integrator.o:", "nrc_api.o:"):
        line = [l for l in make.splitlines() if obj in l][0]
        assert "$(REPROJECT_HDRS)" in line, obj


def test_the_defaults_and_argument_validation(api, sc):
    p = api.make_c_reproject_params()
    assert (p.max_history, p.sigma_alpha, p.sigma_depth) == (64.0, np.float32(0.1), 4.0)
    assert sc.reproject_params() == R.DEFAULTS and sc.reproject_params(max_history=8)["max_history"] == 8.0
    rgba, aov, hr, hn, ha = R.synthetic(48, 32)
    hcam, cam = R.camera_pairs(sc, 48, 32)["orbit2"]
    hist = (hr, hn, ha, hcam)
    nan, inf = math.nan, math.inf
    bad = [dict(max_history=0.0), dict(max_history=-1.0), dict(max_history=inf), dict(max_history=nan), dict(sigma_alpha=0.0),
           dict(sigma_alpha=-1.0), dict(sigma_alpha=nan), dict(sigma_depth=0.0), dict(sigma_depth=nan), dict(sigma_depth=-inf),
           dict(sigma_alpha=1e-42), dict(sigma_depth=1e-42)]
    for kw in bad:
        with pytest.raises(RuntimeError, match="reproject"):
            api.test_reproject_host(hist, rgba, FRAMES, aov, cam, R.params(**kw))
    for kw in bad[:-2]:      # (the last two are refused for an inverse that fp32 cannot hold: the library's check alone)
        with pytest.raises(ValueError):
            sc.reproject_params(**kw)
    for kw in (dict(sigma_alpha=inf, sigma_depth=inf), dict(max_history=1e-3), dict(max_history=1e30)):
        api.test_reproject_host(hist, rgba, FRAMES, aov, cam, R.params(**kw))
    for frames in (0.0, -1.0, nan, inf):
        with pytest.raises(RuntimeError, match="frames"):
            api.test_reproject_host(hist, rgba, frames, aov, cam)
    with pytest.raises(ValueError):
        api.make_c_reproject_params(dict(sigma=1.0))
    with pytest.raises(ValueError):
        api.test_reproject_host((hr, hn, ha), rgba, FRAMES, aov, cam)
    # a singular history camera: no inverse of [A B C]
    flat = dict(inv_proj_view=np.zeros(16, np.float32), pos=hcam["pos"])
    with pytest.raises(RuntimeError, match="singular"):
        api.test_reproject_host((hr, hn, ha, flat), rgba, FRAMES, aov, cam)
    api.test_reproject_host(None, rgba, FRAMES, aov, flat)      # (without history the current camera is not inverted)
    # the C entry points: half a history, in place, null
    L = api.load_library()
    C = api.C
    c, g = np.ascontiguousarray(rgba), np.ascontiguousarray(aov)
    out, cnt = np.empty_like(c), np.empty(c.shape[:2], np.float32)
    ccam, chcam = api.make_c_camera(cam), api.make_c_camera(hcam)

    def call(h0, h1, h2, h3, o=out, n=cnt):
        ptr = lambda a: None if a is None else (C.byref(a) if isinstance(a, api.NrcCamera) else a.ctypes.data_as(C.c_void_p))
        return L.nrc_test_reproject_host(ptr(h0), ptr(h1), ptr(h2), ptr(h3), ptr(c), C.c_float(FRAMES), ptr(g), C.byref(ccam), 48, 32, C.byref(p),
                                         ptr(o), ptr(n))
    hr_, hn_, ha_ = np.ascontiguousarray(hr), np.ascontiguousarray(hn), np.ascontiguousarray(ha)
    assert call(hr_, hn_, ha_, chcam) == 0 and call(None, None, None, None) == 0
    for half in ((hr_, None, ha_, chcam), (hr_, hn_, None, chcam), (hr_, hn_, ha_, None), (None, hn_, ha_, chcam), (None, None, None, chcam)):
        assert call(*half) == -1 and b"all or none" in L.nrc_last_error(), half
    for o, n in ((c, cnt), (hr_, cnt), (g, cnt), (ha_, cnt), (out, hn_), (out, out[0].reshape(-1)[:1])):
        assert call(hr_, hn_, ha_, chcam, o=o, n=n) == -1 and b"in-place" in L.nrc_last_error()
    assert L.nrc_reproject(None, None, None, None, None, C.c_float(FRAMES), None, None, 48, 32, C.byref(p), None, None, None) == -1


def test_cli_reproject_argument_rules():
    from nrc_hpm_renderer_amd import cli
    ns = argparse.Namespace
    cli.check_reproject_args(ns(export=None, gpus=1))                                  # (a namespace without the flag)
    cli.check_reproject_args(ns(reproject=None, orbit=None, export=None, gpus=4, holdout_sphere=None))
    cli.check_reproject_args(ns(reproject=64.0, orbit=8, export="out_%04d.exr", gpus=1, holdout_sphere=None, denoise=3))
    cli.check_reproject_args(ns(reproject=8.0, orbit=64, export="o%d.exr", gpus=1, holdout_sphere=None))
    ok = dict(reproject=64.0, orbit=8, export="out_%04d.exr", gpus=1, holdout_sphere=None)
    for change in (dict(orbit=None), dict(export=None), dict(export="a.exr"), dict(gpus=2), dict(holdout_sphere=8.0), dict(reproject=0.0),
                   dict(reproject=-3.0), dict(reproject=math.inf), dict(reproject=math.nan)):
        with pytest.raises(SystemExit):
            cli.check_reproject_args(ns(**dict(ok, **change)))
