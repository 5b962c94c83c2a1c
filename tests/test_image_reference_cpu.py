"""tests/image_reference.py agrees with the oracle, and the bounds the GPU tests hold the kernels to bite.  The GPU tests
(test_gpu_image_metrics.py, test_gpu_composite.py) compare k_compare_* with metrics_exact within one fp32 ulp and k_composite with
composite_fp32 bit for bit.  Here, without a GPU:

  * metrics_exact equals the oracle's orc_compare on the whole case table, composite_fp32 equals orc_nrc_composite bit for bit;
  * a numpy restatement of the compare kernels (grid-stride sweeps of 256 x 256 pixels, a tree per block, a sequential fold, fp64
    throughout) is within the bound on every case, and subtly wrong variants of it are rejected by a NAMED case of the table: were the
    bound so loose that they passed, the GPU tests would show nothing;
  * the same for wrong variants of the compositing rule."""
import numpy as np
import pytest

import image_cases as ic
import image_reference as ir

f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------------------- the kernels, restated
def _device_sum(terms, acc, drop_tail=False, first_sweep=False, thread_acc=None):
    """per-pixel terms [n] -> the sum as k_compare_1 / _2 + the fold form it: every thread adds its pixels sweep by sweep, a block's 256
    threads are folded by halving, the 256 block sums are added in order -- all in `acc` (thread_acc: the threads' own sums in another type)"""
    n = terms.shape[0]
    sweeps = max(1, -(-n // ic.SWEEP))
    t = np.zeros(sweeps * ic.SWEEP, f64)
    t[:n] = terms
    if drop_tail:
        t[ic.SWEEP * (n // ic.SWEEP):] = 0.0
    t = t.reshape(sweeps, ic.SWEEP)
    if first_sweep:
        t = t[:1]
    ta = thread_acc or acc
    thread = np.zeros(ic.SWEEP, ta)
    for s in range(t.shape[0]):
        thread = (thread + t[s]).astype(ta)
    b = thread.astype(acc).reshape(256, 256).copy()
    off = 128
    while off >= 1:
        b[:, :off] = b[:, :off] + b[:, off:2 * off]
        off >>= 1
    return np.cumsum(b[:, 0], dtype=acc)[-1]


SUM_SWITCHES = ("drop_tail", "first_sweep", "thread_acc")


def _valid(ref, flush_alpha=False, negzero_valid=False):
    a = np.ascontiguousarray(ref, f32).reshape(-1, 4)[:, 3]
    if negzero_valid:
        return a.view(np.uint32) != 0                                  # a compare of the bits: -0.0 is not 0
    if flush_alpha:
        a = np.where(np.abs(a) < np.finfo(f32).tiny, f32(0.0), a)      # denormals read as zero
    return ~(a == f32(0.0))


def _pass1(ref, own, acc=f64, **how):
    """raw {sq err, ref sum, own sum, valid count} of one image or shard"""
    sums = {k: how.pop(k) for k in SUM_SWITCHES if k in how}
    r, o = np.ascontiguousarray(ref, f32).reshape(-1, 4), np.ascontiguousarray(own, f32).reshape(-1, 4)
    v = _valid(r, **how)
    r3, o3 = r[:, :3].astype(f64), o[:, :3].astype(f64)
    d = o3 - r3
    se = np.where(v, d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2], 0.0)
    rs = np.where(v, r3[:, 0] + r3[:, 1] + r3[:, 2], 0.0)
    os_ = np.where(v, o3[:, 0] + o3[:, 1] + o3[:, 2], 0.0)
    return [f64(_device_sum(x, acc, **sums)) for x in (se, rs, os_, v.astype(f64))], v


def _pass2(own, v, mean, acc=f64, **sums):
    o3 = np.ascontiguousarray(own, f32).reshape(-1, 4)[:, :3].astype(f64)
    e = o3 - f64(mean)
    return f64(_device_sum(np.where(v, e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2], 0.0), acc, **sums))


def kernel_metrics(ref, own, acc=f64, div_valid=False, var_around_ref=False, **how):
    """nrc_compare_images as csrc/nrc_integrator.hip states it (k_compare_1, _norm, _2, _final); keywords switch one mistake on"""
    sums = {k: how[k] for k in SUM_SWITCHES if k in how}
    (se, rs, os_, cnt), v = _pass1(ref, own, acc, **how)
    inv = (1.0 / (cnt if div_valid else cnt * 3.0)) if cnt > 0 else 0.0
    mean = os_ * inv
    var = _pass2(own, v, rs * inv if var_around_ref else mean, acc, **sums)
    return dict(mse=float(f32(se * inv)), ref_mean=float(f32(rs * inv)), own_mean=float(f32(mean)), own_var=float(f32(var * inv)),
                valid=float(f32(cnt)))


def kernel_metrics_sharded(ref, own, parts, own_shard_mean=False):
    """nrc_compare_images_sharded on every rank: pass 1 per shard (k_compare_1, _fold), the raw sums added over the ranks, k_compare_scale,
    pass 2 around the GLOBAL mean (k_compare_2, _fold_var), added over the ranks, k_compare_final_sharded"""
    r, o = np.asarray(ref).reshape(-1, 4), np.asarray(own).reshape(-1, 4)
    first = [_pass1(r[p], o[p]) for p in parts]
    se, rs, os_, cnt = [sum((f[0][k] for f in first), f64(0.0)) for k in range(4)]
    inv = 1.0 / (cnt * 3.0) if cnt > 0 else 0.0
    var = f64(0.0)
    for p, (s, v) in zip(parts, first):
        mean = os_ * inv
        if own_shard_mean:
            mean = s[2] / (3.0 * s[3]) if s[3] > 0 else 0.0
        var += _pass2(o[p], v, mean)
    return dict(mse=float(f32(se * inv)), ref_mean=float(f32(rs * inv)), own_mean=float(f32(os_ * inv)), own_var=float(f32(var * inv)),
                valid=float(f32(cnt)))


@pytest.fixture(scope="module")
def exact():
    cache = {}

    def get(w, h, a):
        if (w, h, a) not in cache:
            cache[(w, h, a)] = ir.metrics_exact(*ic.images(w, h, a))
        return cache[(w, h, a)]
    return get


# ---------------------------------------------------------------------------------------------------------------- the metric reference
def test_metrics_exact_on_hand_worked_images():
    ref = np.array([[[1.0, 2.0, 3.0, 1.0], [9.0, 9.0, 9.0, 0.0], [0.0, 0.0, 0.0, -0.0], [0.5, 0.5, 0.5, 1e-45], [4.0, 4.0, 4.0, np.nan]]], f32)
    own = np.array([[[2.0, 2.0, 5.0, 1.0], [7.0, 7.0, 7.0, 1.0], [1.0, 1.0, 1.0, 1.0], [0.5, 1.5, 0.5, 0.0], [4.0, 4.0, 1.0, 0.0]]], f32)
    m = ir.metrics_exact(ref, own)      # valid: pixels 0, 3, 4 -- nine numbers
    assert m["valid"] == 3.0
    inv = 1.0 / 9.0      # (the sums are multiplied by 1 / (3 valid), as norm.comp does)
    assert m["mse"] == (1 + 0 + 4 + 0 + 1 + 0 + 0 + 0 + 9) * inv
    assert m["ref_mean"] == (6 + 1.5 + 12) * inv and m["own_mean"] == (9 + 2.5 + 9) * inv
    mean = 20.5 * inv
    assert abs(m["own_var"] - sum((x - mean) ** 2 for x in (2, 2, 5, 0.5, 1.5, 0.5, 4, 4, 1)) * inv) < 1e-15
    assert ir.metrics_exact(ref[:, 1:3], own[:, 1:3]) == dict(mse=0.0, ref_mean=0.0, own_mean=0.0, own_var=0.0, valid=0.0)
    # exact sums: a term below the running sum's last bit is not lost
    big = np.zeros((1, 3, 4), f32)
    big[..., 3] = 1.0
    o = big.copy()
    o[0, 0, 0], o[0, 1, 0], o[0, 2, 0] = 2.0 ** 60, 1.0, -2.0 ** 60
    assert ir.metrics_exact(big, o)["own_mean"] == 1.0 * inv
    assert ir.ulp_distance(1.0, np.nextafter(f32(1.0), f32(2.0))) == 1 and ir.ulp_distance(0.0, -0.0) == 0
    assert ir.ulp_distance(-1e-45, 1e-45) == 2 and ir.ulp_distance(np.nan, 1.0) == float("inf")


def test_the_table_holds_what_it_says():
    assert len(ic.CASES) == 54
    for w, h, a in ic.CASES:
        ref, own = ic.images(w, h, a)
        assert ref.shape == own.shape == (h, w, 4) and (ref[..., :3] >= 0).all() and (own >= 0).all() and np.isfinite(own).all()
        want = ic.expected_valid(w, h, a)
        got = int(ir.valid_pixels(ref).sum())
        assert want is None and 0.6 * w * h <= got <= 0.8 * w * h + 1 or got == want, (w, h, a, got, want)
    assert 481 * 409 == 3 * ic.SWEEP + 121
    ref, own = ic.images(481, 409, "fireflies")
    assert own[..., :3].mean() > 100 * ref[..., :3].mean()
    ref, own, parts = ic.shards()
    assert [p.size for p in parts][2:] == [1, 1] and ir.valid_pixels(ref)[parts[2]].all() and not ir.valid_pixels(ref)[parts[3]].any()
    o = own.reshape(-1, 4)
    assert o[parts[0], :3].mean() > 100 * o[parts[1], :3].mean()


@pytest.mark.parametrize("w,h,a", ic.CASES, ids=ic.CASE_IDS)
def test_metrics_exact_agrees_with_the_oracle(orc, exact, w, h, a):
    ref, own = ic.images(w, h, a)
    got, want = orc.compare(ref, own), exact(w, h, a)
    print(ic.CASE_IDS[ic.CASES.index((w, h, a))], "oracle ulps from the exact sums:", ir.metric_ulps(got, want))
    assert ir.metric_violations(got, want) == []


@pytest.mark.parametrize("w,h,a", ic.CASES, ids=ic.CASE_IDS)
def test_the_restated_kernels_are_within_the_bound(exact, w, h, a):
    got = kernel_metrics(*ic.images(w, h, a))
    assert ir.metric_violations(got, exact(w, h, a)) == []


def test_the_restated_sharded_kernels_are_within_the_bound():
    ref, own, parts = ic.shards()
    assert ir.metric_violations(kernel_metrics_sharded(ref, own, parts), ir.metrics_exact(ref, own)) == []
    assert ir.metric_violations(kernel_metrics_sharded(ref, own, parts[::-1]), ir.metrics_exact(ref, own)) == []


# ---------------------------------------------------------------------------------------------------------------- the metric bound bites
# mutant -> (the switch, the case of the table that must reject it)
METRIC_MUTANTS = {
    "fp32-accumulators": (dict(acc=f32), (481, 409, "fireflies")),
    "last-partial-sweep-dropped": (dict(drop_tail=True), (65537, 1, "last-only")),
    "only-the-first-sweep": (dict(first_sweep=True), (65537, 1, "all")),
    "alpha-denormals-flushed": (dict(flush_alpha=True), (200, 96, "cycle")),
    "negative-zero-valid": (dict(negzero_valid=True), (257, 1, "cycle")),
    "divided-by-valid": (dict(div_valid=True), (1, 1, "all")),
    "variance-around-ref-mean": (dict(var_around_ref=True), (481, 409, "fireflies")),
}


@pytest.mark.parametrize("name", list(METRIC_MUTANTS))
def test_wrong_metric_kernels_are_rejected(exact, name):
    how, named = METRIC_MUTANTS[name]
    why = ir.metric_violations(kernel_metrics(*ic.images(*named), **how), exact(*named))
    print(name, "rejected by %dx%d-%s:" % named, why)
    assert why, (name, named)
    # ... and by how much of the table (the three-sweep size and the sizes around one sweep are enough to see every mutant)
    by = [i for (w, h, a), i in zip(ic.CASES, ic.CASE_IDS) if w * h <= ic.SWEEP + 1 and a != "none"
          and ir.metric_violations(kernel_metrics(*ic.images(w, h, a), **how), exact(w, h, a))]
    print(name, "also rejected by:", by)


def test_a_variance_around_each_shard_s_own_mean_is_rejected():
    ref, own, parts = ic.shards()
    why = ir.metric_violations(kernel_metrics_sharded(ref, own, parts, own_shard_mean=True), ir.metrics_exact(ref, own))
    print(why)
    assert any(x.startswith("own_var") for x in why) and len(why) == 1


def test_fp32_accumulators_fail_without_fireflies_too():
    """the bound does not lean on the firefly case: plain uniform images at three sweeps reject fp32 sums"""
    assert ir.metric_violations(kernel_metrics(*ic.images(481, 409, "all"), acc=f32), ir.metrics_exact(*ic.images(481, 409, "all")))


def test_what_one_ulp_cannot_see_and_zero_would():
    """the record for a later 1 -> 0 tightening: a kernel whose THREADS sum in fp32 (the block tree and the fold in fp64) stays within one ulp
    on the whole table -- a thread adds at most four pixels, and 65 536 such roundings average out far below fp32's resolution -- but is off
    by exactly one ulp where a single pixel is valid and its sum is rounded twice"""
    worst, seen_by_zero = 0, []
    for (w, h, a), i in zip(ic.CASES, ic.CASE_IDS):
        u = ir.metric_ulps(kernel_metrics(*ic.images(w, h, a), thread_acc=f32), ir.metrics_exact(*ic.images(w, h, a)))
        worst = max(worst, max(u.values()))
        if max(u.values()) > 0:
            seen_by_zero.append(i)
    print("fp32 thread sums: worst %d ulp, non-zero on %s" % (worst, seen_by_zero))
    assert worst == 1 and any(i.endswith("last-only") for i in seen_by_zero)


# ---------------------------------------------------------------------------------------------------------------- compositing
def composite_inputs(W, H, seed, other_info=False):
    """primary, info, radiance (x * H + y order; negative, NaN and infinite entries among it) of one synthetic frame"""
    rng = np.random.default_rng(seed)
    primary = rng.random((H, W, 4), dtype=f32)
    info = (rng.random((H, W)) < 0.6).astype(f32)
    if other_info:
        info[rng.random((H, W)) < 0.3] = f32(2.0)
    y = rng.standard_normal((W * H, 3)).astype(f32)
    y[rng.random(W * H) < 0.1] = np.nan
    y[rng.random(W * H) < 0.05, 1] = np.inf
    y[rng.random(W * H) < 0.05, 2] = -np.inf
    return primary, info, y


def composite_rule(primary, info, y_lin, prev, k, show_nrc, fma=False, clamp=True, gate_nonzero=False, row_major=False, ib_ratio=False):
    """frame k (1-based) of a blend chain; keywords switch one mistake on"""
    H, W = prev.shape[:2]
    p = primary.reshape(H, W, 4)
    y = y_lin.reshape(H, W, 3) if row_major else y_lin.reshape(W, H, 3).transpose(1, 0, 2)
    live = (info != f32(0.0)) if gate_nonzero else (info == f32(1.0))

    def mad(a, b, c):      # a * b + c: two roundings, or one
        return (a.astype(f64) * f64(b) + c.astype(f64)).astype(f32) if fma else a * b + c
    with np.errstate(invalid="ignore", over="ignore"):
        yc = np.fmax(f32(0.0), y) if clamp else np.where(np.isnan(y), f32(0.0), y)
        c = np.concatenate([p[..., :3], np.ones((H, W, 1), f32)], axis=2)
        if show_nrc:
            c[..., :3] = np.where(live.reshape(H, W, 1), mad(yc, p[..., 3:4], p[..., :3]), p[..., :3])
        bf = f32(1.0) / f32(k)
        ib = f32(k - 1) / f32(k) if ib_ratio else f32(1.0) - bf
        return mad(c, bf, ib * prev)


def _chain(orc, W, H, show_nrc, other_info=False, **mutation):
    """five chained frames: (reference image, oracle image, rule image)"""
    a, b, c = (np.zeros((H, W, 4), f32) for _ in range(3))
    for k in range(1, 6):
        primary, info, y = composite_inputs(W, H, 100 + k, other_info)
        a = ir.composite_fp32(primary, info, y, a, f32(1.0) / f32(k), show_nrc)
        if orc is not None:
            b = orc.nrc_composite(W, H, show_nrc, float(f32(1.0) / f32(k)), primary, info, y, b.copy())
        c = composite_rule(primary, info, y, c, k, show_nrc, **mutation)
    return a, b, c


@pytest.mark.parametrize("show_nrc", [1, 0])
@pytest.mark.parametrize("other_info", [False, True], ids=["info01", "info012"])
def test_composite_fp32_equals_the_oracle_bit_for_bit(orc, show_nrc, other_info):
    a, b, c = _chain(orc, 7, 5, show_nrc, other_info)
    assert ir.same_bits(a, b) and ir.same_bits(a, c)
    assert np.isfinite(a).all() == (show_nrc == 0)      # (an infinite radiance stays in the blend; a NaN or -Inf one adds nothing)
    assert np.isfinite(a).mean() > 0.5 and not np.isnan(a).any() and (a[..., 3] == 1.0).mean() > 0.5


# mutant -> (the switch, the chain that must reject it: frame size, info values)
COMPOSITE_MUTANTS = {
    "contracted-to-one-fma": (dict(fma=True), (7, 5, False)),
    "no-clamp": (dict(clamp=False), (7, 5, False)),
    "gate-info-nonzero": (dict(gate_nonzero=True), (7, 5, True)),
    "radiance-indexed-row-major": (dict(row_major=True), (7, 5, False)),
    "ib-as-ratio": (dict(ib_ratio=True), (7, 5, False)),
}


@pytest.mark.parametrize("name", list(COMPOSITE_MUTANTS))
def test_wrong_compositing_rules_are_rejected(name):
    how, (W, H, other_info) = COMPOSITE_MUTANTS[name]
    a, _, c = _chain(None, W, H, 1, other_info, **how)
    differing = int(((a.view(np.uint32) != c.view(np.uint32)) & ~(np.isnan(a) & np.isnan(c))).any(axis=2).sum())
    print(name, "differs in %d of %d pixels" % (differing, W * H))
    assert differing > 0
    if name == "gate-info-nonzero":      # (a frame whose info holds only 0 and 1 cannot tell the two gates apart)
        a, _, c = _chain(None, W, H, 1, False, **how)
        assert ir.same_bits(a, c)
    if name == "ib-as-ratio":            # 1 - 1/3 and 2/3 round differently; 1/2 and 1/4 do not
        assert f32(1.0) - f32(1.0) / f32(3.0) != f32(2.0) / f32(3.0)
