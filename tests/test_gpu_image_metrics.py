"""The image metrics (nrc_compare_images: k_compare_1 / _norm / _2 / _final; nrc_compare_images_sharded: + _fold / _scale / _fold_var /
_final_sharded) against the exact-sum reference of tests/image_reference.py, on the case table of tests/image_cases.py: sizes below, at
and beyond one grid-stride sweep of 256 x 256 pixels, and alpha patterns that run every branch of the valid rule (ref.w == 0 -> skip: -0.0
skipped; a denormal, NaN and negative alphas counted; no valid pixel at all; only the last pixel valid).

Bound (image_reference.metric_violations): mse, ref_mean, own_mean, own_var each within ONE fp32 ulp of the exact value rounded to fp32,
valid equal.  tests/test_image_reference_cpu.py shows that the bound rejects fp32 accumulators, a dropped tail sweep, a wrong valid rule,
a wrong divisor and a variance around the wrong mean.  Nothing here renders."""
import ctypes as C

import pytest

import image_cases as ic
import image_reference as ir

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exact():
    cache = {}

    def get(w, h, a):
        if (w, h, a) not in cache:
            cache[(w, h, a)] = ir.metrics_exact(*ic.images(w, h, a))
        return cache[(w, h, a)]
    return get


@pytest.fixture(scope="module")
def one_rank(api, torch_gpu):
    """a cache of one rank: nrc_compare_images_sharded needs no communicator, and its scratch lives here between the calls"""
    c = api.NeuralRadianceCache(api.AppConfig(train_batch_count=1, log2_train_batch_size=8))
    yield c
    c.Destroy()


def _both(api, torch, cache, w, h, a):
    ref, own = (torch.tensor(x, device="cuda") for x in ic.images(w, h, a))
    return api.CompareImages(ref, own), api.CompareImagesSharded(cache, ref, own)


@pytest.mark.parametrize("w,h,a", ic.CASES, ids=ic.CASE_IDS)
def test_metrics_equal_the_exact_sums(api, torch_gpu, one_rank, exact, w, h, a):
    want = exact(w, h, a)
    plain, sharded = _both(api, torch_gpu, one_rank, w, h, a)
    print("ulps %dx%d-%s plain %s sharded %s" % (w, h, a, ir.metric_ulps(plain, want), ir.metric_ulps(sharded, want)))
    assert ir.metric_violations(plain, want) == []
    assert ir.metric_violations(sharded, want) == []
    if ic.expected_valid(w, h, a) is not None:
        assert plain["valid"] == sharded["valid"] == ic.expected_valid(w, h, a)
    if a == "none":
        assert all(v == 0.0 for v in plain.values()) and all(v == 0.0 for v in sharded.values())


def test_no_partial_sum_survives_between_calls(api, torch_gpu, one_rank, exact):
    """the sharded scratch (block partials, raw sums, the variance sum) is kept by the cache: a large frame, then one pixel, then a frame
    without a valid pixel, then the large frame again -- every Result is that call's own"""
    for w, h, a in ((481, 409, "seeded70"), (1, 1, "all"), (200, 96, "none"), (481, 409, "seeded70"), (65537, 1, "last-only"), (481, 409, "fireflies")):
        plain, sharded = _both(api, torch_gpu, one_rank, w, h, a)
        assert ir.metric_violations(sharded, exact(w, h, a)) == [], (w, h, a)
        assert ir.metric_violations(plain, exact(w, h, a)) == [], (w, h, a)


def test_every_rank_of_a_sharded_frame_gets_the_whole_frame_s_result(api, torch_gpu):
    """four "ranks" in one process (the hook technique of test_gpu_gather.py, on plain tensors): a bright shard, a dark one, a shard of ONE
    pixel and a shard without a valid pixel.  A rank's all-reduce hook adds what the other ranks' calls left in theirs; the variance must
    be taken around the WHOLE frame's mean, which is far from every shard's own"""
    torch = torch_gpu
    ref, own, parts = ic.shards()
    want = ir.metrics_exact(ref, own)
    world = len(parts)
    r4, o4 = ref.reshape(-1, 4), own.reshape(-1, 4)
    refs = [torch.tensor(r4[p].reshape(1, -1, 4), device="cuda") for p in parts]
    owns = [torch.tensor(o4[p].reshape(1, -1, 4), device="cuda") for p in parts]
    caches = [api.NeuralRadianceCache(api.AppConfig(train_batch_count=1, log2_train_batch_size=8)) for _ in range(world)]
    keep, partial = [], {}                                             # (rank, call index) -> this rank's local sums

    def run(r, others):
        calls = []

        def allreduce(_user, buf, n, stream):
            torch.cuda.synchronize()
            t = api._wrap_device(buf, int(n) * 8, torch.float64, (int(n),))
            partial[(r, len(calls))] = t.clone()
            if others is not None:
                for k in range(world):
                    if k != r:
                        t += others[(k, len(calls))]
            calls.append(int(n))
            torch.cuda.synchronize()
            return 0

        def allgather(_user, send, recv, nbytes, stream):
            return 1                                                   # (not used by the metrics)

        hooks = (api.ALLREDUCE_F64_HOOK(allreduce), api.ALLGATHER_HOOK(allgather))
        keep.append(hooks)
        api._check(caches[r].L.nrc_cache_set_collective_hooks(caches[r].h, C.c_int(r), C.c_int(world), hooks[0], hooks[1], None))
        res = api.CompareImagesSharded(caches[r], refs[r], owns[r])
        assert calls == [4, 1]
        return res

    for r in range(world):                 # first round: every rank's pass-1 sums (pass 2 then uses a local mean: discarded)
        run(r, None)
    first = {k: v for k, v in partial.items() if k[1] == 0}
    # raw pass-1 sums of the shards, as stated: the one-pixel shard counts one pixel, the invalid shard nothing
    assert float(first[(2, 0)][3]) == 1.0 and not first[(3, 0)].any()
    for r in range(world):                 # second round, pass 1 complete: the pass-2 sums are now taken around the GLOBAL mean
        run(r, {**first, **{(k, 1): torch.zeros(1, dtype=torch.float64, device="cuda") for k in range(world)}})
    second = dict(partial)
    for r in range(world):
        res = run(r, second)
        print("ulps sharded rank %d of %d: %s" % (r, world, ir.metric_ulps(res, want)))
        assert ir.metric_violations(res, want) == [], r
    assert want["valid"] > 500
    for c in caches:
        c.Destroy()
