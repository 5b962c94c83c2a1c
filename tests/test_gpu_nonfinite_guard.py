"""The training guard (include/nrc_hpm.h, nrc_cache_set_nonfinite_policy): with NRC_NONFINITE_SKIP a training step whose loss or gradient
is not finite is the identity on weights, EMA weights and Adam moments, is counted, and every other step is bit for bit what it is without
the guard.  "Bad" batches here are NUMBERS -- a NaN target, a finite gradient beyond fp16's range -- that the kernels handle as IEEE
values; nothing faults.  All comparisons are bitwise: the contract (a skipped step consumes its step number) makes the run with a skipped
step k equal the run without that batch and SetStep(k) in its place."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import nrc_debug

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODELS = dict(m6x64=dict(), m8x128=dict(nn_width=128, nn_depth=8), hashgrid=dict(pos_id=0, hashgrid_log2_size=12, nn_depth=3))
SETS = ("w", "ema", "m", "v")


def queries(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((n, 5), dtype=np.float32)
    x[:, :3] += 31.0
    x[:, 3] = x[:, 3] * 2.0 - 0.5
    return x


def batches(torch, n=2048, poison_row=17):
    """A, P, B: three batches of inputs and targets; P is a clean batch with ONE ray's target set to NaN"""
    out = []
    for k, name in enumerate("APB"):
        x = torch.from_numpy(queries(n, seed=100 + k)).cuda()
        t = np.random.default_rng(200 + k).random((n, 3), dtype=np.float32)
        if name == "P":
            t[poison_row, 1] = np.nan
        out.append((x, torch.from_numpy(t).cuda()))
    return out


def state(c):
    return [c.GetParams(k) for k in range(4)]


def assert_same_bits(p, q, what=""):
    for name, a, b in zip(SETS, p, q):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, name, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


def step(c, xb):
    c.Backward(*xb)
    c.OptimizerStep()


def test_policy_off_keeps_todays_behaviour(api, torch_gpu):
    """1. default policy: the poisoned batch's non-finite gradient reaches the master weights (what the guard is for)"""
    c = api.NeuralRadianceCache(api.AppConfig())
    A, P, B = batches(torch_gpu)
    step(c, A)
    assert np.isfinite(c.GetParams(c.MASTER)).all()
    step(c, P)
    assert not np.isfinite(c.GetParams(c.MASTER)).all()
    step(c, B)
    assert not np.isfinite(c.GetParams(c.MASTER)).all()
    if hasattr(c.L, "nrc_cache_get_nonfinite_policy"):      # (the test also runs against a library without the guard)
        assert c.GetNonFinitePolicy() == api.NRC_NONFINITE_PROPAGATE and c.GetSkippedSteps() == (0, 0)
    c.Destroy()


# which optimizer kernels a case runs (csrc/nrc_mlp.hip, Mlp::optimizer_step with the guard on):
#   fused     k_opt_pack<sgd, GuardArgs>; HashGrid: + k_grid_opt2<sgd, FROM16 = true, GuardArgs> (the table gradient from the packed fp16 table,
#             whose entries a bad step must still clear); the verdict from k_reduce_grads<GuardArgs>
#   unfused   NRC_DEBUG=no_fused_opt: k_adam_ema<GuardArgs> / k_sgd_ema<GuardArgs> + the repack launches
#   vector    the caller holds nrc_cache_grad_ptr (GradTensor()), so the optimizer reads the fp32 vector: HashGrid: k_grid_opt2<sgd, FROM16 = false,
#             GuardArgs>; the verdict from k_guard_scan, the launch of its own
# (k_grid_opt2 is the table's only optimizer kernel: an odd number of entries or a matrix block that is no multiple of four parameters is
# refused by Mlp's constructor, and no model it accepts has either)
@pytest.mark.parametrize("path", ["fused", "unfused", "vector"])
@pytest.mark.parametrize("optimizer", ["Adam", "SGD"])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_a_skipped_step_is_the_identity_exactly(api, torch_gpu, monkeypatch, model, optimizer, path):
    """2. run X: SKIP, batches A, P, B.  Run Y: a fresh cache, A, SetStep(GetStep() + 1), B.  All four parameter sets and the step number
    are bit-identical, and X reports one skipped step, the second."""
    kw = dict(MODELS[model], optimizer=optimizer)
    A, P, B = batches(torch_gpu)
    nrc_debug(monkeypatch, no_fused_opt=True) if path == "unfused" else nrc_debug(monkeypatch)
    X, Y = api.NeuralRadianceCache(api.AppConfig(**kw)), api.NeuralRadianceCache(api.AppConfig(**kw))
    nrc_debug(monkeypatch)
    if path == "vector":
        X.GradTensor()
        Y.GradTensor()
    X.SetNonFinitePolicy(api.NRC_NONFINITE_SKIP)
    assert X.GetNonFinitePolicy() == api.NRC_NONFINITE_SKIP
    step(X, A)
    before = state(X)
    step(X, P)
    assert not np.isfinite(X.GetLoss())                      # the skipped step's loss is still published
    assert_same_bits(state(X), before, "across the skipped step")
    assert X.GetSkippedSteps() == (1, 2)
    step(X, B)
    step(Y, A)
    Y.SetStep(Y.GetStep() + 1)
    step(Y, B)
    assert_same_bits(state(X), state(Y), "X vs Y")
    assert X.GetStep() == Y.GetStep() == 3
    assert X.GetSkippedSteps() == (1, 2)
    assert all(np.isfinite(s).all() for s in state(X))
    assert not np.array_equal(state(X)[0], before[0])        # B's step was taken
    X.Destroy()
    Y.Destroy()


@pytest.mark.parametrize("model", sorted(MODELS))
def test_good_steps_are_untouched(api, torch_gpu, model):
    """3. twenty clean steps with SKIP and with PROPAGATE: the same parameters and losses, bit for bit; nothing skipped"""
    a, b = api.NeuralRadianceCache(api.AppConfig(**MODELS[model])), api.NeuralRadianceCache(api.AppConfig(**MODELS[model]))
    a.SetNonFinitePolicy(api.NRC_NONFINITE_SKIP)
    n = 2048
    losses = [[], []]
    for k in range(20):
        x = torch_gpu.from_numpy(queries(n, seed=300 + k)).cuda()
        t = torch_gpu.from_numpy(np.random.default_rng(400 + k).random((n, 3), dtype=np.float32)).cuda()
        for i, c in enumerate((a, b)):
            step(c, (x, t))
            losses[i].append(c.GetLoss())
    assert_same_bits(state(a), state(b))
    assert np.array_equal(np.asarray(losses[0], np.float32).view(np.uint32), np.asarray(losses[1], np.float32).view(np.uint32))
    assert np.isfinite(losses[0]).all() and a.GetSkippedSteps() == (0, 0)
    a.Destroy()
    b.Destroy()


@pytest.mark.parametrize("model", sorted(MODELS))
def test_the_next_inference_uses_the_kept_weights(api, torch_gpu, model):
    """4. the host flips to the other inference set whatever the verdict: after a skipped step both inference paths return what they
    returned before it (a guard that does not repack that set returns the weights of two steps ago, one that repacks garbage NaN)"""
    c = api.NeuralRadianceCache(api.AppConfig(**MODELS[model]))
    c.SetNonFinitePolicy(api.NRC_NONFINITE_SKIP)
    A, P, B = batches(torch_gpu)
    step(c, A)
    step(c, B)
    q = torch_gpu.from_numpy(queries(4096, seed=9)).cuda()

    def infer():
        o = [torch_gpu.empty((4096, 3), device="cuda") for _ in range(2)]
        c.Infer(q, o[0], True)
        c.Infer(q, o[1], False)
        return [t.cpu().numpy() for t in o]

    before = infer()
    step(c, P)
    after = infer()
    assert c.GetSkippedSteps() == (1, 3)
    for name, p, r in zip(("useEma=True", "useEma=False"), before, after):
        assert np.isfinite(p).all() and np.array_equal(p.view(np.uint32), r.view(np.uint32)), name
    step(c, P)                                                # and once more, onto the other set
    for name, p, r in zip(("useEma=True", "useEma=False"), before, infer()):
        assert np.array_equal(p.view(np.uint32), r.view(np.uint32)), name
    assert c.GetSkippedSteps() == (2, 4)
    c.Destroy()


@pytest.mark.parametrize("policy", ["skip", "propagate"])
def test_fp16_exchange_overflow_with_a_finite_fp32_gradient(api, torch_gpu, policy):
    """5. fp16 exchange through an identity hook, L2 loss, targets of 1e5: the fp32 gradient (x loss_scale 128) is finite with
    max |g| > 65 504 and the loss is finite, so only rule 2 -- a non-finite word in the gradient the optimizer reads, here the fp16
    rounding's inf -- can fire.  SKIP: step skipped, parameters unchanged bitwise.  PROPAGATE: parameters non-finite."""
    cfg = api.AppConfig(loss_fn="L2", train_batch_count=1, log2_train_batch_size=10)
    c = api.NeuralRadianceCache(cfg)
    n = 1024
    x = torch_gpu.from_numpy(queries(n, seed=5)).cuda()
    t = torch_gpu.full((n, 3), 1.0e5, device="cuda")
    qi, qo = torch_gpu.zeros((16, 5), device="cuda"), torch_gpu.zeros((16, 3), device="cuda")
    c.Init(16, qi, qo, x, t)
    # the precondition, on the fp32 gradient as backward leaves it
    c.Backward(x, t)
    g32 = c.GetParams(c.GRAD)
    assert np.isfinite(g32).all() and np.abs(g32).max() > 65504.0, np.abs(g32).max()
    seen = []
    c.SetGradHook(lambda g, loss: seen.append((g.clone(), loss.clone())))
    c.SetExchangeDtype("f16")
    if policy == "skip":
        c.SetNonFinitePolicy(api.NRC_NONFINITE_SKIP)
    before = state(c)
    c.InferAndTrain(None, True)
    loss = c.GetLoss()
    g_hook, loss_hook = seen[0][0].cpu().numpy(), seen[0][1].cpu().numpy()
    assert np.isfinite(loss) and np.isfinite(loss_hook[0])
    assert np.isinf(g_hook).any() and not np.isnan(g_hook).any()      # what the hook is handed: the fp16-rounded values
    if policy == "skip":
        assert c.GetSkippedSteps() == (1, 1)
        assert_same_bits(state(c), before)
    else:
        assert not np.isfinite(c.GetParams(c.MASTER)).all()
    c.SetGradHook(None)
    c.Destroy()


def test_hashgrid_table_is_kept_and_left_clean(api, torch_gpu):
    """6. a poisoned target on a HashGrid model is caught by rule 1 (the loss); table weights and table moments stay as they were, and the
    following clean step equals the same step of a cache that never saw the poisoned batch -- a table-gradient buffer left dirty would
    add the poisoned batch's entries to it"""
    kw = dict(pos_id=0, hashgrid_log2_size=12, nn_depth=3)
    X, Y = api.NeuralRadianceCache(api.AppConfig(**kw)), api.NeuralRadianceCache(api.AppConfig(**kw))
    X.SetNonFinitePolicy(api.NRC_NONFINITE_SKIP)
    A, P, B = batches(torch_gpu)
    step(X, A)
    step(Y, A)
    before = state(X)
    assert (before[2][-8192:] != 0.0).any()                   # (the table is the tail of every vector) A touched entries: their moments moved
    step(X, P)
    assert not np.isfinite(X.GetLoss()) and X.GetSkippedSteps() == (1, 2)
    assert_same_bits(state(X), before)
    Y.SetStep(Y.GetStep() + 1)
    step(X, B)
    step(Y, B)
    assert_same_bits(state(X), state(Y))
    assert np.isfinite(state(X)[0]).all()
    X.Destroy()
    Y.Destroy()


def test_through_the_renderer(api, sc, torch_gpu, sphere_scene):
    """7. an NRC renderer (64^3 sphere, 128 x 80) with self_train = 1 and SKIP, frames rendered with train=True.  The construction the issue
    proposes -- a NaN in the EMA set, read by the tail inference -- does NOT poison the targets on the device: the specified target formula
    takes fmax(0, tail estimate), which drops a NaN, and min(8, .), which bounds an inf (tests/test_gpu_self_training.py, combine).  The
    poison used instead goes through the public surface too and through an input every training batch of the frame reads: one NaN in the
    MASTER set (SetParams(MASTER, ...), an output-layer weight), so every batch's prediction, loss and gradient are NaN.  While it is in
    place every training batch is skipped: all four sets keep their bits (under PROPAGATE the NaN would spread to every weight, the EMA
    set and both moments within one step) and the counter advances by the batches of those frames.  With the weight restored, steps are
    taken again."""
    cfg = api.AppConfig(train_batch_count=2, log2_train_batch_size=9, log2_infer_batch_size=14, self_train=1)
    nrc = api.NeuralRadianceCache(cfg)
    nrc.SetNonFinitePolicy(api.NRC_NONFINITE_SKIP)
    W, H = 128, 80
    ren = api.NrcHpmRenderer(W, H, False, sc.make_camera(aspect=W / H), cfg, sphere_scene, nrc)
    frs = sc.frame_randoms(12, seed=5)
    for f in range(3):
        ren.SetFrameRandom(frs[f])
        ren.Render(None, True)
    torch_gpu.cuda.synchronize()
    assert nrc.GetSkippedSteps() == (0, 0) and nrc.GetStep() == 6
    good = state(nrc)
    assert all(np.isfinite(s).all() for s in good)
    poisoned = good[0].copy()
    poisoned[-1] = np.nan
    nrc.SetParams(nrc.MASTER, poisoned)
    bad_frames = 3
    for f in range(3, 3 + bad_frames):
        ren.SetFrameRandom(frs[f])
        ren.Render(None, True)
        assert not np.isfinite(nrc.GetLoss())                  # the construction does poison the step on the device
    torch_gpu.cuda.synchronize()
    now = state(nrc)
    assert_same_bits(now, [poisoned] + good[1:], "across the skipped frames")
    assert nrc.GetSkippedSteps() == (bad_frames * 2, 6 + bad_frames * 2)
    nrc.SetParams(nrc.MASTER, good[0])
    for f in range(6, 9):
        ren.SetFrameRandom(frs[f])
        ren.Render(None, True)
    torch_gpu.cuda.synchronize()
    assert nrc.GetSkippedSteps()[0] == bad_frames * 2          # the counter stands still ...
    later = state(nrc)
    assert nrc.GetStep() == 18 and np.isfinite(nrc.GetLoss())
    assert all(not np.array_equal(later[k], good[k]) for k in range(4)) and all(np.isfinite(s).all() for s in later)      # ... and the weights move
    ren.Destroy()
    nrc.Destroy()


def test_two_ranks_reach_the_same_verdict(api, torch_gpu, tmp_path):
    """8. two processes on one GPU, gloo hook transport, fp16 exchange; only rank 1's second batch overflows fp16.  Both ranks skip that
    step -- the verdict is taken from the summed bits both hold -- and stay bit-identical replicas."""
    out = str(tmp_path / "guard")
    port = 29900 + (os.getpid() % 300)
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "tests", "workers", "nonfinite_guard_worker.py"), out],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    a, b = (np.load(out + ".%d.npz" % k) for k in range(2))
    assert int(a["rank"]) == 0 and int(b["rank"]) == 1
    # the precondition: rank 0's own gradient of the bad step fits fp16, rank 1's does not, and both are finite in fp32
    assert np.isfinite(a["g_local_bad"]).all() and np.abs(a["g_local_bad"]).max() < 65504.0
    assert np.isfinite(b["g_local_bad"]).all() and np.abs(b["g_local_bad"]).max() > 65504.0
    assert tuple(a["skipped"]) == tuple(b["skipped"]) == (1, 2)
    assert int(a["step"]) == int(b["step"]) == 3
    for key in SETS:
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key
        assert np.isfinite(a[key]).all(), key
        assert np.array_equal(a[key + "_after_bad"].view(np.uint32), a[key + "_before_bad"].view(np.uint32)), key
    assert not np.array_equal(a["w"], a["w_before_bad"])      # the third step was taken
