"""The optimizer step against the build BEFORE the optimizer's host code and update rules were folded into one (csrc/nrc_mlp.hip,
Mlp::optimizer_step): the bitwise tests elsewhere compare two paths of one build and cannot see a change that moves both.

tests/golden/optimizer_step_bits.json holds, per case and per step, the sha256 of the four buffers GetParams(0..3) (weights, EMA weights,
Adam moments) and the GetSkippedSteps() pair, recorded from the library of the commit before that change:

    NRC_HPM_LIB=<that commit's libnrc_hpm.so> python tests/test_gpu_optimizer_bits.py tests/golden/optimizer_step_bits.json

(never from the code under test).  The optimizer is driven alone, so every case is reproducible run to run: a step is SetParams(4, g) with
a synthetic gradient vector (integer hashes of seed and index, no library's random stream) + OptimizerStep(), no Backward.  Of a table's
entries about three in four have an exactly zero gradient, re-drawn every step: k_grid_opt2's all-zero thread, its mixed thread and
"moments moved, gradient now zero" all occur.  Four steps; step 3's gradient holds one inf."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "optimizer_step_bits.json")

HASH_LOG2 = 10
MODELS = dict(m6x64=dict(), m2x16=dict(nn_width=16, nn_depth=2), hashgrid=dict(pos_id=0, hashgrid_log2_size=HASH_LOG2, nn_depth=2))
TABLE_PARAMS = 2 * 16 * (1 << HASH_LOG2)      # 16 levels, each capped at 2^HASH_LOG2 entries of two features
OPTIMIZERS = ("Adam", "SGD")
PATHS = ("default", "no_fused_opt")
POLICIES = ("PROPAGATE", "SKIP")
STEPS, BAD_STEP, BAD_INDEX = 4, 3, 7      # (the inf sits among the matrix gradients: the part every scan reads)
CASES = [(m, o, p, q) for m in sorted(MODELS) for o in OPTIMIZERS for p in PATHS for q in POLICIES]


def case_id(model, optimizer, path, policy):
    return "%s-%s-%s-%s" % (model, optimizer, path, policy)


def hash32(seed, n):
    """splitmix64 of (seed, index) -> uint32: the same words on every machine and under every numpy"""
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(32)).astype(np.uint32)


def gradient(n, n_table, step):
    """uniform multiples of 2^-20 in [-8, 8) (the vector carries the loss scale of 128); table part: zero on ~3 entries in 4"""
    g = ((hash32(2 * step, n) >> np.uint32(8)).astype(np.int64) - (1 << 23)).astype(np.float32) / np.float32(1 << 20)
    if n_table:
        keep = (hash32(2 * step + 1, n_table // 2) & np.uint32(3)) == 0
        g[n - n_table:] *= np.repeat(keep, 2)
    if step == BAD_STEP:
        g[BAD_INDEX] = np.inf
    return g


def drive(api, c, model, policy):
    """the four steps on cache c -> per step {"params": [sha256 x 4], "skipped": [n, last]}, and the state after BAD_STEP"""
    n = c.ParamCount()
    n_table = TABLE_PARAMS if "pos_id" in MODELS[model] else 0
    assert n > n_table + BAD_INDEX
    if policy == "SKIP":
        c.SetNonFinitePolicy(api.NRC_NONFINITE_SKIP)
    out, after_bad = [], None
    for step in range(1, STEPS + 1):
        c.SetParams(4, gradient(n, n_table, step))
        c.OptimizerStep()
        state = [c.GetParams(k) for k in range(4)]
        if step == BAD_STEP:
            after_bad = state
        out.append(dict(params=[hashlib.sha256(np.ascontiguousarray(s, "<f4").tobytes()).hexdigest() for s in state],
                        skipped=list(c.GetSkippedSteps())))
    return out, after_bad


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


@pytest.mark.gpu
@pytest.mark.parametrize("model,optimizer,path,policy", CASES, ids=[case_id(*c) for c in CASES])
def test_optimizer_step_bits_equal_the_recorded_build(api, torch_gpu, monkeypatch, recorded, model, optimizer, path, policy):
    from conftest import nrc_debug
    nrc_debug(monkeypatch, no_fused_opt=True) if path == "no_fused_opt" else nrc_debug(monkeypatch)
    c = api.NeuralRadianceCache(api.AppConfig(**dict(MODELS[model], optimizer=optimizer)))
    nrc_debug(monkeypatch)
    got, after_bad = drive(api, c, model, policy)
    c.Destroy()
    want = recorded[case_id(model, optimizer, path, policy)]
    for step, (g, w) in enumerate(zip(got, want), 1):
        print("step %d: %s %s" % (step, g["skipped"], " ".join(h[:12] for h in g["params"])))
        assert g == w, "step %d differs from the recorded build" % step
    assert len(got) == len(want) == STEPS
    if policy == "SKIP":
        assert tuple(got[-1]["skipped"]) == (1, BAD_STEP)
        assert all(np.isfinite(s).all() for s in after_bad)
    else:
        assert not all(np.isfinite(s).all() for s in after_bad)


def record(path):
    import torch
    sys.path.insert(0, ROOT)
    from nrc_hpm_renderer_amd import api
    assert os.environ.get("NRC_HPM_LIB"), "record from the library of the commit before the change: set NRC_HPM_LIB"
    torch.cuda.set_device(0)
    cases = {}
    for model, optimizer, p, policy in CASES:
        os.environ.pop("NRC_DEBUG", None)
        if p == "no_fused_opt":
            os.environ["NRC_DEBUG"] = "no_fused_opt"
        c = api.NeuralRadianceCache(api.AppConfig(**dict(MODELS[model], optimizer=optimizer)))
        os.environ.pop("NRC_DEBUG", None)
        cases[case_id(model, optimizer, p, policy)], _ = drive(api, c, model, policy)
        c.Destroy()
    with open(path, "w") as f:
        json.dump(dict(recorded_from=api.load_library().nrc_version().decode(), cases=cases), f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d cases from %s" % (len(cases), api.LIB_PATH))


if __name__ == "__main__":
    record(sys.argv[1])
