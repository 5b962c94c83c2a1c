"""The generic and HashGrid MLP kernels (csrc/nrc_mlp.hip: k_train_gen, k_train_gen2, k_infer_gen and the table kernels around them)
beyond one round of workgroups and at batch tails.  They are persistent kernels: the host caps the grid at a multiple of the CU count, a
workgroup loops over its groups of tiles, streams the weight stages through two alternating LDS buffers (k_train_gen, k_infer_gen: the
buffer of a stage is the parity of a counter that runs on ACROSS rounds) or through registers one stage ahead (k_train_gen2), and
prefetches the next round's stage 0 while a round finishes.  Every batch size here is derived from the CU count C of the device by the
host's own launch rule (repeated in launch_gen / launch_gen2 / infer_pass below and asserted, so a changed rule fails here instead of
silently testing one round again); the figures in the docstrings are for the 256 CUs of an MI355X.  All models have depth 2.
References: the other kernel family (bit for bit), the same kernels on batches that fit one round (sum of parts), the CPU oracle."""
import numpy as np
import pytest

from conftest import nrc_debug
from test_gpu_mlp import c_mlp_params, queries, randomize, rel

pytestmark = pytest.mark.gpu

N_MAX = 300000
DEPTH = 2
LOSS_SCALE = 128.0

# (posID, dirID, width, hashgrid_log2_size): Identity, Frequency + OneBlob, TriangleWave, HashGrid 2^16 (levels 2..15 have bin lists),
# HashGrid 2^11 (no level has eight bins: every (entry, value) pair goes through the fixed-point shadow)
MODELS_UP_TO_64 = [(1, 1, 32, 0), (3, 0, 64, 0), (2, 2, 64, 0), (0, 0, 64, 16), (0, 2, 32, 11)]
MODELS_128 = [(3, 0, 128, 0), (1, 1, 128, 0)]


def model_id(m):
    return "pos%d-dir%d-w%d" % m[:3] + ("-hash%d" % m[3] if m[0] == 0 else "")


def cu_count(torch):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def ceil_div(a, b):
    return -(-a // b)


def launch_gen(n_tiles, C):
    """Mlp::backward, k_train_gen<W, WAVES>: eight waves (one tile each) when n_tiles > 8 C, else four; grid = ceil(n_tiles / waves)
    workgroups, capped at 2 C -> (waves, groups of tiles, grid)"""
    waves = 8 if n_tiles > 8 * C else 4
    groups = ceil_div(n_tiles, waves)
    return waves, groups, min(groups, 2 * C)


def launch_gen2(n_tiles, C, width):
    """Mlp::backward, k_train_gen2<W, NT>: sgn = 4 / (W / 32) sample groups per workgroup, nt = 2 tiles per sample group when
    n_tiles > 4 sgn C, else 1; grid = ceil(n_tiles / (sgn nt)) workgroups, capped at 2 C -> (sgn, nt, groups, grid)"""
    sgn = 4 // (width // 32)
    nt = 2 if n_tiles > 4 * sgn * C else 1
    groups = ceil_div(n_tiles, sgn * nt)
    return sgn, nt, groups, min(groups, 2 * C)


def infer_pass(width, C):
    """Mlp::infer, generic branch, k_infer_gen: a workgroup pass is 256 queries at every width (4 waves x 2 tiles up to 64 neurons,
    8 waves x 1 tile for 128); grid = ceil(n / 256) capped at 4 C (up to 64 neurons) or 2 C (128) -> queries of the first pass"""
    return (4 if width <= 64 else 2) * C * 256


def train_tiles(case, C, width):
    """32-ray tiles of a training case, with the round structure it must reach under the rules above"""
    if case == "A":        # k_train_gen<W,8>: one round, the last workgroup with five of its eight waves
        n_tiles = 8 * C + 8 + 5
        waves, groups, grid = launch_gen(n_tiles, C)
        assert waves == 8 and groups == grid and n_tiles % 8 == 5
    elif case == "B":      # k_train_gen<W,8>: a second round of four groups, the last one with three of eight waves
        n_tiles = 16 * C + 24 + 3
        waves, groups, grid = launch_gen(n_tiles, C)
        assert waves == 8 and grid == 2 * C and groups - grid == 4 and n_tiles % 8 == 3
    elif case == "C":      # k_train_gen2<128,1>: a second round of three groups
        n_tiles = 2 * C + 3
        sgn, nt, groups, grid = launch_gen2(n_tiles, C, 128)
        assert width == 128 and (sgn, nt) == (1, 1) and grid == 2 * C and groups - grid == 3
    elif case == "D":      # k_train_gen2<128,2>, nt = 2 chosen by the host: a second round of three groups, the last with one tile of two
        n_tiles = 4 * C + 5
        sgn, nt, groups, grid = launch_gen2(n_tiles, C, 128)
        assert width == 128 and (sgn, nt) == (1, 2) and grid == 2 * C and groups - grid == 3 and n_tiles % 2 == 1
    else:                  # "X1" / "X2": k_train_gen2<W,nt> (NRC_DEBUG=train_gen_old=0) for W <= 64: a second round begins at
        want_nt = int(case[1])      # n_tiles > 2 C sgn nt; one full group and one group with a single tile in it
        sgn = 4 // (width // 32)
        n_tiles = 2 * C * sgn * want_nt + sgn * want_nt + 1
        sgn, nt, groups, grid = launch_gen2(n_tiles, C, width)
        assert nt == want_nt and grid == 2 * C and groups - grid == 2 and n_tiles % (sgn * nt) == 1
    assert n_tiles * 32 < N_MAX
    return n_tiles


def make_pair(api, orc, model, seed=3):
    pos_id, dir_id, width, hg = model
    c = api.NeuralRadianceCache(api.AppConfig(pos_id=pos_id, dir_id=dir_id, nn_width=width, nn_depth=DEPTH, hashgrid_log2_size=hg))
    onn = orc.nn_create(pos_id=pos_id, dir_id=dir_id, width=width, depth=DEPTH, hashgrid_log2_size=hg)
    assert c.ParamCount() == onn.n_params
    randomize(c, onn, seed=seed, scale=1.0)
    assert onn.n_mlp == c_mlp_params(width, DEPTH, (onn.enc_dims + 15) // 16 * 16)      # the matrices first, a trainable table behind them
    return c, onn


def same_weights(api, model, onn):
    """another cache of the model with the weights `randomize` left in the oracle"""
    pos_id, dir_id, width, hg = model
    c = api.NeuralRadianceCache(api.AppConfig(pos_id=pos_id, dir_id=dir_id, nn_width=width, nn_depth=DEPTH, hashgrid_log2_size=hg))
    c.SetParams(0, np.array(onn.buffer(0)))
    c.SetParams(1, np.array(onn.buffer(1)))
    return c


def model_queries(model, n, seed, nan_frac):
    x = queries(n, seed=seed, nan_frac=nan_frac)
    if model[0] in (0, 1):
        x[:, :3] -= 31.0                                     # keep Identity / HashGrid positions in [0, 1)
    return x


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def table_sum_bound(whole, abs_parts, k_parts):
    """see check_sum_of_parts"""
    return 2.0 ** -11 * (1.0 + 2.0 ** -10) * (np.abs(whole) + abs_parts) + (k_parts + 1) * 2.0 ** -25


def check_sum_of_parts(c, d_x, d_t, parts, n_mlp, tag):
    """The gradient and loss of batch (d_x, d_t) against the float64 sum of the gradients and losses of its consecutive `parts`
    (row counts), computed on the same cache against the same normaliser n.  Per-ray arithmetic is the same in every launch.
    MLP part: only the fp32 sums over rays are cut at other places (k_wgrad / k_wgrad2 chunks, k_reduce_grads) -> rel-L2 < 1e-5, the loss
    within 1e-5 relative (the bounds of test_backward_of_a_batch_longer_than_one_round_of_workgroups for the fused kernel).
    Table part (values as GetParams(4) holds them: fp16 numbers, loss scale included): a ray sends the same fp16 pairs to the same
    entries in whichever launch it runs, a launch adds an entry's pairs EXACTLY (64-bit fixed point: k_grid_scatter / k_grid_gather) and
    rounds the sum to fp16 once.  With S_k the exact sum of part k and S = sum_k S_k the whole batch's: whole = rn(S), part_k = rn(S_k),
    |rn(v) - v| <= 2^-11 |v| for a normal result and <= 2^-25 for a subnormal one (spacing 2^-24), and |v| <= (1 + 2^-10) |rn(v)|
    for a normal one (1 / (1 - 2^-11) < 1 + 2^-10).  So
        |whole - sum_k part_k| <= |rn(S) - S| + sum_k |rn(S_k) - S_k| <= 2^-11 (1 + 2^-10) (|whole| + sum_k |part_k|) + (K + 1) 2^-25
    for every entry (float64 adds the K fp16 numbers without rounding).  A second pass over the whole batch repeats every bit.
    Returns (whole gradient, loss, figures)."""
    n = d_x.shape[0]
    assert sum(parts) == n and all(p % 32 == 0 for p in parts)
    c.Backward(d_x, d_t)
    whole, loss_whole = c.GetParams(4), c.GetLoss()
    c.Backward(d_x, d_t)
    assert np.array_equal(bits(whole), bits(c.GetParams(4))) and c.GetLoss() == loss_whole, tag
    assert np.isfinite(whole).all() and np.abs(whole[:n_mlp]).max() > 0.0, tag
    total, total_abs, loss, a = np.zeros(whole.size, np.float64), np.zeros(whole.size, np.float64), 0.0, 0
    for p in parts:
        c.Backward(d_x[a:a + p].contiguous(), d_t[a:a + p].contiguous(), nNorm=n)
        g = c.GetParams(4).astype(np.float64)
        total += g
        total_abs += np.abs(g)
        loss += c.GetLoss()
        a += p
    fig = dict(parts_mlp=rel(total[:n_mlp], whole[:n_mlp].astype(np.float64)), parts_loss=abs(loss - loss_whole) / abs(loss_whole))
    tab_excess = None
    if whole.size > n_mlp:
        tab = whole[n_mlp:].astype(np.float64)
        assert np.abs(tab).max() > 0.0, tag
        err = np.abs(tab - total[n_mlp:])
        bound = table_sum_bound(tab, total_abs[n_mlp:], len(parts))
        tab_excess = float((err / bound).max())
        fig["parts_table_max_err_over_bound"] = tab_excess
        fig["parts_table_rel"] = rel(total[n_mlp:], tab)
    print("ROUNDS %s sum-of-parts %s" % (tag, fig))
    assert fig["parts_mlp"] < 1e-5, (tag, fig)
    assert fig["parts_loss"] < 1e-5, (tag, fig)
    if tab_excess is not None:
        assert tab_excess <= 1.0, (tag, fig)
    return whole, loss_whole, fig


def check_oracle_backward(onn, x, t, whole, loss_whole, tag):
    """bounds of test_generic_models_match_oracle / test_hashgrid_model_matches_oracle"""
    loss_ref = onn.backward(x, t)
    g, g_ref = whole.astype(np.float64) / LOSS_SCALE, np.array(onn.buffer(4), np.float64)
    nm = onn.n_mlp
    fig = dict(oracle_loss=abs(loss_whole - loss_ref) / abs(loss_ref), oracle_mlp=rel(g[:nm], g_ref[:nm]))
    if g.size > nm:
        fig["oracle_table"] = rel(g[nm:], g_ref[nm:])
    print("ROUNDS %s oracle %s" % (tag, fig))
    assert fig["oracle_loss"] < 3e-3, (tag, fig)
    assert fig["oracle_mlp"] < 2e-2, (tag, fig)
    assert fig.get("oracle_table", 0.0) < 3e-2, (tag, fig)


def run_training_case(api, orc, torch, monkeypatch, model, case, default_mode, other_mode, oracle=True):
    C = cu_count(torch)
    n = 32 * train_tiles(case, C, model[2])
    tag = "%s %s n=%d" % (case, model_id(model), n)
    x = model_queries(model, n, seed=11 + model[0] * 7 + model[1], nan_frac=0.0)
    t = (np.random.default_rng(22).random((n, 3), dtype=np.float32) * 2).astype(np.float32)
    d_x, d_t = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    nrc_debug(monkeypatch, **default_mode)
    c, onn = make_pair(api, orc, model)
    nm = onn.n_mlp
    whole, loss_whole, _ = check_sum_of_parts(c, d_x, d_t, [min(8192, n - a) for a in range(0, n, 8192)], nm, tag)
    c.Destroy()
    # the other kernel family: every output element is the same sequence of MFMAs (test_training_kernels_agree, beyond a round)
    nrc_debug(monkeypatch, **other_mode)
    c2 = same_weights(api, model, onn)
    c2.Backward(d_x, d_t)
    other, loss_other = c2.GetParams(4), c2.GetLoss()
    c2.Destroy()
    nrc_debug(monkeypatch)
    differ = int((bits(other[:nm]) != bits(whole[:nm])).sum())
    print("ROUNDS %s kernel-agreement: %d of %d MLP gradient words differ, loss %r / %r" % (tag, differ, nm, loss_whole, loss_other))
    assert differ == 0 and loss_other == loss_whole, (tag, differ, loss_whole, loss_other)
    if oracle:
        check_oracle_backward(onn, x, t, whole, loss_whole, tag)


def other_family(width):
    """k_train_gen is the default up to 64 neurons, k_train_gen2 for 128 (Mlp::backward): NRC_DEBUG=train_gen_old picks the other one"""
    return dict(train_gen_old=0 if width <= 64 else 1)


@pytest.mark.parametrize("model", MODELS_UP_TO_64, ids=model_id)
@pytest.mark.parametrize("case", ["A", "B"])
def test_training_with_eight_waves_per_workgroup(api, orc, torch_gpu, monkeypatch, model, case):
    """k_train_gen<W,8>, which the host takes beyond 8 C tiles (65 536 rays) and no other test launches.
    A: 8 C + 13 tiles = 65 952 rays: 258 workgroups, one round, the last workgroup with five of its eight waves at work.
    B: 16 C + 27 tiles = 131 936 rays: 516 groups on 512 workgroups -- workgroups 0..3 run a second group, into whose buffer the end
       of the first one prefetched stage 0 (five stages per group, six with a trainable table: the stage parity of a group differs
       from round to round for the plain models and not for the HashGrid ones); the last group has three of eight waves.
    Compared bit for bit with k_train_gen2 on the same batch, which is past ITS first round of 512 workgroups at both sizes
    (W = 32: A nt = 1, 516 groups, B nt = 2, 516 groups; W = 64: A nt = 2, 516 groups, B nt = 2, 1 031 groups), with the sum of
    8 192-ray parts (every part one round of k_train_gen<W,4>) and with the oracle.
    Measured on an MI355X; no MLP gradient word and no loss bit differed between the two kernels in any case.
    sum of parts: MLP rel-L2 (bound 1e-5), loss (1e-5), largest table error / its bound (1) | oracle: loss (3e-3), MLP (2e-2), table (3e-2)
      A 1/1/32        1.0e-7  1.8e-8  -     | 1.6e-7  2.1e-7  -
      A 3/0/64        8.5e-8  9.2e-9  -     | 7.4e-8  2.1e-6  -
      A 2/2/64        9.3e-8  4.3e-8  -     | 0       2.4e-7  -
      A 0/0/64 2^16   9.3e-8  3.1e-8  0.78  | 0       1.8e-7  2.5e-4
      A 0/2/32 2^11   1.1e-7  5.5e-8  0.73  | 0       1.7e-7  2.2e-4
      B 1/1/32        1.4e-7  9.8e-9  -     | 7.9e-8  1.8e-7  -
      B 3/0/64        1.3e-7  1.5e-8  -     | 7.4e-8  1.9e-6  -
      B 2/2/64        1.2e-7  5.3e-8  -     | 2.7e-7  2.6e-7  -
      B 0/0/64 2^16   1.2e-7  4.5e-8  0.59  | 0       1.1e-6  2.9e-4
      B 0/2/32 2^11   1.1e-7  3.5e-8  0.64  | 0       1.3e-7  2.2e-4"""
    run_training_case(api, orc, torch_gpu, monkeypatch, model, case, dict(), other_family(model[2]))


def test_training_with_eight_waves_per_workgroup_128_wide(api, orc, torch_gpu, monkeypatch):
    """k_train_gen<128,8> (NRC_DEBUG=train_gen_old=1; the 128-wide default is k_train_gen2) at case B, 131 936 rays: a second round
    of four groups, the last with three of eight waves; 32 KB weight stages, the largest the kernel streams.  Against
    k_train_gen2<128,2> (2 062 groups on 512 workgroups: five rounds) bit for bit and against the sum of its 8 192-ray parts; no
    oracle pass here (6 s for this width at this size) -- cases C and D anchor the 128-wide kernels to it.
    Measured on an MI355X: sum of parts MLP rel-L2 6.3e-8 (bound 1e-5), loss 2.7e-8 (1e-5); none of the 27 008 gradient words and no
    loss bit differs from k_train_gen2's"""
    run_training_case(api, orc, torch_gpu, monkeypatch, (3, 0, 128, 0), "B", dict(train_gen_old=1), dict(train_gen_old=0), oracle=False)


@pytest.mark.parametrize("model", MODELS_128, ids=model_id)
@pytest.mark.parametrize("case", ["C", "D"])
def test_training_128_wide_beyond_one_round(api, orc, torch_gpu, monkeypatch, model, case):
    """k_train_gen2<128,NT>, the default of the 128-wide models, one sample group per workgroup.
    C: 2 C + 3 tiles = 16 480 rays, one tile above the largest batch of the other tests: nt = 1, 515 groups on 512 workgroups --
       workgroups 0..2 run a second group with the stage-0 fragments they loaded during the last stage of the first.
    D: 4 C + 5 tiles = 32 928 rays: the host picks nt = 2 by itself (n_tiles > 4 C), 515 groups, the last one with one tile of two.
    Against k_train_gen<128,4> (129 / 258 groups: one round) bit for bit, the sum of 8 192-ray parts and the oracle.
    Measured on an MI355X; no MLP gradient word and no loss bit differed between the two kernels in any case.
    sum of parts: MLP rel-L2 (bound 1e-5), loss (1e-5) | oracle: loss (3e-3), MLP gradient (2e-2)
      C 3/0/128   7.4e-8  9.7e-8 | 3.4e-7  1.8e-6
      C 1/1/128   6.8e-8  5.2e-8 | 6.1e-8  2.0e-7
      D 3/0/128   6.5e-8  3.0e-8 | 1.4e-7  6.6e-6
      D 1/1/128   6.5e-8  1.9e-8 | 6.1e-8  1.9e-7"""
    run_training_case(api, orc, torch_gpu, monkeypatch, model, case, dict(), other_family(128))


@pytest.mark.parametrize("model,case", [((1, 1, 32, 0), "X1"), ((1, 1, 32, 0), "X2"), ((3, 0, 64, 0), "X1"), ((3, 0, 64, 0), "X2"),
                                        ((0, 0, 64, 16), "X1")],
                         ids=lambda v: model_id(v) if isinstance(v, tuple) else v)
def test_training_rows_split_over_waves_beyond_one_round_up_to_64_neurons(api, orc, torch_gpu, monkeypatch, model, case):
    """k_train_gen2<32,NT> / <64,NT> (NRC_DEBUG=train_gen_old=0; sgn = 4 / 2 sample groups per workgroup) in a second round of two
    groups, the last one holding a single tile: n_tiles = 2 C sgn nt + sgn nt + 1.
    W = 32: X1 2 053 tiles = 65 696 rays (nt = 1), X2 4 105 tiles = 131 360 rays (nt = 2, the host's choice beyond 4 sgn C tiles).
    W = 64: X1 1 027 tiles = 32 864 rays, X2 2 053 tiles = 65 696 rays; the HashGrid model adds the sixth stage (W0^T delta_0).
    Against k_train_gen (four waves up to 8 C tiles: one round; eight beyond: 4 105 tiles are two rounds) bit for bit, the sum of
    8 192-ray parts and the oracle.
    Measured on an MI355X; no MLP gradient word and no loss bit differed between the two kernels in any case.
    sum of parts: MLP rel-L2 (bound 1e-5), loss (1e-5), largest table error / its bound (1) | oracle: loss (3e-3), MLP (2e-2), table (3e-2)
      X1 1/1/32        9.2e-8  8.3e-8  -     | 7.9e-8  1.8e-7  -
      X2 1/1/32        1.2e-7  3.2e-8  -     | 0       1.5e-7  -
      X1 3/0/64        6.9e-8  5.5e-8  -     | 3.7e-7  1.9e-6  -
      X2 3/0/64        8.7e-8  4.1e-8  -     | 0       2.1e-6  -
      X1 0/0/64 2^16   7.7e-8  1.8e-8  0.86  | 1.7e-7  3.0e-7  2.6e-4"""
    run_training_case(api, orc, torch_gpu, monkeypatch, model, case, dict(train_gen_old=0), dict(train_gen_old=1))


@pytest.mark.parametrize("model", MODELS_UP_TO_64 + MODELS_128, ids=model_id)
def test_small_and_ragged_training_batches_sum_to_the_batch(api, orc, torch_gpu, model):
    """A 1 024-ray batch and its parts of 32, 96, 160, 224 and 512 rays against the normaliser 1 024: single workgroups that are half
    empty (k_train_gen: 1, 3, 5, 7 tiles on four-wave workgroups; k_train_gen2<128,1>: one tile each), k_encode_hash with n % 128 != 0
    (ceil(n / 128) * 8 workgroups on an 8-XCD part) and k_grid_scatter with n % 256 != 0 (ceil(n / 256) per level).  The parts sum to
    the whole within the bounds of check_sum_of_parts -- no single ReLU tie decides that, as it could decide a 32-ray comparison with
    the oracle --, and the whole batch is the oracle's (loss 3e-3, MLP gradient 2e-2, table gradient 3e-2).
    Measured on an MI355X over the seven models: sum of parts MLP rel-L2 4.2e-8 .. 5.1e-8, loss <= 8.8e-8, largest table error / its bound
    0.85 (2^16) and 0.92 (2^11); oracle loss <= 4.0e-6, MLP gradient <= 8.6e-6, table gradient 2.3e-4 and 2.5e-4"""
    n = 1024
    tag = "ragged %s" % model_id(model)
    c, onn = make_pair(api, orc, model)
    x = model_queries(model, n, seed=13 + model[0] * 7 + model[1], nan_frac=0.0)
    t = (np.random.default_rng(23).random((n, 3), dtype=np.float32) * 2).astype(np.float32)
    whole, loss_whole, _ = check_sum_of_parts(c, torch_gpu.from_numpy(x).cuda(), torch_gpu.from_numpy(t).cuda(), [32, 96, 160, 224, 512],
                                              onn.n_mlp, tag)
    c.Destroy()
    check_oracle_backward(onn, x, t, whole, loss_whole, tag)


# one model per k_infer_gen template: pos 3 / dir 0 runs <W, ., false, ., ENC80 = true> with the EMA weights (encoding inside the kernel)
# and k_encode + <W, ., false> with the master weights; other plain encodings k_encode + <W, ., false>; HashGrid k_encode_hash_lm + <W, ., true>
INFER_MODELS = [(3, 0, 32, 0), (3, 0, 64, 0), (3, 0, 128, 0), (2, 1, 32, 0), (1, 2, 64, 0), (0, 0, 64, 12), (0, 1, 128, 12), (0, 2, 32, 12)]


def infer_queries(model, n, seed):
    return model_queries(model, n, seed=seed, nan_frac=0.1 if model[1] == 0 else 0.0)      # only OneBlob absorbs a NaN phi (quirk Q5)


def infer_guarded(c, torch, x, use_ema):
    """Infer into a tensor with eight guard rows behind the tail, which must come back untouched"""
    n = x.shape[0]
    d_out = torch.full((n + 8, 3), -7.0, device="cuda")
    c.Infer(torch.from_numpy(x).cuda(), d_out[:n], use_ema)
    out = d_out.cpu().numpy()
    assert (out[n:] == -7.0).all(), "rows behind the tail were written"
    return out[:n]


@pytest.mark.parametrize("use_ema", [True, False], ids=["ema", "master"])
@pytest.mark.parametrize("model", INFER_MODELS, ids=model_id)
def test_inference_in_its_second_pass(api, orc, torch_gpu, model, use_ema):
    """k_infer_gen beyond its first pass: 4 C x 256 + 549 = 262 693 queries up to 64 neurons (1 024 workgroups; workgroups 0..2 run a
    second group of 256 queries, the third one with a 37-query tail: five of its tiles idle, one ragged), 2 C x 256 + 549 = 131 621
    for 128 neurons (512 workgroups of eight waves).  A group is three stages at depth 2, so the second group reads its stage 0 from
    the OTHER buffer than the first, put there by the prefetch at the end of the first.  Three 1 024-query slices -- the start, the
    rows astride the end of pass one, the end with the ragged tile -- are bit-identical to Infer of the slice alone (results are per
    query) and within rel-L2 3e-3 of the oracle; eight guard rows behind the tail stay as they were.
    Measured on an MI355X: no row of any slice differs from the slice alone; largest of the three slices' rel-L2 to the oracle (bound
    3e-3), EMA / master weights:
      3/0/32  2.4e-5 / 1.2e-5    3/0/64  3.4e-5 / 1.1e-5    3/0/128  5.3e-5 / 2.2e-5    2/1/32  7.6e-6 / 9.6e-6    1/2/64  9.6e-6 / 1.4e-5
      HashGrid 2^12: 0/0/64  1.4e-5 / 1.3e-5    0/1/128  4.8e-6 / 1.1e-5    0/2/32  1.7e-5 / 2.6e-5"""
    C = cu_count(torch_gpu)
    p1 = infer_pass(model[2], C)
    n = p1 + 512 + 37
    assert p1 < n < N_MAX and ceil_div(n, 256) - p1 // 256 == 3
    c, onn = make_pair(api, orc, model)
    x = infer_queries(model, n, seed=17 + model[0] * 7 + model[1])
    out = infer_guarded(c, torch_gpu, x, use_ema)
    for a in (0, p1 - 512, n - 1024):
        xs = np.ascontiguousarray(x[a:a + 1024])
        alone = infer_guarded(c, torch_gpu, xs, use_ema)
        differ = int((bits(alone) != bits(out[a:a + 1024])).any(axis=1).sum())
        err = rel(out[a:a + 1024], onn.forward(xs, use_ema, 1))
        print("ROUNDS infer %s %s n=%d rows %d..: %d rows differ from the slice alone, oracle rel-L2 %.3g" % (
            model_id(model), "ema" if use_ema else "master", n, a, differ, err))
        assert np.isfinite(out[a:a + 1024]).all()
        assert differ == 0, (a, differ)
        assert err < 3e-3, (a, err)
    c.Destroy()


@pytest.mark.parametrize("use_ema", [True, False], ids=["ema", "master"])
@pytest.mark.parametrize("model", INFER_MODELS, ids=model_id)
def test_inference_tails_of_the_generic_kernels(api, orc, torch_gpu, model, use_ema):
    """test_inference_ragged_sizes for every k_infer_gen template and both weight sets: 1, 31, 32, 33, 255, 256 and 257 queries (a
    lone lane, a tile short of / exactly / one past full, a workgroup pass short of / exactly / one past full) with guard rows behind
    the tail; rel-L2 3e-3 to the oracle, and below a full tile -- where a norm over three numbers hides little -- also the absolute
    bound of test_inference_matches_oracle.  Measured on an MI355X: rel-L2 <= 7.0e-5 over all models, weight sets and sizes"""
    c, onn = make_pair(api, orc, model)
    for n in (1, 31, 32, 33, 255, 256, 257):
        x = infer_queries(model, n, seed=100 + n)
        got, ref = infer_guarded(c, torch_gpu, x, use_ema), onn.forward(x, use_ema, 1)
        err, err_abs = rel(got, ref), float(np.abs(got - ref).max())
        print("ROUNDS tails %s %s n=%d: rel-L2 %.3g, max abs %.3g (|ref| max %.3g)" % (model_id(model), "ema" if use_ema else "master", n, err,
                                                                                 err_abs, np.abs(ref).max()))
        assert np.isfinite(got).all(), n
        assert err < 3e-3, (n, err)
        if n < 32:
            assert err_abs < 2e-2 * max(1.0, float(np.abs(ref).max())), (n, err_abs)
    c.Destroy()
