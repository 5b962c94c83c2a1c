"""Renderer-mode inference (csrc/nrc_mlp.hip: k_infer<6, ., 2, LISTED>, k_infer_gen with the frame's live-query list or with skip_in,
k_encode_hash_list; csrc/nrc_api.hip: Cache::infer_all) past one round of its persistent workgroups, per query.  Every frame of the product
and of the benchmark runs these launches, with other instantiations and other host rules than the dense mode of nrc_cache_infer that
test_gpu_mlp_rounds.py drives past a round; the only other per-query test of them, test_live_query_list_changes_no_pixel, renders 256x160
and stays inside one round of every kernel, one group per workgroup and one stride of the list encoder.

Reference.  Results are per query, so the radiance of EVERY live pixel of a frame is compared bit for bit (uint32; a NaN on both sides
counts as equal: about 15 % of the live queries carry the NaN angle of quirk Q5, which only the OneBlob direction encoding absorbs) with
the dense kernel's output for the same 5-float query: cache.Infer(q_live, out, useEma=True) on a SECOND cache of the same model that was
given the same vectors 0 and 1.  Dense mode past one round is pinned to the oracle by test_gpu_mlp_rounds.py; as an independent anchor,
2 048 live queries drawn with a seeded generator from all over the frame are compared with the oracle's forward pass at the tolerances
the existing tests use (rel-L2 2e-3 fused, 3e-3 generic, 3e-2 HashGrid at positions near 31: test_hashgrid_model_matches_oracle's quirk-Q3
block).  For the direction encodings that pass a NaN on, the anchor is drawn from the live queries whose angle is a number -- a norm
over NaNs says nothing; the bit comparison covers the others.  Dead pixels: the handed-out query row and radiance are zero.

Weights: vectors 0 and 1 perturbed as test_gpu_mlp.randomize does (EMA != master; inference reads the EMA set), a HashGrid table set to
N(0, 0.3^2) with an EMA offset.  Nothing is trained: frames are Render(None, False).

Every case restates the host's launch rule (renderer_launch, list_encoder_stride below: Mlp::infer / Mlp::launch_features), computes the
rounds from the device's CU count C and asserts which launch form the rule selects, that the launch spans more than one round and that
its last group is ragged -- a changed rule fails here instead of silently testing one round again -- and asserts the frame's live count
exactly, so a changed fixture fails loudly.  Figures in the docstrings are for the 256 CUs of an MI355X."""
import numpy as np
import pytest

from conftest import FRAME_RANDOM, nrc_debug
from test_gpu_mlp import randomize, rel
from test_gpu_mlp_rounds import ceil_div, cu_count

pytestmark = pytest.mark.gpu

# name -> volume ("full": 16^3 voxels of 255; "cloud": the cloud16 fixture), camera position (None: make_camera's default), W, H, live
# pixels (counted with the CPU oracle's nrc_gen_rays, to which k_gen_rays is bit-identical).  W H is a multiple of 16 (the renderer
# refuses anything else).
FRAMES = {
    "all-live": ("full", (30.0, 0.0, 0.0), 784, 431, 337904),      # the camera stands inside the box; the last tile has 16 of 32 entries
    "mostly-live": ("full", None, 1024, 601, 568617),              # 92.4 %, live % 32 = 9
    "cloud": ("cloud", None, 1024, 601, 142906),                   # 23.2 %, large dead regions, live % 32 = 26
    "cloud-4k": ("cloud", None, 2560, 1440, 820388),               # 22.3 %, above 3 << 20 queries
}
# name -> (posID, dirID, width, depth, hashgrid_log2_size)
MODELS = {
    "fused": (3, 0, 64, 6, 0),
    "enc80-64": (3, 0, 64, 2, 0),
    "enc80-128": (3, 0, 128, 2, 0),
    "triwave-64": (2, 0, 64, 2, 0),
    "triwave-128": (2, 2, 128, 2, 0),
    "identity-32": (1, 1, 32, 2, 0),
    "hashgrid-64": (0, 0, 64, 2, 16),
    "hashgrid-128": (0, 2, 128, 2, 14),
}
OTHER_FRAME_RANDOMS = [[0.125, 0.375, 0.625, 0.875], [0.9, 0.1, 0.6, 0.3], [0.45, 0.85, 0.05, 0.7]]
N_ANCHOR = 2048


def query_count(W, H):
    """queries of a frame inside the renderer: whole 8x8 pixel tiles in tile-major order (csrc/nrc_integrator.hip: query_count,
    query_index) -- the n of a launch over the frame and the range of the list's indices"""
    return ceil_div(W, 8) * ceil_div(H, 8) * 64


def is_fused(model):
    return model[:4] == (3, 0, 64, 6)


def renderer_launch(model, n, C, listed):
    """Mlp::infer with skip_zero_queries for a launch over n queries (the whole frame with a list -- the live count is known to the
    device only --, a batch without one) -> (launch form, queries per workgroup and round, workgroups).
    fused 6x64: k_infer<6, T, 2, LISTED>, T = 256 up to 3 << 20 queries and 512 above; a workgroup takes T / 64 waves x 2 tiles of 32 per
    round; ceil(tiles / that) workgroups, capped at 2 C.
    generic up to 64 neurons: k_infer_gen<W, 256, ., 2>: 4 waves x 2 tiles = 256 queries per group; ceil(tiles / 8), capped at 4 C.
    generic 128 neurons, renderer mode only: k_infer_gen<128, 256, ., 1>: 4 waves x 1 tile = 128 queries per group; ceil(tiles / 4),
    capped at NRC_GEN128_WG4_PER_CU = 2 per CU."""
    tiles = ceil_div(n, 32)
    width = max(model[2], 32)
    if is_fused(model):
        threads = 256 if n <= 3 << 20 else 512
        per = threads // 64 * 2
        return "k_infer<6,%d,2,%s>" % (threads, "LISTED" if listed else "false"), per * 32, min(ceil_div(tiles, per), 2 * C)
    if width <= 64:
        return "k_infer_gen<%d,256,NT=2>%s" % (width, " list" if listed else " skip_in"), 256, min(ceil_div(tiles, 8), 4 * C)
    return "k_infer_gen<128,256,NT=1>%s" % (" list" if listed else " skip_in"), 128, min(ceil_div(tiles, 4), 2 * C)


def list_encoder_stride(C):
    """Mlp::launch_features, k_encode_hash_list: 2 C chunks per feature slot (both launch mappings: gridDim.y = slots, or the XCD
    mapping with gridDim.y == 1 and xcd_chunks = 2 C), a chunk walks the list 256 entries at a time -> list entries per stride"""
    return 2 * C * 256


def check_listed_rounds(model, frame, C, want_form):
    """the round conditions of a launch over the frame's list; -> figures for the log"""
    _, _, W, H, live = FRAMES[frame]
    form, per_group, grid = renderer_launch(model, query_count(W, H), C, True)
    groups = ceil_div(ceil_div(live, 32), per_group // 32)
    assert form == want_form, (form, want_form)
    assert groups > grid, "one round: %d groups on %d workgroups" % (groups, grid)
    assert live % per_group != 0 and live % 32 != 0, "no ragged last group"
    fig = dict(form=form, rounds=round(groups / grid, 2))
    if model[0] == 0:
        stride = list_encoder_stride(C)
        assert live > stride and live % stride != 0 and live % 256 != 0, "k_encode_hash_list: one stride"
        fig["encoder_strides"] = round(live / stride, 2)
    return fig


@pytest.fixture(scope="module")
def volumes(cloud16):
    return {"full": np.full((16, 16, 16), 255, np.uint8), "cloud": cloud16}


def setup(api, sc, volumes, frame, model, log2_infer_batch_size):
    """test_gpu_integrator._nrc_setup with the frame's camera -> (cache, renderer)"""
    vol, pos, W, H, _ = FRAMES[frame]
    scene = sc.make_scene(volumes[vol], scene_id=4)
    cfg = api.AppConfig(train_batch_count=1, log2_train_batch_size=10, log2_infer_batch_size=log2_infer_batch_size, pos_id=model[0],
                        dir_id=model[1], nn_width=model[2], nn_depth=model[3], hashgrid_log2_size=model[4])
    nrc = api.NeuralRadianceCache(cfg)
    cam = sc.make_camera(aspect=W / H) if pos is None else sc.make_camera(pos=pos, aspect=W / H)
    return nrc, api.NrcHpmRenderer(W, H, False, cam, cfg, scene, nrc)


def make_oracle(orc, model):
    return orc.nn_create(pos_id=model[0], dir_id=model[1], width=model[2], depth=model[3], hashgrid_log2_size=model[4])


def set_weights(nrc, onn, model):
    """seeded, EMA != master; the oracle network holds the same vectors afterwards"""
    assert nrc.ParamCount() == onn.n_params
    randomize(nrc, onn, seed=3, scale=1.0)
    if model[0] == 0:      # O(0.3) table entries so that the gathers matter (test_hashgrid_model_matches_oracle)
        rng = np.random.default_rng(17)
        nm, nt = onn.n_mlp, onn.n_params - onn.n_mlp
        w, e = np.array(onn.buffer(0)), np.array(onn.buffer(1))
        w[nm:] = (rng.standard_normal(nt) * 0.3).astype(np.float32)
        e[nm:] = w[nm:] + (rng.standard_normal(nt) * 0.05).astype(np.float32)
        onn.buffer(0)[:] = w
        onn.buffer(1)[:] = e
        nrc.SetParams(0, w)
        nrc.SetParams(1, e)


def same_bits(torch, a, b):
    """uint32 equality per element, a NaN on both sides counting as equal"""
    return (a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))


_REFERENCE = {}      # (model name, frame) -> (live queries, dense radiance, anchor rows, oracle radiance of the anchor rows); never changed


def reference(api, orc, torch, name, frame, onn, q_live):
    """the dense kernel's radiance of the frame's live queries (public order) and the oracle's of the anchor rows: computed once per
    (model, frame) -- the frame and the weights are seeded, so every test of the pair must meet the very same queries"""
    key = (name, frame)
    if key in _REFERENCE:
        assert torch.equal(_REFERENCE[key][0].view(torch.int32), q_live.view(torch.int32)), "the frame's live queries changed between tests"
        return _REFERENCE[key][1:]
    model = MODELS[name]
    dense_cache = api.NeuralRadianceCache(api.AppConfig(pos_id=model[0], dir_id=model[1], nn_width=model[2], nn_depth=model[3],
                                                        hashgrid_log2_size=model[4]))
    dense_cache.SetParams(0, np.array(onn.buffer(0)))
    dense_cache.SetParams(1, np.array(onn.buffer(1)))
    dense = torch.full((q_live.shape[0], 3), -7.0, device="cuda")
    dense_cache.Infer(q_live, dense, useEma=True)
    torch.cuda.synchronize()
    dense_cache.Destroy()
    usable = torch.arange(q_live.shape[0], device="cuda")
    if model[1] != 0:      # only OneBlob absorbs a NaN angle
        usable = usable[~torch.isnan(q_live[:, 4])]
    pick = np.sort(np.random.default_rng(2048).choice(int(usable.shape[0]), N_ANCHOR, replace=False))
    rows = usable[torch.from_numpy(pick).cuda()]
    ref = onn.forward(q_live[rows].cpu().numpy(), True, 1)
    _REFERENCE[key] = (q_live.clone(), dense, rows, ref)
    return _REFERENCE[key][1:]


def live_mask(ren, W, H):
    """the pixels that scattered, in the x * H + y order the query and radiance buffers are handed out in"""
    return ren.Buffer("info").reshape(H, W).t().reshape(-1) == 1.0


def render_and_check(api, orc, sc, torch, volumes, name, frame, log2_infer_batch_size, n_frames, tag, expect_list):
    """n_frames - 1 frames with other frame randoms (the buffer sets are triple-buffered and the list counter of a set is cleared by the
    compositing launch of its last user: the fourth frame reuses the first set, at full size), then the frame of FRAME_RANDOM, which is
    checked.  -> the renderer's list of live query indices (its own tile-major order; device tensor) when it keeps one"""
    model = MODELS[name]
    _, _, W, H, want_live = FRAMES[frame]
    nrc, ren = setup(api, sc, volumes, frame, model, log2_infer_batch_size)
    onn = make_oracle(orc, model)
    set_weights(nrc, onn, model)
    for fr in OTHER_FRAME_RANDOMS[:n_frames - 1] + [FRAME_RANDOM]:
        ren.SetFrameRandom(fr)
        ren.Render(None, False)
    live = live_mask(ren, W, H)
    n_live = int(live.sum())
    assert n_live == want_live, "the frame's live count changed: %d, expected %d" % (n_live, want_live)
    q_pub = ren.Buffer("infer_input").clone()
    out_pub = ren.Buffer("infer_output").clone()
    live_list = None
    if expect_list:
        live_list = ren.Buffer("live")[1:1 + n_live].clone()
        assert int(live_list.min()) >= 0 and int(live_list.max()) < query_count(W, H) and int(torch.unique(live_list).shape[0]) == n_live
    else:
        with pytest.raises(RuntimeError, match="keeps no live-query list"):
            ren.Buffer("live")
    ren.Destroy()
    nrc.Destroy()
    # dead pixels: what test_live_query_list_changes_no_pixel asserts for them
    assert not bool(q_pub[~live].any()) and not bool(out_pub[~live].any())
    q_live, out_live = q_pub[live].contiguous(), out_pub[live].contiguous()
    nan_angle = float(torch.isnan(q_live[:, 4]).float().mean())
    assert nan_angle > 0.0 and not bool(torch.isnan(q_live[:, :4]).any())      # quirk Q5 is in the frame (about 15 % of the live queries)
    dense, rows, ref = reference(api, orc, torch, name, frame, onn, q_live)
    # the reference is no trivial one: finite wherever the query is absorbed, and not zero
    absorbed = torch.ones_like(q_live[:, 4], dtype=torch.bool) if model[1] == 0 else ~torch.isnan(q_live[:, 4])
    assert bool(torch.isfinite(dense[absorbed]).all()) and float(dense[absorbed].abs().max()) > 0.0
    assert float((dense[absorbed].abs().sum(dim=1) > 0.0).float().mean()) > 0.5
    same = same_bits(torch, out_live, dense).all(dim=1)
    differ = int((~same).sum())
    got = out_live[rows].cpu().numpy()
    err = rel(got, ref)
    tol = 3e-2 if model[0] == 0 else (2e-3 if is_fused(model) else 3e-3)
    print("RENDER-ROUNDS %s: live %d (NaN angle %.3f), %d live pixels differ from the dense kernel, anchor rel-L2 %.3g (bound %g)" % (
        tag, n_live, nan_angle, differ, err, tol))
    assert differ == 0, (tag, differ, torch.nonzero(~same)[:8].reshape(-1).tolist())
    assert np.isfinite(got).all() and np.isfinite(ref).all(), tag
    assert err < tol, (tag, err)
    return live_list


CASES_A = [(m, "all-live") for m in MODELS] + [("fused", "cloud"), ("hashgrid-64", "cloud")]
FORMS_LISTED = {
    "fused": "k_infer<6,256,2,LISTED>", "enc80-64": "k_infer_gen<64,256,NT=2> list", "enc80-128": "k_infer_gen<128,256,NT=1> list",
    "triwave-64": "k_infer_gen<64,256,NT=2> list", "triwave-128": "k_infer_gen<128,256,NT=1> list",
    "identity-32": "k_infer_gen<32,256,NT=2> list", "hashgrid-64": "k_infer_gen<64,256,NT=2> list",
    "hashgrid-128": "k_infer_gen<128,256,NT=1> list",
}


@pytest.mark.parametrize("name,frame", CASES_A, ids=["%s-%s" % c for c in CASES_A])
def test_one_batch_with_the_live_list(api, orc, sc, torch_gpu, volumes, name, frame):
    """log2_infer_batch_size = 21: the frame is ONE batch and every model runs over the list.
    all-live, 784x431, 337 904 live queries = 10 559 tiles and one of 16 entries: 2.58 rounds of k_infer<6,256,2,LISTED> (the second and
    third through the prefetched, carried list index), 1.29 of k_infer_gen up to 64 neurons (330 of 1 024 workgroups run a second group:
    stage parity 3 at depth 2), 5.2 of the 128-wide 4-wave form, 2.58 strides of k_encode_hash_list.
    cloud, 1024x601, 142 906 live queries of 615 424 in no particular order, reaching all over the query buffer: 1.09 rounds of k_infer
    and 1.09 strides of k_encode_hash_list (fused and hashgrid-64 only: k_infer_gen<64> itself stays inside a round on this frame).
    The fourth frame of the renderer is checked: its buffer set and list are the first frame's, used again.
    Measured on an MI355X: see docs/MEASUREMENT_LOG.md (no live pixel of any case differed from the dense kernel)."""
    C = cu_count(torch_gpu)
    model = MODELS[name]
    if frame == "cloud" and not is_fused(model):
        # k_infer_gen<64> stays inside one round on this frame (559 groups on 1 024 workgroups): the case is here for the list encoder
        _, _, W, H, live = FRAMES[frame]
        form, per_group, grid = renderer_launch(model, query_count(W, H), C, True)
        assert form == FORMS_LISTED[name]
        stride = list_encoder_stride(C)
        assert live > stride and live % stride != 0 and live % 256 != 0, "k_encode_hash_list: one stride"
        fig = dict(form=form, encoder_strides=round(live / stride, 2))
    else:
        fig = check_listed_rounds(model, frame, C, FORMS_LISTED[name])
    tag = "A %s %s %s" % (name, frame, fig)
    render_and_check(api, orc, sc, torch_gpu, volumes, name, frame, 21, 4, tag, expect_list=True)


@pytest.mark.parametrize("name", ["fused", "enc80-64"])
def test_batches_merged_into_one_launch_over_the_list(api, orc, sc, torch_gpu, volumes, name):
    """log2_infer_batch_size = 16 on all-live: the reference's slicing gives five batches of 65 536 queries and one of 10 224, and
    Cache::infer_all turns them into ONE launch over the list for the models that encode inside their kernel -- the launch of case A,
    so the radiance is bit-identical to case A's under the same reference (it is shared).  The renderer keeps a list (Buffer("live"))."""
    C = cu_count(torch_gpu)
    _, _, W, H, _ = FRAMES["all-live"]
    assert ceil_div(query_count(W, H), 1 << 16) == 6
    fig = check_listed_rounds(MODELS[name], "all-live", C, FORMS_LISTED[name])
    live_list = render_and_check(api, orc, sc, torch_gpu, volumes, name, "all-live", 16, 4, "B %s all-live %s" % (name, fig), expect_list=True)
    assert live_list is not None and int(live_list.max()) >= 5 << 16      # the list reaches into the last batch's queries


_LIVE_INDICES = {}      # frame -> internal (tile-major) query indices of its live pixels, from a list-mode renderer; never changed


def live_indices(api, sc, torch, volumes, frame):
    if frame not in _LIVE_INDICES:
        _, _, W, H, want_live = FRAMES[frame]
        nrc, ren = setup(api, sc, volumes, frame, MODELS["fused"], 21)
        ren.SetFrameRandom(FRAME_RANDOM)
        ren.Render(None, False)
        n_live = int((ren.Buffer("info") == 1.0).sum())
        assert n_live == want_live
        _LIVE_INDICES[frame] = ren.Buffer("live")[1:1 + n_live].clone().to(torch.int64)
        ren.Destroy()
        nrc.Destroy()
    return _LIVE_INDICES[frame]


def units_behind_round_one(torch, idx, n_batch, unit, first_round_units):
    """for the units (consecutive `unit` queries) of batch 0 = queries 0 .. n_batch - 1 behind the first round (unit index >=
    first_round_units): whether the unit holds a live query (host array of bool)"""
    assert n_batch % unit == 0
    present = torch.zeros(n_batch // unit, dtype=torch.bool, device=idx.device)
    present[idx[idx < n_batch] // unit] = True
    return present[first_round_units:].cpu().numpy()


def check_skipped_and_running_units(later, tag):
    """one unit behind the first round holds no live query -- it is skipped whole -- and a LATER one holds some: it runs behind the skip"""
    dead = np.flatnonzero(~later)
    assert dead.size > 0, "%s: no unit behind the first round is skipped whole" % tag
    assert later[dead[0]:].any(), "%s: no unit runs behind a skipped one" % tag
    return int(dead.size), int(later.sum())


def workgroups_that_skip_then_run(present, first_round_units):
    """`present`: the units of batch 0 behind round one (units_behind_round_one, one unit per group; a round is first_round_units groups).
    Workgroup w takes groups w, w + grid, w + 2 grid, ...: -> (workgroups whose sequence holds a skipped group with a running one behind
    it, workgroups that ran a group before such a skip).  This is what `continue` has to survive: the skip leaves stage 0 staged in
    buffer q & 1 for the running group behind it, and after a group that ran, q is what that group's stages left."""
    grid = first_round_units
    rounds = ceil_div(present.size, grid)
    seq = np.zeros(rounds * grid, bool)
    seq[:present.size] = present
    seq = seq.reshape(rounds, grid)
    runs_later = np.flip(np.maximum.accumulate(np.flip(seq, 0), 0), 0)
    ran_before = np.maximum.accumulate(seq, 0)
    skip_then_run = ~seq[:-1] & runs_later[1:]
    return int(skip_then_run.any(0).sum()), int((skip_then_run[1:] & ran_before[:-2]).any(0).sum()) if rounds > 2 else 0


CASES_C = [(m, f) for f in ("cloud", "mostly-live") for m in ("triwave-64", "triwave-128", "hashgrid-64", "hashgrid-128")]


@pytest.mark.parametrize("name,frame", CASES_C, ids=["%s-%s" % c for c in CASES_C])
def test_several_batches_without_a_list(api, orc, sc, torch_gpu, volumes, name, frame):
    """log2_infer_batch_size = 19 at 1024x601 and a model with an encoder kernel: wants_live_list() is false, the renderer keeps no list
    and launches k_encode / k_encode_hash_lm + k_infer_gen with skip_in per batch -- batch 0 is 524 288 consecutive queries (2 048 groups
    of 256 on 1 024 workgroups: 2 rounds; 4 096 groups of 128 on 512 workgroups at 128 neurons: 8 rounds), batch 1 the rest at a pointer
    offset: 98 304 queries, for the renderer's query buffer holds whole 8x8 pixel tiles (128 x 76 x 64 = 622 592 queries, not W H).  Both
    batches are whole groups: what is ragged here is the content.  A group whose queries are all dead is skipped with `continue` while
    stage 0 stays staged and the stage parity runs on, and batch 0 holds such a group behind the first round with a running group behind
    it -- shown from the live indices a list-mode renderer of the same frame reports, in the renderer's own query order.
    cloud: 672 groups of 256 skipped and 352 running behind round one; 2 160 and 1 424 of 128.  What matters to `continue` is the
    sequence of ONE workgroup, and that is asserted as well: 174 of the 1 024 workgroups skip their first group and run their second
    (two rounds allow nothing else); at 128 neurons 328 of 512 workgroups run a group behind a skipped one, 18 of them after they had
    run an earlier group (the parity q is not 0 at the skip).
    mostly-live: 112 groups of 128 skipped, 3 472 running -- but the dead groups are the frame's left and right margins, a round is eight
    rows of pixel tiles, and so the workgroups that skip a group skip all of theirs: no workgroup runs a group behind a skip at either
    width (scratch mutant: `q++` in front of the `continue` passes these four cases and fails the four of cloud).  At 256 queries per
    group the frame holds NO group without a live query behind round one (asserted, so that the sentence stays true): there the 64-wide
    kernels meet waves whose two tiles are dead inside running groups (159 of them) -- `wave_runs` false beside running waves.  These
    cases are multi-round launches over mostly running groups and a second batch at a pointer offset; the `continue` path is cloud's."""
    C = cu_count(torch_gpu)
    model = MODELS[name]
    _, _, W, H, _ = FRAMES[frame]
    n0 = 1 << 19
    assert n0 < query_count(W, H) < 2 * n0 and query_count(W, H) - n0 == 98304
    form, per_group, grid = renderer_launch(model, n0, C, False)
    assert form == ("k_infer_gen<128,256,NT=1> skip_in" if model[2] == 128 else "k_infer_gen<64,256,NT=2> skip_in")
    groups = n0 // per_group
    assert groups >= 2 * grid, "batch 0 is less than two rounds"
    idx = live_indices(api, sc, torch_gpu, volumes, frame)
    later = units_behind_round_one(torch_gpu, idx, n0, per_group, grid)
    all_groups = units_behind_round_one(torch_gpu, idx, n0, per_group, 0)
    skip_run, run_skip_run = workgroups_that_skip_then_run(all_groups, grid)
    if frame == "cloud":
        assert skip_run > 0, "no workgroup runs a group behind a skipped one"
        assert run_skip_run > 0 or groups // grid == 2, "no workgroup skips a group between two running ones"
    if frame == "mostly-live" and per_group == 256:
        assert later.all(), "the frame now holds a skipped group of 256 behind round one: assert it as the other cases do"
        pairs = units_behind_round_one(torch_gpu, idx, n0, 64, grid * 4)
        assert not pairs.all(), "no wave of a running group is idle"
        what = "every group runs, %d waves idle in running groups" % int((~pairs).sum())
    else:
        what = "%d groups skipped, %d running" % check_skipped_and_running_units(later, name)
    tag = "C %s %s %s rounds %.2f, behind round one: %s; workgroups that run behind a skip %d, between two runs %d" % (
        name, frame, form, groups / grid, what, skip_run, run_skip_run)
    render_and_check(api, orc, sc, torch_gpu, volumes, name, frame, 19, 1, tag, expect_list=False)


def test_fused_kernel_without_a_list(api, orc, sc, torch_gpu, volumes, monkeypatch):
    """NRC_DEBUG=no_live_list, fused model, cloud at log2_infer_batch_size = 19: k_infer<6,256,2,false> with zero-tile skipping -- batch 0
    is 16 384 tiles on 512 workgroups of 8 tiles: 4 rounds; a wave's pair of tiles (64 queries) that holds no live query stores zeros
    without running the network, and such pairs (3 752) and running ones (2 392) both lie behind the first round."""
    C = cu_count(torch_gpu)
    model = MODELS["fused"]
    n0 = 1 << 19
    form, per_group, grid = renderer_launch(model, n0, C, False)
    assert form == "k_infer<6,256,2,false>" and n0 // per_group >= 2 * grid
    idx = live_indices(api, sc, torch_gpu, volumes, "cloud")      # (rendered before the switch is set: that renderer keeps its list)
    skipped, running = check_skipped_and_running_units(units_behind_round_one(torch_gpu, idx, n0, 64, grid * per_group // 64), "fused")
    nrc_debug(monkeypatch, no_live_list=True)
    tag = "C fused cloud %s rounds %.2f, behind round one: %d tile pairs skipped, %d running" % (form, n0 // per_group / grid, skipped, running)
    render_and_check(api, orc, sc, torch_gpu, volumes, "fused", "cloud", 19, 1, tag, expect_list=False)
    nrc_debug(monkeypatch)


def test_eight_wave_fused_form_above_three_million_queries(api, orc, sc, torch_gpu, volumes):
    """cloud at 2560x1440 = 3 686 400 queries in one batch (log2_infer_batch_size = 22): above 3 << 20 the host launches
    k_infer<6,512,2,LISTED>, 1 024 C list entries per round -- 820 388 live queries are 3.13 rounds, the last group with 164 of 512."""
    C = cu_count(torch_gpu)
    _, _, W, H, live = FRAMES["cloud-4k"]
    assert 3 << 20 < query_count(W, H) <= 1 << 22 and live > 1024 * C
    fig = check_listed_rounds(MODELS["fused"], "cloud-4k", C, "k_infer<6,512,2,LISTED>")
    render_and_check(api, orc, sc, torch_gpu, volumes, "fused", "cloud-4k", 22, 1, "D fused cloud-4k %s" % fig, expect_list=True)
