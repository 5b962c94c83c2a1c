"""The capped-state side of the exact empty-space skip, pinned: which RNG states can run into DeltaTrack's cap of 128 collisions in empty
space (k_flight_table), which of them a medium selects (k_flight_select: count, list of up to eight, one bit per state) and what skip_setup
makes of it (list or bits mode, no mask above lambda 100).

* The device's table -- the one the renderers read, through nrc_test_flight_select -- is the oracle's, bit for bit, for all 2^23 states.
* The selection at twelve lambdas (below, between, at and above table values; NaN) is flight_reference.select()'s of that table.
* End to end, in a view along the diagonal of an EMPTY box, where every tile is one the mask rejects and a pixel scatters only by running
  into the cap: frames that pin a pixel into each of the seven small non-zero capped states, in list mode (eight states) and with one
  state more (bits mode); 64 ordinary frames of a medium dense enough for 30 000 capped states, in which 84 pixels scatter; and the two
  sides of lambda = 100.  Frames with the skip, without it and the oracle's are bit-identical.

tests/test_flight_reference_cpu.py holds the references to the fp64 table and shows that these assertions reject wrong implementations.
Not seen here: a state wrongly ADDED to the selection by skip_setup's own list handling -- it costs time, never a pixel."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flight_cases as cases  # noqa: E402
import flight_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = cases.W, cases.H
CFG = dict(train_batch_count=1, log2_train_batch_size=8, log2_infer_batch_size=14)
LAMBDA_IDS = ["minus-1", "0", "70", "equal-70.0336", "tie-70.7917", "80-list-full", "equal-82.6352-nine", "97.4", "100", "300", "inf", "nan"]


@pytest.fixture(scope="module")
def device_table(api, torch_gpu):
    """the free-flight table the renderers of this process read"""
    return api.test_flight_select(-1.0, want_table=True)[4]


def test_device_table_is_the_oracle_table(device_table):
    ref.check_table(device_table, cases.oracle_table())


@pytest.mark.parametrize("lam", [lam for lam, _ in ref.LAMBDAS], ids=LAMBDA_IDS)
def test_selection_matches_the_reference(api, device_table, lam):
    out = api.test_flight_select(lam)
    print("lambda %r: count %d, list %r" % (lam, out[0], out[1].tolist()))
    ref.check_selection(device_table, lam, *out, api.FLIGHT_BITS_SENTINEL)


def test_selection_on_reused_buffers_leaves_nothing_stale(api, device_table, torch_gpu):
    """a renderer reuses its buffers from one medium to the next: 97.4 and then 70.0 on the same ones"""
    fill = api.FLIGHT_BITS_SENTINEL - (1 << 32)
    buffers = (torch_gpu.full((9,), fill, dtype=torch_gpu.int32, device="cuda"),
               torch_gpu.full((ref.N_WORDS + 2,), fill, dtype=torch_gpu.int32, device="cuda"))
    first = api.test_flight_select(97.4, buffers=buffers)
    ref.check_selection(device_table, 97.4, *first, api.FLIGHT_BITS_SENTINEL)
    assert first[0] > ref.LIST_MAX
    ref.check_selection(device_table, 70.0, *api.test_flight_select(70.0, buffers=buffers), api.FLIGHT_BITS_SENTINEL)


# ------------------------------------------------------------------------------------------------------------------ end to end
def render(api, density_factor, frame_randoms, tile=None):
    """{skip: [per frame (primary, info, infer_input, MC image, NRC density look-ups, HotTiles())]} of the diagonal view of the empty box"""
    from nrc_hpm_renderer_amd import parallel
    scene, cam = cases.scene(density_factor), cases.camera()
    lw = W if tile is None else parallel.local_width(tile[0], tile[1], W)
    out = {}
    for skip in (True, False):
        cfg = api.AppConfig(**CFG)
        nrc = api.NeuralRadianceCache(cfg)
        ren = api.NrcHpmRenderer(lw, H, False, cam, cfg, scene, nrc, tile=tile)
        mc = api.McHpmRenderer(lw, H, cases.MC_PATH_LENGTH, False, cam, scene, tile=tile)
        ren.SetEmptySkip(skip)
        mc.SetEmptySkip(skip)
        ren.CountFetches(True)
        frames = []
        for frame_random in frame_randoms:
            ren.SetFrameRandom(frame_random)
            ren.Render(None, False)
            n_fetch = ren.CountFetches(True)
            mc.SetFrameRandom(frame_random)
            mc.Render()
            frames.append((ren.Buffer("primary").cpu().numpy().reshape(H, lw, 4).copy(), ren.Buffer("info").cpu().numpy().reshape(H, lw).copy(),
                           ren.Buffer("infer_input").cpu().numpy().reshape(lw, H, 5).copy(), mc.GetImage().cpu().numpy().copy(), n_fetch,
                           ren.HotTiles()))
        out[skip] = frames
        mc.Destroy()
        ren.Destroy()
        nrc.Destroy()
    return out


def check_frames(out, density_factor, frame_randoms, columns=None):
    """skip on == skip off == the oracle, on every frame and in every buffer"""
    sel = slice(None) if columns is None else columns
    for k, frame_random in enumerate(frame_randoms):
        o = cases.oracle_frame(density_factor, frame_random)
        want = (o["primary"][:, sel], o["info"][:, sel], o["infer_input"].reshape(W, H, 5)[sel], o["mc"][:, sel])
        for b, name in enumerate(("primary", "info", "infer_input", "MC image")):
            assert ref.same_bits(out[True][k][b], out[False][k][b]), "frame %d, %s: the skip changes the frame" % (k, name)
            assert ref.same_bits(out[True][k][b], want[b]), "frame %d, %s: not the oracle's" % (k, name)
        if columns is None:
            assert out[False][k][4] == o["n_fetch"]           # without the mask the device executes the algorithm's look-ups


@pytest.mark.parametrize("density_factor", [cases.RHO_LIST, cases.RHO_NINE], ids=["list-of-8", "bits-9-states"])
def test_a_pixel_pinned_into_each_small_capped_state(api, torch_gpu, density_factor):
    """One frame per non-zero capped state below the ninth entry, the pixel of the central ray (or its neighbour) pinned into that state: it
    scatters, alone in its frame, although every tile of the view is empty.  At 0.74 skip_setup hands the eight states over as a list -- a
    dropped entry or a wrong comparison loses the pixel; at 0.765 a ninth state switches to the bit table, of which these frames read
    seven individual bits.  (What these frames cannot see is a table whose chain starts one draw late: the seven states are a 3-cycle of
    the hash, 2282633 -> 1922895 -> 5527704 -> 2282633, and its four other preimages, so such a table selects the same eight.  The table
    comparison and the 64 ordinary frames see it.)"""
    states = sorted(cases.PINNED)
    frame_randoms = [cases.PINNED[s][1] for s in states]
    out = render(api, density_factor, frame_randoms)
    check_frames(out, density_factor, frame_randoms)
    for k, state in enumerate(states):
        x, y = cases.PINNED[state][0]
        info = cases.oracle_frame(density_factor, frame_randoms[k])["info"]
        assert info[y, x] == 1.0 and info.sum() == 1.0
        on, off = out[True][k], out[False][k]
        print("state %d: look-ups %d with the skip, %d without, HotTiles() %r" % (state, on[4], off[4], on[5]))
        assert 0 < on[4] < off[4]
        assert off[5] is None
        if density_factor == cases.RHO_LIST:
            assert on[5] is not None and on[5][0] == [(x // 8, y // 8)] and on[5][1] == 1
        else:
            assert on[5] is None                              # tiles are promoted from the list only (camera_launch_setup): none in bits mode


def test_bits_mode_at_scale(api, torch_gpu):
    """30 000 capped states: over 64 ordinary frames 84 pixels of the empty box scatter (at least 40: asserted), each found through its
    bit of the device's bit table.  A bit lost anywhere among those the frames read loses a pixel."""
    frame_randoms = cases.scale_frame_randoms()
    out = render(api, cases.RHO_BITS, frame_randoms)
    check_frames(out, cases.RHO_BITS, frame_randoms)
    scattered = sum(int(cases.oracle_frame(cases.RHO_BITS, fr)["info"].sum()) for fr in frame_randoms)
    assert scattered >= 40
    assert sum(f[4] for f in out[True]) < sum(f[4] for f in out[False])
    assert all(f[4] <= g[4] for f, g in zip(out[True], out[False]))


def test_bits_mode_as_column_tile_3_of_8(api, torch_gpu):
    """the RNG seed is the pixel's GLOBAL column: one of the scale frames as the strip of rank 3 of 8, which holds one of its scattered pixels"""
    from nrc_hpm_renderer_amd import parallel
    frame_randoms = cases.scale_frame_randoms()[cases.TILED_FRAME:cases.TILED_FRAME + 1]
    columns = cases.tile_columns()
    assert cases.oracle_frame(cases.RHO_BITS, frame_randoms[0])["info"][:, columns].sum() >= 1.0
    out = render(api, cases.RHO_BITS, frame_randoms, tile=parallel.column_tile(cases.TILED_RANK, cases.TILED_WORLD, W, H))
    check_frames(out, cases.RHO_BITS, frame_randoms, columns=columns)
    assert out[True][0][4] < out[False][0][4]


def test_lambda_boundary(api, torch_gpu):
    """skip_setup refuses the mask above lambda 100: at density factor 0.92 (99.6) it is applied -- fewer look-ups --, at 0.93 (100.6) it
    is not -- the same look-ups --, and both frames are the oracle's"""
    assert ref.skip_lambda(cases.scene(cases.RHO_BITS)) <= 100.0 < ref.skip_lambda(cases.scene(cases.RHO_OFF))
    frame_randoms = cases.scale_frame_randoms()[:2]
    applied = render(api, cases.RHO_BITS, frame_randoms)
    check_frames(applied, cases.RHO_BITS, frame_randoms)
    refused = render(api, cases.RHO_OFF, frame_randoms)
    check_frames(refused, cases.RHO_OFF, frame_randoms)
    for k in range(len(frame_randoms)):
        assert applied[True][k][4] < applied[False][k][4]
        assert refused[True][k][4] == refused[False][k][4]
    assert sum(int(cases.oracle_frame(cases.RHO_OFF, fr)["info"].sum()) for fr in frame_randoms) >= 1
