"""The references tests/test_gpu_flight_states.py pins the capped-state side of the empty-space skip to, checked on the CPU:

* the oracle's free-flight table (orc_flight_table, written from delta_track's statement) against fp64 sums with log1p
  (tests/flight_reference.py: plain numpy) within the derived bound, and the counts of states below the lambdas the GPU test selects at;
* the 0.2 % skip_lambda adds: the fp32 recurrence delta_track really runs, t = fma(-log(1 - u), 1 / sigma, t), against the table;
* the assertions the GPU test makes (flight_reference.check_table / check_selection) run against eight deliberately wrong tables and
  selections -- each must be rejected at a named case, and the right ones accepted."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flight_cases as cases  # noqa: E402
import flight_reference as ref  # noqa: E402
import rng_search  # noqa: E402

SENTINEL = 0xA5C3F00D
BLOCK = 1 << 16
BLOCKS = {      # four blocks of 2^16 states
    "first": np.arange(BLOCK, dtype=np.uint32),
    "middle": np.arange(1 << 22, (1 << 22) + BLOCK, dtype=np.uint32),
    "last": np.arange(ref.N_STATES - BLOCK, ref.N_STATES, dtype=np.uint32),
    "strided": np.arange(BLOCK, dtype=np.uint32) * np.uint32(128) + np.uint32(77),
}


@pytest.fixture(scope="session")
def table():
    return cases.oracle_table()


def spec_log_term(orc):
    """u -> -orc_logf(1 - u) in fp32: the flight term of delta_track with the math spec's log"""
    return lambda u: -orc.math_eval(0, np.float32(1.0) - u)[0]


# ------------------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("block", sorted(BLOCKS))
def test_oracle_table_is_within_the_derived_bound_of_fp64_sums(table, block):
    """measured: 9.3e-5 (first), 9.7e-5 (middle), 1.06e-4 (last), 1.02e-4 (strided); the bound is 1.1e-3"""
    states = BLOCKS[block]
    dev = np.abs(ref.table64(states) - table[states].astype(np.float64))
    print("block %s: largest |fp32 table - fp64 sums| = %.3e (bound %.3e)" % (block, dev.max(), ref.TABLE_BOUND))
    assert dev.max() <= ref.TABLE_BOUND
    assert (table[states] < 256.0).all()                      # what the bound assumes of the sums


def test_oracle_table_blocks_agree_with_a_table_that_starts_elsewhere(orc, table):
    """orc_flight_table's `first` / `count` and its threads: pieces of the table equal the whole, whatever the number of threads"""
    for first, count, threads in ((0, 5, 1), (1 << 22, 4097, 3), (ref.N_STATES - 9000, 9000, 16)):
        assert ref.same_bits(orc.flight_table(first, count, threads), table[first:first + count])


def test_the_numpy_chain_with_the_spec_log_is_the_oracle_table(orc, table):
    """two statements of one chain, written apart: flight_reference.walk_sum with the oracle's log, summed in fp32, is the oracle's table bit
    for bit -- the right chain passes the check the wrong ones below fail"""
    for block in ("first", "strided"):
        ref.check_table(ref.walk_sum(BLOCKS[block], spec_log_term(orc), np.float32), table[BLOCKS[block]])


def test_small_entries_and_counts(table):
    """the figures the GPU test's lambdas were chosen from: one entry is 0, seven lie in 70.03 .. 70.85 (two triple ties), the ninth smallest
    is 82.63517, 30 335 do not exceed 100"""
    order = np.argsort(table, kind="stable")[:9]
    assert order[0] == 0 and table[0] == 0.0
    assert sorted(order[1:8].tolist()) == sorted(ref.SMALL_STATES)
    values = table[np.asarray(ref.SMALL_STATES)]
    assert values.tolist() == [np.float32(70.03356170654297)] + [np.float32(70.79169464111328)] * 3 + [np.float32(70.84893798828125)] * 3
    assert order[8] == 3416349 and table[3416349] == np.float32(82.63516998291016)
    want = {-1.0: 0, 0.0: 1, 70.0: 1, 70.03: 1, float(np.float32(70.03356170654297)): 2, float(np.float32(70.79169464111328)): 5, 80.0: 8,
            82.64: 9, float(np.float32(82.63516998291016)): 9, 100.0: 30335, 300.0: ref.N_STATES, float("inf"): ref.N_STATES,
            float("nan"): ref.N_STATES}
    for lam, n in want.items():
        assert ref.select(table, lam)[0] == n, lam
    n_974 = ref.select(table, 97.4)[0]
    assert 8 < n_974 < 30335


def test_select_bit_layout():
    """bit (m & 31) of word (m >> 5), on a table whose selection is known without select()"""
    t = np.full(ref.N_STATES, 5.0, np.float32)
    picked = [0, 1, 31, 32, 63, 64, 4097, ref.N_STATES - 1]
    t[picked] = 1.0
    t[77] = np.nan
    n, states, bits = ref.select(t, 1.0)
    assert n == 9 and states.tolist() == sorted(picked + [77])
    want = np.zeros(ref.N_WORDS, np.uint32)
    for m in picked + [77]:
        want[m >> 5] |= np.uint32(1) << np.uint32(m & 31)
    assert (bits == want).all() and bits[0] == 0x80000003 and bits[1] == 0x80000001 and bits[-1] == 0x80000000


def test_skip_lambda_of_the_end_to_end_scenes(table):
    """the density factors of the GPU test's frames give the modes they are there for: a list of exactly eight states, nine states (bits),
    30 000 states (bits), and a lambda above 100 (no mask)"""
    lam = {rho: ref.skip_lambda(cases.scene(rho)) for rho in (cases.RHO_LIST, cases.RHO_NINE, cases.RHO_BITS, cases.RHO_OFF)}
    assert abs(lam[cases.RHO_LIST] - 80.08) < 0.01 and abs(lam[cases.RHO_NINE] - 82.785) < 0.01
    assert abs(lam[cases.RHO_BITS] - 99.56) < 0.01 and abs(lam[cases.RHO_OFF] - 100.64) < 0.01
    n, states, _ = ref.select(table, np.float32(lam[cases.RHO_LIST]))
    assert n == 8 and states.tolist() == sorted([0] + ref.SMALL_STATES)
    assert ref.select(table, np.float32(lam[cases.RHO_NINE]))[0] == 9
    assert 20000 < ref.select(table, np.float32(lam[cases.RHO_BITS]))[0] < 30335
    assert lam[cases.RHO_BITS] <= 100.0 < lam[cases.RHO_OFF]
    # no chord of the view is longer than the diagonal: the states the list leaves out cannot cap at RHO_LIST ...
    assert table[3416349] > cases.RHO_LIST * 107.5
    # ... and every chord is above 95 % of it: the listed states can
    assert table[np.asarray(ref.SMALL_STATES)].max() < cases.RHO_LIST * 0.95 * 107.5


def test_pinned_frames_pin_their_pixel_and_no_other(table):
    """each frame of flight_cases.PINNED puts its pixel into its state, and no other pixel of the frame is in one of the nine smallest states"""
    nine = np.asarray(sorted([0, 3416349] + ref.SMALL_STATES), np.uint32)
    for state, ((x, y), frame_random) in cases.PINNED.items():
        m = cases.frame_states(frame_random)
        assert m[y, x] == state
        assert abs(x - 128) <= 1 and abs(y - 72) <= 1
        assert int(np.isin(m, nine).sum()) == 1
    assert rng_search.frame_random_for_state0(2, 3, 256, 144) == [0.7795426845550537, 0.04615384712815285, 0.75, 0.125]      # the old name
    x, y = cases.PINNED[5527704][0]
    assert rng_search.frame_random_for_state(x, y, 256, 144, 5527704) == cases.PINNED[5527704][1]
    assert rng_search.frame_random_for_state(128, 72, 256, 144, 2282633) is None


def test_oracle_scatters_the_pinned_pixel_alone(table):
    """the cases bite: in the oracle, which walks every ray, the pinned pixel -- and it alone -- scatters in the empty box"""
    for rho in (cases.RHO_LIST, cases.RHO_NINE):
        for state, ((x, y), frame_random) in cases.PINNED.items():
            info = cases.oracle_frame(rho, frame_random)["info"]
            assert info[y, x] == 1.0 and info.sum() == 1.0, (rho, state)


def test_the_scale_frames_scatter_often_enough():
    """bits mode at scale cannot go hollow: over the 64 frames the oracle scatters at least 40 pixels of the empty box (84 here), every one
    in a state the selection at that lambda holds; at least one lies in the columns of the tiled renderer's frame"""
    table = cases.oracle_table()
    lam = np.float32(ref.skip_lambda(cases.scene(cases.RHO_BITS)))
    total = 0
    for frame_random in cases.scale_frame_randoms():
        info = cases.oracle_frame(cases.RHO_BITS, frame_random)["info"]
        m = cases.frame_states(frame_random)
        assert not (table[m[info == 1.0]] > lam).any()
        total += int(info.sum())
    print("scattered pixels over the %d frames: %d" % (cases.SCALE_FRAMES, total))
    assert total >= 40
    info = cases.oracle_frame(cases.RHO_BITS, cases.scale_frame_randoms()[cases.TILED_FRAME])["info"]
    assert info[:, cases.tile_columns()].sum() >= 1.0


# ------------------------------------------------------------------------------------------------------------------ the margin
def margin_states(table):
    """2^16 states: every state whose entry is below 101 (all that any lambda the mask accepts can select), filled up from the others"""
    low = np.nonzero(table < 101.0)[0]
    assert low.size < BLOCK
    rest = np.setdiff1d(np.arange(0, ref.N_STATES, 61), low)[:BLOCK - low.size]
    return np.concatenate([low, rest]).astype(np.uint32)


@pytest.mark.parametrize("sigma", [0.3, 0.74, 0.92])
def test_the_walk_stays_within_half_the_margin_of_the_table(orc, table, sigma):
    """skip_lambda adds 0.2 % for the rounding of the walk's own sums: the walk adds flights of length -log(1 - u) / sigma in fp32,
    t = fma(-log(1 - u), 1 / sigma, t) with 1 / sigma rounded, while the table adds -log(1 - u).  After the 128 flights
    |t * sigma - table[m]| <= 0.001 * table[m]: half of the margin.  (The fma is restated as the fp64 product -- exact: 48 bits -- plus t
    rounded to fp64, then to fp32: it can differ from a true fma by a double rounding, 2^-29 of an ulp on average, nothing at this scale.)
    measured, largest |t * sigma - table| / table: 1.009e-6 (sigma 0.3), 1.019e-6 (0.74), 1.014e-6 (0.92)"""
    states = margin_states(table)
    assert states.size == BLOCK and np.unique(states).size == BLOCK
    inv = np.float64(np.float32(1.0) / np.float32(sigma))
    r = ref.float_construct(states)
    t = np.zeros(BLOCK, np.float32)
    term = spec_log_term(orc)
    for _ in range(128):
        u = ref.random1(r)
        t = (term(u).astype(np.float64) * inv + t.astype(np.float64)).astype(np.float32)
        r = ref.random1(u)
    want = table[states].astype(np.float64)
    err = np.abs(t.astype(np.float64) * np.float64(np.float32(sigma)) - want)
    pos = want > 0.0
    print("sigma %g: largest |t * sigma - table| / table = %.3e" % (sigma, (err[pos] / want[pos]).max()))
    assert (err <= 0.001 * want).all()
    assert int((~pos).sum()) == 1                             # state 0: both are 0


# ------------------------------------------------------------------------------------------------------------------ the checks bite
WRONG_CHAINS = {
    "every draw a flight": dict(every_draw_a_flight=True),
    "the chain started one draw late": dict(start_one_draw_late=True),
    "127 flights": dict(flights=127),
}


@pytest.mark.parametrize("wrong", sorted(WRONG_CHAINS))
def test_the_table_check_rejects_a_wrong_chain(orc, table, wrong):
    """named case: the first 2^16 states (state 0 among them, whose entry every chain gets right)"""
    got = ref.walk_sum(BLOCKS["first"], spec_log_term(orc), np.float32, **WRONG_CHAINS[wrong])
    assert got[0] == 0.0
    with pytest.raises(AssertionError, match="entries differ"):
        ref.check_table(got, table[BLOCKS["first"]])


class SelectionModel:
    """launch_flight_select restated on numpy buffers (9 words; 2^18 + 2 words, both pre-filled with the sentinel), right or with one defect"""

    def __init__(self, table, defect=None):
        self.table, self.defect = table, defect
        self.fresh()

    def fresh(self):
        self.sel = np.full(9, SENTINEL, np.uint32)
        self.bits = np.full(ref.N_WORDS + 2, SENTINEL, np.uint32)

    def run(self, lam, fresh=True):
        if fresh:
            self.fresh()
        if self.defect != "a count that is not reset between calls":
            self.sel[:] = 0                                   # the memset in front of the kernel
        with np.errstate(invalid="ignore"):
            capped = ~(self.table >= np.float32(lam)) if self.defect == ">= for >" else ~(self.table > np.float32(lam))
        words = np.packbits(capped, bitorder="little").view("<u4").astype(np.uint32)
        if self.defect == "bits most-significant-first":
            words = np.packbits(capped, bitorder="big").view(">u4").astype(np.uint32)
        if self.defect == "the upper ballot half written to word + 2":
            self.bits[2:ref.N_WORDS + 2:2] = words[1::2]      # one wave per 64 states: its upper half lands two words on ...
            self.bits[0:ref.N_WORDS:2] = words[0::2]          # ... where the next wave's lower half goes
        else:
            self.bits[:ref.N_WORDS] = words
        states = np.nonzero(capped)[0].astype(np.uint32)      # (the device's order is whatever the atomics gave: here ascending)
        listed = states[:-1] if self.defect == "a list that omits its last entry" else states
        for m in listed[:ref.LIST_MAX + 1]:
            k = int(self.sel[0])
            self.sel[0] = np.uint32((k + 1) & 0xFFFFFFFF)
            if k < ref.LIST_MAX:
                self.sel[1 + k] = m
        rest = states.size - min(listed.size, ref.LIST_MAX + 1)
        self.sel[0] = np.uint32((int(self.sel[0]) + rest) & 0xFFFFFFFF)
        return int(self.sel[0]), self.sel[1:].copy(), self.bits[:ref.N_WORDS].copy(), self.bits[ref.N_WORDS:].copy()


def check_every_lambda(model, table, only=None):
    for lam, _ in ref.LAMBDAS:
        if only is None or lam == only or (lam != lam and only != only):
            ref.check_selection(table, lam, *model.run(lam), SENTINEL)


def check_reuse(model, table):
    """97.4 and then 70.0 on the same buffers: nothing stale may remain"""
    model.run(97.4)
    ref.check_selection(table, 70.0, *model.run(70.0, fresh=False), SENTINEL)


def test_the_selection_checks_accept_the_right_selection(table):
    model = SelectionModel(table)
    check_every_lambda(model, table)
    check_reuse(model, table)


# defect -> (the case that must reject it, what the rejection says)
WRONG_SELECTIONS = {
    ">= for >": (float(np.float32(70.03356170654297)), "count 1, reference 2"),                # a lambda equal to a table value
    "bits most-significant-first": (0.0, "bit words differ, the first is word 0: 0x80000000, reference 0x1"),
    "the upper ballot half written to word + 2": (100.0, "bit words differ"),
    "a list that omits its last entry": (80.0, "the list repeats a state"),
    "a count that is not reset between calls": ("reuse", "count [0-9]+, reference 1"),
}


@pytest.mark.parametrize("defect", sorted(WRONG_SELECTIONS))
def test_the_selection_checks_reject_a_wrong_selection(table, defect):
    case, message = WRONG_SELECTIONS[defect]
    model = SelectionModel(table, defect)
    with pytest.raises(AssertionError, match=message):
        if case == "reuse":
            check_reuse(model, table)
        else:
            check_every_lambda(model, table, only=case)
    if defect == "the upper ballot half written to word + 2":      # ... and the slack words catch the last wave's on a table of zeros
        with pytest.raises(AssertionError, match="bit words differ|behind the bit table"):
            check_every_lambda(model, table, only=300.0)
