"""tests/train_grid_cases.py without a GPU: the table reaches what each case is there for (asserted from the oracle's gen_rays frames, not
from the table's comments), the oracle's prep_train does not depend on its thread count, and the oracle's ring equals the independent
ring model."""
import numpy as np
import pytest

import train_grid_cases as tc


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scattered(name, case, o):
    """per train index: scattered or not, as prep_train_rays decides it (a train pixel outside the frame reads 0)"""
    y, x, inside = tc.train_pixels(tc.case_grid(case), case["W"], case["H"])
    s = np.zeros(len(y), bool)
    s[inside] = o["info"][y[inside], x[inside]] == 1.0
    return s, inside


@pytest.mark.parametrize("name", list(tc.CASES))
def test_the_table_reaches_what_it_says(orc, name):
    case = tc.CASES[name]
    g = tc.case_grid(case)
    T = case["count"] << case["log2"]
    tw, th, rs = g["tw"], g["th"], g["ring_size"]
    assert (tw, th) == case["grid"] and (g["x_dist"], g["y_dist"]) == case["dist"] and tw * th == T
    per = (T + tc.SCAN_THREADS - 1) // tc.SCAN_THREADS
    assert per == case["per"]
    if name in ("A", "A-tall", "Z", "B", "SQ", "C", "C1"):
        assert T % 128 != 0
    if name in ("A-tall", "B"):
        assert th % 8 != 0
    if name in ("A", "SQ", "C"):
        assert tw % 8 != 0
    if name in ("A-tall", "SQ", "TALL2"):
        assert case["W"] <= case["H"] and tw < th
    if name == "TALL2":
        assert g["x_dist"] != g["y_dist"]
    if name in ("D", "F"):                       # scan threads whose run is empty, behind one that is full
        assert per >= 2 and (T + per - 1) // per < tc.SCAN_THREADS
    if name == "G":
        assert per > 64
    assert (rs == 0) == (name == "Z")
    if name == "F":
        assert rs > T
    gens = tc.gen_rays_of(orc, name, case)
    frames = tc.model_frames(name)
    for o, m in zip(gens, frames):
        s, inside = scattered(name, case, o)
        assert s.any() and (~s & inside).any()               # both kinds in every frame
        assert (not inside.all()) == (name in ("SQ", "C", "D"))
        if per >= 2:                                          # a scan thread's run holds both kinds: the run-local ranks are exercised
            runs = s[:T // per * per].reshape(-1, per)
            assert (runs.any(axis=1) & ~runs.all(axis=1)).any()
        if name == "E":
            assert m["n_push"] > rs
        if rs:
            assert m["n_push"] == int(s.sum()) and m["n_pop"] == T - m["n_push"]
    if name in ("C", "C1", "E"):                              # a frame starts with a head or tail that clear.comp has to wrap
        assert any((m["before"] >= rs).any() for m in frames)
    if name == "C1":
        assert any(m["before"][0] >= rs for m in frames)


def test_the_small_ring_setup_overflows_its_ring(orc):
    case = tc.SMALL_RING
    g = tc.case_grid(case)
    assert g == dict(tw=32, th=32, x_dist=4, y_dist=2, ring_size=256)
    for o in tc.gen_rays_of(orc, "small-ring", case):
        s, _ = scattered("small-ring", case, o)
        assert s.sum() > g["ring_size"]


@pytest.mark.parametrize("name", ["E", "small-ring"])
def test_prep_train_does_not_depend_on_the_thread_count(orc, name):
    """a frame that pushes more entries than the ring holds writes slots more than once: the last push in linear train-index order wins,
    whichever thread traced its row -- 30 runs at threads = 8 equal the run at threads = 1 bit for bit"""
    case = tc.SMALL_RING if name == "small-ring" else tc.CASES[name]
    spp, length = case.get("spp", 1), case.get("length", 1)
    gens = tc.gen_rays_of(orc, name, case)
    want = tc.prep_train_frames(orc, case, gens, spp, length, 1)
    for run in range(30):
        got = tc.prep_train_frames(orc, case, gens, spp, length, 8)
        for f, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a["head_tail"], b["head_tail"]), (run, f)
            for k in ("tin", "tgt", "ring"):
                assert np.array_equal(bits(a[k]), bits(b[k])), (run, f, k)


@pytest.mark.parametrize("name", list(tc.CASES))
def test_the_oracles_ring_is_the_ring_models(orc, name):
    gens, frames = tc.oracle_frames(orc, name)
    for f, (a, m) in enumerate(zip(frames, tc.model_frames(name))):
        assert np.array_equal(a["head_tail"], m["head_tail"]), f
        assert np.array_equal(bits(a["ring"]), bits(m["ring"])), f
    if name == "Z":
        ring, head_tail = tc.new_ring(tc.case_grid(tc.CASES[name]))
        assert np.array_equal(frames[-1]["ring"], ring) and not frames[-1]["head_tail"].any()
        assert not any(f["tin"].any() or f["tgt"].any() for f in frames)
