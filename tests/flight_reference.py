"""The capped-state side of the empty-space skip, restated in plain numpy (imports neither the product nor the oracle).

A camera wave may leave a tile unwalked only when no pixel of it can run into DeltaTrack's cap of 128 collisions in empty space
(path_trace.glsl:161-173).  Whether a pixel can is a function of its RNG state alone:

    table[m]   the distance, in units of 1 / sigma_max, that a walk which starts in state float_construct(m) and rejects every collision
               has covered after 128 free flights.  Draws alternate flight, acceptance (path_trace.glsl:163-170); a flight adds -log(1 - u).
    selection  the states with not (table[m] > lambda), lambda = skip_lambda(scene): their count, the first eight, and one bit per state.

table64 is that table with fp64 sums and log1p; the device's (k_flight_table) and the oracle's (orc_flight_table) sum in fp32 with the math
spec's log.  check_table / check_selection are the assertions tests/test_gpu_flight_states.py makes on the device's output;
tests/test_flight_reference_cpu.py runs the same functions on deliberately wrong tables and selections, which they must reject."""
import numpy as np

N_STATES = 1 << 23
N_WORDS = N_STATES // 32
LIST_MAX = 8
M23 = np.uint32(0x7FFFFF)


def hash1(x):
    """random.glsl:24-32"""
    x = np.asarray(x, np.uint32)
    with np.errstate(over="ignore"):
        x = x + (x << np.uint32(10))
        x = x ^ (x >> np.uint32(6))
        x = x + (x << np.uint32(3))
        x = x ^ (x >> np.uint32(11))
        x = x + (x << np.uint32(15))
    return x


def float_construct(m):
    """random.glsl:41-51: the float in [0, 1) with mantissa m"""
    return ((np.asarray(m, np.uint32) & M23) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)


def random1(x):
    """random.glsl:54"""
    return float_construct(hash1(np.ascontiguousarray(x, np.float32).view(np.uint32)))


def walk_sum(states, term, dtype, flights=128, every_draw_a_flight=False, start_one_draw_late=False):
    """sum over `flights` free flights of term(u) (an array of `dtype`), u the flight draws of walks starting in `states`.  The two flags
    and a flights other than 128 are the WRONG chains tests/test_flight_reference_cpu.py rejects."""
    r = float_construct(np.asarray(states, np.uint32))
    if start_one_draw_late:
        r = random1(r)
    d = np.zeros(r.shape, dtype)
    for _ in range(flights):
        u = random1(r)                       # the flight's draw
        d = (d + term(u)).astype(dtype)
        r = u if every_draw_a_flight else random1(u)      # the acceptance draw: made, compared with density 0, lost
    return d


def table64(states):
    """the table entries of `states` (mantissas) with -log1p(-u) summed in fp64"""
    return walk_sum(states, lambda u: -np.log1p(-u.astype(np.float64)), np.float64)


# per entry, fp32 table against table64: 128 additions, each rounding a sum below 256 (half an ulp: 2^-17), plus 128 logs of magnitude below
# 16 (-log(2^-23) = 15.94), each within one ulp (2^-20) of the true value (tests/test_oracle_math.py::test_math_spec_accuracy)
TABLE_BOUND = 128 * (2.0 ** -17 + 2.0 ** -20)


def select(table, lam):
    """(count, the selected states in ascending order, the N_WORDS bit words): state m is selected iff not (table[m] > lambda) in fp32 --
    equality selects, and so does a NaN on either side; bit (m & 31) of word (m >> 5) is set for a selected state"""
    table = np.asarray(table, np.float32)
    assert table.shape == (N_STATES,)
    with np.errstate(invalid="ignore"):
        capped = ~(table > np.float32(lam))
    bits = np.packbits(capped, bitorder="little").view("<u4").astype(np.uint32)
    states = np.nonzero(capped)[0].astype(np.uint32)
    return int(states.size), states, bits


def skip_lambda(scene):
    """the largest optical depth a ray of `scene` (scene.make_scene) can have, as skip_setup computes it: fp64 arithmetic on the fp32 density
    factor and box size the renderer holds.  The mask is applied when this is at most 100; the kernel compares with float32 of it."""
    size = np.asarray(scene["size"], np.float32).astype(np.float64)
    diag = float(np.sqrt(size[0] * size[0] + size[1] * size[1] + size[2] * size[2]))
    return float(np.float32(scene["density_factor"])) * (diag + 0.5) * 1.002


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def check_table(got, want):
    """the table under test equals the reference bit for bit"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, "%d of %d entries differ, the first at index %d: %r, reference %r" % (bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def check_selection(table, lam, count, lst, bits, slack, sentinel):
    """what a selection at `lam` (count; lst: the LIST_MAX words behind the count; bits: N_WORDS words; slack: the two words behind them,
    pre-filled with `sentinel`) has to be for `table`"""
    n, states, ref_bits = select(table, lam)
    assert count == n, "lambda %r: count %d, reference %d" % (lam, count, n)
    head = np.asarray(lst, np.uint32)[:min(n, LIST_MAX)]
    assert np.unique(head).size == head.size, "lambda %r: the list repeats a state: %r" % (lam, head.tolist())
    assert np.isin(head, states).all(), "lambda %r: the list %r holds states outside the selection" % (lam, head.tolist())
    if n <= LIST_MAX:
        assert sorted(head.tolist()) == states.tolist(), "lambda %r: list %r, reference %r" % (lam, sorted(head.tolist()), states.tolist())
    bits = np.asarray(bits, np.uint32)
    assert bits.shape == (N_WORDS,)
    bad = np.nonzero(bits != ref_bits)[0]
    assert bad.size == 0, "lambda %r: %d bit words differ, the first is word %d: %#x, reference %#x" % (lam, bad.size, bad[0], int(bits[bad[0]]), int(ref_bits[bad[0]]))
    assert np.asarray(slack, np.uint32).tolist() == [sentinel, sentinel], "lambda %r: the words behind the bit table were written: %r" % (lam, slack)


# the lambdas of the selection test and what each is there for (the table values among them are entries of the table: equality selects)
LAMBDAS = [
    (-1.0, "nothing selected"),
    (0.0, "state 0 alone"),
    (70.0, "below the smallest non-zero entry"),
    (float(np.float32(70.03356170654297)), "equality selects"),
    (float(np.float32(70.79169464111328)), "a triple tie"),
    (80.0, "list exactly full"),
    (float(np.float32(82.63516998291016)), "9 states: one more than the list holds"),
    (97.4, "bits mode"),
    (100.0, "the largest lambda skip_setup accepts"),
    (300.0, "every state"),
    (float("inf"), "every state"),
    (float("nan"), "not (d > NaN) selects every state: the conservative answer"),
]
# the seven non-zero states below the ninth smallest entry (82.63517), ascending by their table value (70.03 .. 70.85)
SMALL_STATES = [2282633, 1922895, 2160624, 7178807, 1547426, 5279004, 5527704]
