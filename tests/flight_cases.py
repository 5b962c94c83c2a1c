"""What tests/test_flight_reference_cpu.py and tests/test_gpu_flight_states.py share: the oracle's free-flight table (computed once per
session), the diagonal view of an empty box in which ordinary RNG states run into DeltaTrack's cap, the frames that pin a pixel into each
of the seven small capped states, and the oracle's frames of that view (computed once each)."""
import functools
import math

import numpy as np

import flight_reference as ref
import rng_search
from nrc_hpm_renderer_amd import parallel, scene as sc

W, H = 256, 144            # the smallest frame at which the diagonal view keeps every chord above 95 % of the box diagonal
MC_PATH_LENGTH = 8


@functools.lru_cache(maxsize=None)
def oracle():
    from oracle import Oracle
    return Oracle()


@functools.lru_cache(maxsize=None)
def oracle_table():
    """orc_flight_table over all 2^23 states (about 2 s on 16 threads), read-only"""
    t = oracle().flight_table(threads=16)
    t.setflags(write=False)
    return t


# ---------------------------------------------------------------------------------------------------------------- scene and view
# An all-zero 16^3 volume: the box is 62.07^3, its diagonal 107.5, every tile of every view is one the mask rejects.  The eye stands on the
# diagonal, 15 % outside the corner, and looks along it through 20 degrees: every chord is nearly the whole diagonal, so at density factor
# rho a pixel scatters iff its state's table entry is below about rho * 107.5.
def scene(density_factor):
    s = sc.make_scene(np.zeros((16, 16, 16), np.uint8), scene_id=4, env=sc.procedural_sky(32, 16))
    s["density_factor"] = float(density_factor)
    return s


def camera():
    pos = 1.15 * np.asarray(sc.volume_size((16, 16, 16)), np.float64) / 2.0
    return sc.make_camera(pos=pos, view_dir=-pos, aspect=W / H, fovy=math.radians(20.0))


# density factor -> skip_lambda: 0.74 -> 80.08 (the list holds exactly the eight states up to 70.85; the ninth entry is 82.64),
# 0.765 -> 82.79 (nine states: one bit per state), 0.92 -> 99.56 (30 000 states), 0.93 -> 100.64 (above 100: the mask is not applied)
RHO_LIST, RHO_NINE, RHO_BITS, RHO_OFF = 0.74, 0.765, 0.92, 0.93

# state -> (pixel (x, y), frame random): `python tests/rng_search.py state <state> 256 144 <x> <y>`.  (128, 72) is the pixel of the central
# ray; it has no frame random for states 2282633 and 1922895, whose frames pin a neighbour.
PINNED = {
    2282633: ((128, 73), [0.5651434659957886, 0.04615384712815285, 0.75, 0.125]),
    1922895: ((129, 72), [0.6573262214660645, 0.015384615398943424, 0.75, 0.125]),
    2160624: ((128, 72), [0.3636997938156128, 0.015384615398943424, 0.75, 0.125]),
    7178807: ((128, 72), [0.350913405418396, 0.015384615398943424, 0.75, 0.125]),
    1547426: ((128, 72), [0.5381089448928833, 0.04615384712815285, 0.75, 0.125]),
    5279004: ((128, 72), [0.28246212005615234, 0.015384615398943424, 0.75, 0.125]),
    5527704: ((128, 72), [0.8901646137237549, 0.015384615398943424, 0.75, 0.125]),
}
assert sorted(PINNED) == sorted(ref.SMALL_STATES)

SCALE_FRAMES, SCALE_SEED = 64, 11
TILED_RANK, TILED_WORLD, TILED_FRAME = 3, 8, 8      # the frame that also runs as column tile 3 of 8: one of its three scattered pixels lies there


def scale_frame_randoms():
    return np.asarray(sc.frame_randoms(SCALE_FRAMES, seed=SCALE_SEED), np.float32)


def frame_states(frame_random, columns=None):
    """the RNG state (mantissa) every pixel starts the frame in, [H][columns] (numpy restatement of InitRandom: tests/rng_search.py)"""
    gx, y = np.meshgrid(np.arange(W) if columns is None else np.asarray(columns), np.arange(H))
    r = rng_search.init_random(gx.astype(np.float32), y.astype(np.float32), W, H, frame_random)
    return (r + np.float32(1.0)).view(np.uint32) & np.uint32(0x7FFFFF)


def tile_columns():
    return parallel.rank_columns(TILED_RANK, TILED_WORLD, W)


@functools.lru_cache(maxsize=None)
def _oracle_frame(density_factor, frame_random):
    s, cam = scene(density_factor), camera()
    o = oracle().nrc_gen_rays(s, cam, W, H, 1, 0.0, list(frame_random), threads=8)
    mc, _, _ = oracle().mc_render(s, cam, W, H, MC_PATH_LENGTH, list(frame_random), threads=8)
    out = dict(primary=o["primary"], info=o["info"], infer_input=o["infer_input"], mc=mc, n_fetch=o["n_fetch"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def oracle_frame(density_factor, frame_random):
    """the oracle's NRC primary / info / infer_input buffers and MC image of one frame of the view (25 ms each on 8 threads; cached)"""
    return _oracle_frame(float(density_factor), tuple(float(x) for x in frame_random))
