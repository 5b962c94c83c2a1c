"""Scenes of tests/test_gpu_trip_edges.py and tests/test_trip_edge_cases_cpu.py: media that take the tracking loops to the places where
their per-trip bookkeeping is thinnest in the other suites ("Trip overhead").

  cap          16^3 voxels of byte 0, density factor 8: a chord through the box of 62.07^3 holds some five hundred majorant collisions and
               accepts none, so a camera walk ends on the cap of 128 collisions (path_trace.glsl:161) -- the only way a pixel of an empty
               medium can scatter -- and its shadow and sky walks run on in the same medium until they leave or are capped too.
  late_accept  16^3 voxels of byte 1, the same factor: a collision is accepted with probability 1 / 255, so camera walks end by acceptance
               at every collision index up to the cap, odd ones (the first collision of a trip) and even ones, the 127th and 128th included.
  odd_box      20 x 12 x 36 voxels (x, y, z): no power of two and no multiple of the 8-voxel occupancy cell.  Seeded random bytes, whole
               8^3 cells zeroed at random: occupied and empty cells are neighbours and the cells at the far faces are cut by the volume.

late_accept's certificate restates the camera walk's acceptance chain in numpy: the draws alternate free flight, acceptance
(path_trace.glsl:163-170), and in a medium of one byte the acceptance test compares every acceptance draw with ONE number."""
import numpy as np

import far_cut_reference as fc
import flight_reference as fl
import skip_reference as ref

W = H = 64
CASES = ("cap", "late_accept", "odd_box")
DENSITY_FACTOR = 8.0
FRAME_RANDOM = {"cap": [0.25, 0.5, 0.75, 1.0], "late_accept": [0.25, 0.5, 0.75, 1.0], "odd_box": [0.25, 0.5, 0.75, 1.0]}
ODD_DIMS = (20, 12, 36)         # x, y, z
CELL = 8


def volume(name):
    """uint8 [z][y][x]"""
    if name == "cap":
        return np.zeros((16, 16, 16), np.uint8)
    if name == "late_accept":
        return np.ones((16, 16, 16), np.uint8)
    assert name == "odd_box"
    nx, ny, nz = ODD_DIMS
    rng = np.random.default_rng(11)
    vol = rng.integers(0, 256, (nz, ny, nx)).astype(np.uint8)
    gz, gy, gx = -(-nz // CELL), -(-ny // CELL), -(-nx // CELL)
    empty = rng.random((gz, gy, gx)) < 0.4
    for cz, cy, cx in np.argwhere(empty):
        vol[cz * CELL:(cz + 1) * CELL, cy * CELL:(cy + 1) * CELL, cx * CELL:(cx + 1) * CELL] = 0
    return vol


def make_case(sc, name):
    """(scene, camera): all three lights, so that trace_dir_light, trace_point_light and sample_env all walk the medium"""
    scene = sc.make_scene(volume(name), scene_id=4, env=sc.procedural_sky(32, 16))
    scene["point_light_strength"] = 64.0
    scene["point_light_pos"] = np.array([3.0, -2.0, 5.0], np.float32)
    if name in ("cap", "late_accept"):
        scene["density_factor"] = float(np.float32(DENSITY_FACTOR))
    return scene, sc.make_camera(aspect=W / H)


def enters_box(scene, cam):
    """bool [H][W]: the pixel's camera ray meets the volume's box (an fp64 slab test)"""
    half = 0.5 * np.asarray(scene["size"], np.float32).astype(np.float64)
    origin, dirs = ref.camera_rays(cam, W, H, np.arange(W))
    return np.isfinite(fc.exit_distances(origin, dirs, np.concatenate([-half, half])[None, :])).reshape(H, W)


def cells(vol):
    """per 8^3 cell of the volume, [gz][gy][gx]: (occupied: holds a non-zero voxel; cut: the volume ends inside it)"""
    nz, ny, nx = vol.shape
    gz, gy, gx = -(-nz // CELL), -(-ny // CELL), -(-nx // CELL)
    pad = np.zeros((gz * CELL, gy * CELL, gx * CELL), np.uint8)
    pad[:nz, :ny, :nx] = vol
    occupied = pad.reshape(gz, CELL, gy, CELL, gx, CELL).max(axis=(1, 3, 5)) != 0
    cz, cy, cx = np.meshgrid(np.arange(gz), np.arange(gy), np.arange(gx), indexing="ij")
    cut = ((cz + 1) * CELL > nz) | ((cy + 1) * CELL > ny) | ((cx + 1) * CELL > nx)
    return occupied, cut


def acceptance_probability(scene, byte):
    """what DeltaTrack compares an acceptance draw with at a voxel of `byte`: getDensity() * (1 / factor), in fp32 (volume.glsl:31-39,
    path_trace.glsl:154,168)"""
    f = np.float32(scene["density_factor"])
    dens = f * (np.float32(byte) * (np.float32(1.0) / np.float32(255.0)))
    return np.float32(dens * (np.float32(1.0) / f))


def first_acceptance(orc, scene, frame_random, byte):
    """int [H][W]: the collision at which the pixel's first camera walk accepts in a medium of `byte` everywhere that never ends, 1 .. 128;
    0: none of the 128 is accepted.  The pixel's RNG state is init_random(x / W, y / H) (the oracle's: orc.rng_kat), the chain and the
    comparison are restated here."""
    p = acceptance_probability(scene, byte)
    inv_w, inv_h = np.float32(1.0) / np.float32(W), np.float32(1.0) / np.float32(H)
    state = np.zeros((H, W), np.float32)
    for y in range(H):
        for x in range(W):
            state[y, x] = orc.rng_kat(float(np.float32(x) * inv_w), float(np.float32(y) * inv_h), frame_random, 0)[0]
    first = np.zeros((H, W), np.int64)
    for k in range(1, 129):
        state = fl.random1(state)            # the free flight's draw
        state = fl.random1(state)            # the acceptance draw
        first = np.where((first == 0) & (p > state), k, first)
    return first


def certified_acceptances(orc, scene, cam, frame_random, byte=1):
    """int [H][W]: the collision at which the pixel's first camera walk ENDED BY ACCEPTANCE, 0 where that is not certain.  Certain: the
    pixel scattered, the oracle's walk drew exactly as many free flights as the restated chain needs to its first acceptance (so it did
    not leave the box before), and that number is not 0."""
    lengths, info = orc.nrc_walk_lengths(scene, cam, W, H, 1, 0.0, frame_random, walks_per_pixel=1, threads=8)
    first = first_acceptance(orc, scene, frame_random, byte)
    return np.where((info == 1) & (first > 0) & (lengths[..., 0] == first), first, 0), first, lengths[..., 0], info
