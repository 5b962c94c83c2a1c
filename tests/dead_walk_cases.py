"""Scenes of tests/test_gpu_dead_walks.py: media on which ratio tracking's transmittance reaches exactly 0 long before a walk ends.

With density_factor 0.6 the factor of a collision at byte 255 is fma(-0.6f * (255 * (1 / 255.f)), 1 / 0.6f, 1) = -1.59e-8 (negative:
the sign of a zero transmittance alternates in the reference), at byte 254 it is 3.92e-3.  Six collisions at 255 or about nineteen at 254
take the product to 0 in fp32.  The 32^3 volumes fill the default box of 62.07^3: a voxel is 1.94 long and the majorant's mean free path
1 / 0.6 = 1.67, so a shadow walk along the light axis (+z) through the whole box has some twenty collisions before it leaves."""
import numpy as np

FRAME_RANDOM = [0.25, 0.5, 0.75, 1.0]
W = H = 64
N = 32
SCENES = ("all255", "all254", "split", "cloud")


def volume(name, cloud16):
    if name == "all255":
        return np.full((N, N, N), 255, np.uint8)
    if name == "all254":
        return np.full((N, N, N), 254, np.uint8)
    if name == "split":
        # [z][y][x]; the directional light's shadow rays travel towards +z: walks that start among bytes 1..64 are alive until they cross
        # into the saturated half, beside walks that start inside it
        vol = np.random.default_rng(5).integers(1, 65, (N, N, N)).astype(np.uint8)
        vol[N // 2:] = 255
        return vol
    if name == "thin":                       # bytes <= 64: a factor is at least 1 - 64 / 255, and 0.749^128 = 8.6e-17 is far from 0
        return np.random.default_rng(6).integers(0, 65, (N, N, N)).astype(np.uint8)
    assert name == "cloud"
    return cloud16


def make_case(sc, name, cloud16):
    """(scene, camera).  The saturated media are lit by the directional light alone (what the all-255 scene's zero pixels need: a
    sky sample that leaves through the near face survives); the split medium and the cloud by all three lights, so that
    trace_dir_light, trace_point_light and sample_env all meet dead walks."""
    vol = volume(name, cloud16)
    if name in ("all255", "all254", "thin"):
        scene = sc.make_scene(vol, scene_id=0)
    else:
        scene = sc.make_scene(vol, scene_id=4, env=sc.procedural_sky(32, 16))
        scene["point_light_strength"] = 64.0
        scene["point_light_pos"] = np.array([3.0, -2.0, 5.0], np.float32)
    return scene, sc.make_camera(aspect=W / H)
