"""Sparse volume keys (nrc_renderer_set_volume_key_bricks), the parts that need no GPU: scene.volumes_to_key_bricks and its inverse, the
byte formula, the CLI's --sparse-keys rules, the device-free host logic (csrc/nrc_volume_key_bricks.hpp, which
tests/cpp/volume_key_bricks_main.cpp drives on the CPU under ASan + UBSan), the new entry points in the header and both mirrors -- and that
the key sequence the GPU tests use exercises what the feature is about."""
import argparse
import os
import re
import subprocess

import numpy as np
import pytest

from key_bricks_common import N_KEYS, SHAPES, cells_of, key_bricks_of, keys_of, times_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nrc-hpm-renderer_amd", "csrc")
HEADER = "nrc_volume_key_bricks.hpp"


# ---------------------------------------------------------------------------------------------------------------- helper and bytes
@pytest.mark.parametrize("name", list(SHAPES))
def test_volumes_to_key_bricks_round_trips(sc, cloud16, name):
    shape = SHAPES[name]
    keys = keys_of(cloud16, shape)
    counts, origins, bricks = key_bricks_of(sc, cloud16, shape)
    assert counts.dtype == np.uint32 and counts.shape == (N_KEYS,) and counts[2] == 0      # (the all-zero key: no brick)
    assert origins.dtype == np.int32 and origins.shape == (int(counts.sum()), 3) and origins.flags.c_contiguous
    assert bricks.dtype == np.uint8 and bricks.shape == (int(counts.sum()), 8, 8, 8) and bricks.flags.c_contiguous
    first = 0
    for k in range(N_KEYS):      # every key's slice is that key's own list
        o, b = sc.volume_to_bricks(keys[k])
        assert np.array_equal(origins[first:first + len(o)], o) and np.array_equal(bricks[first:first + len(o)], b)
        first += len(o)
    back = sc.key_bricks_to_volumes(counts, origins, bricks, shape)
    assert back.dtype == np.uint8 and back.flags.c_contiguous and np.array_equal(back, keys)
    f32 = sc.volumes_to_key_bricks([k.astype(np.float32) / np.float32(255) for k in keys[:2]])
    assert f32[2].dtype == np.float32 and np.array_equal(f32[0], counts[:2]) and np.array_equal(f32[1], origins[:int(counts[:2].sum())])


def test_key_brick_helpers_reject_what_they_cannot_use(sc):
    with pytest.raises(ValueError):
        sc.volumes_to_key_bricks([])
    with pytest.raises(ValueError):
        sc.volumes_to_key_bricks([np.zeros((8, 8, 8), np.uint8), np.zeros((8, 8, 9), np.uint8)])
    with pytest.raises(ValueError):
        sc.volumes_to_key_bricks([np.zeros((8, 8, 8), np.uint8), np.zeros((8, 8, 8), np.float32)])
    o, b = np.zeros((2, 3), np.int32), np.zeros((2, 8, 8, 8), np.uint8)
    with pytest.raises(ValueError):
        sc.key_bricks_to_volumes([1, 2], o, b, (8, 8, 8))
    with pytest.raises(ValueError):      # a bad origin, as bricks_to_volume reports it
        sc.key_bricks_to_volumes([1, 1], np.array([[0, 0, 0], [8, 0, 0]], np.int32), b, (8, 8, 8))
    got = sc.key_bricks_to_volumes([1, 1], np.array([[0, 0, 0], [8, 0, 0]], np.int32), b, (8, 8, 8), ignore_invalid=True)
    assert got.shape == (2, 8, 8, 8)
    # of two bricks with one origin inside a key the last wins; the same origin in another key is that key's
    b2 = np.stack([np.full((8, 8, 8), v, np.uint8) for v in (1, 2, 3)])
    got = sc.key_bricks_to_volumes([2, 1], np.zeros((3, 3), np.int32), b2, (8, 8, 8))
    assert (got[0] == 2).all() and (got[1] == 3).all()


def test_the_byte_formula_is_below_the_dense_bytes_for_the_fixture_cloud(sc, cloud16):
    """keys of the fixture's own dims (cloud, a rolled copy, the cloud upside down): 512 * bricks + 4 * n_keys * cells against n_keys * voxels"""
    keys = np.stack([cloud16, np.roll(cloud16, (30, 20, -50), axis=(0, 1, 2)), cloud16[::-1]])
    counts, origins, bricks = sc.volumes_to_key_bricks(keys)
    nz, ny, nx = cloud16.shape
    cells = ((nz + 7) // 8) * ((ny + 7) // 8) * ((nx + 7) // 8)
    held = sc.key_brick_bytes(counts, cloud16.shape)
    assert counts[0] == 1233 and cells == 20 * 11 * 16
    assert held == 512 * int(counts.sum()) + 4 * 3 * cells == bricks.nbytes + 4 * 3 * cells
    dense = keys.nbytes
    assert dense == 3 * nz * ny * nx
    assert held < dense, (held, dense)
    assert 512 * 1233 / cloud16.size < 0.39      # (the fixture: 38 % of its dense bytes as bricks)
    print("fixture keys: %d bytes as bricks, %d dense (%.1f %%)" % (held, dense, 100.0 * held / dense))


# ---------------------------------------------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_inputs_are_not_vacuous(sc, cloud16, name):
    """on the CPU, before any GPU call: over the tested pairs with 0 < W < 256 there is an 8^3 cell with a brick in key a only, one in b
    only, one in both and one in neither; a one-sided voxel whose in-between differs from its key (blending against 0 is not a copy); and a
    cell that is occupied in a key and empty in the in-between (the occupancy has to follow q)"""
    shape = SHAPES[name]
    keys = keys_of(cloud16, shape)
    counts, _, _ = key_bricks_of(sc, cloud16, shape)
    for k in range(N_KEYS):      # (a key's bricks are its occupied cells)
        assert int(cells_of(keys[k]).sum()) == int(counts[k])
    seen = dict(a_only=0, b_only=0, both=0, neither=0)
    one_sided_differs = vanishes = 0
    for t in times_of(shape):
        i, W = sc.key_of_time(t, N_KEYS)
        if W in (0, 256):
            continue
        ca, cb = cells_of(keys[i]), cells_of(keys[i + 1])
        seen["a_only"] += int((ca & ~cb).sum())
        seen["b_only"] += int((~ca & cb).sum())
        seen["both"] += int((ca & cb).sum())
        seen["neither"] += int((~ca & ~cb).sum())
        q = sc.volume_at(keys, t)
        nz, ny, nx = shape
        up = lambda c: np.repeat(np.repeat(np.repeat(c, 8, 0), 8, 1), 8, 2)[:nz, :ny, :nx]      # noqa: E731  (cells -> voxels)
        only_a, only_b = up(ca & ~cb), up(~ca & cb)
        one_sided_differs += int(((q != keys[i]) & only_a).sum()) + int(((q != keys[i + 1]) & only_b).sum())
        vanishes += int(((ca | cb) & ~cells_of(q)).sum())
    assert min(seen.values()) >= 1, seen
    assert one_sided_differs >= 1
    assert vanishes >= 1


# ---------------------------------------------------------------------------------------------------------------- the device-free header
def test_the_header_compiles_without_rocm_and_the_library_depends_on_it():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-include", HEADER, "-x", "c++", os.devnull],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-4000:]
    code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, HEADER)).read())
    assert not re.search(r"hip|nccl|__device__|__host__", code, re.I)
    assert "nrc_common.hpp" not in code
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^KEY_BRICK_HDRS = " + re.escape(HEADER) + "$", makefile, re.M)
    assert re.search(r"^SRCS = [^\n]*\$\(KEY_BRICK_HDRS\)", makefile, re.M)      # among the build id's sources
    rule = re.search(r"^\$\(OUT\)/nrc_api\.o:([^\n]*)$", makefile, re.M)
    assert rule and "$(KEY_BRICK_HDRS)" in rule.group(1)
    assert '#include "%s"' % HEADER in open(os.path.join(CSRC, "nrc_api.hip")).read()


def test_the_host_logic_under_the_sanitizers():
    """tests/cpp/volume_key_bricks_main.cpp: its own main, built from the device-free header alone with ASan + UBSan (no recovery) and run
    directly: counts and offsets, the bytes held, origins that name key and brick, sizes that do not fit"""
    build = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "volume_key_bricks_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "volume_key_bricks_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out and "FAILED" not in out, out[-4000:]
    m = re.search(r"^volume_key_bricks: (\d+) checks, 0 failed$", out, re.M)
    assert m and int(m.group(1)) >= 50, out[-400:]      # (every CHECK of the program ran)


# ---------------------------------------------------------------------------------------------------------------- CLI
def _args(**kw):
    d = dict(orbit=None, frames=4, benchmark=False, vdb=None, gpus=1, export=None, animate=False, bricks=False, sparse_keys=False, time_scale=1.0)
    d.update(kw)
    return argparse.Namespace(**d)


def test_cli_sparse_keys_argument_rules():
    from nrc_hpm_renderer_amd import cli
    seq = ["a.vdb", "b.vdb", "c.vdb"]
    assert cli.check_animate_args(_args(orbit=4, vdb=seq, animate=True, sparse_keys=True)) is True
    assert cli.check_orbit_args(_args(orbit=4, vdb=seq, animate=True, sparse_keys=True)) == 4
    assert cli.check_animate_args(_args(orbit=4, vdb=seq, animate=True)) is True      # (dense keys: as before)
    with pytest.raises(SystemExit, match="--sparse-keys goes with --animate"):
        cli.check_animate_args(_args(orbit=4, vdb=seq, sparse_keys=True))
    with pytest.raises(SystemExit, match="--sparse-keys goes with --animate"):
        cli.check_animate_args(_args(sparse_keys=True))
    for bad in (dict(animate=True, sparse_keys=True), dict(animate=True, sparse_keys=True, orbit=4, vdb=["a.vdb"]),
                dict(animate=True, sparse_keys=True, vdb=seq)):      # --animate's own needs stay
        with pytest.raises(SystemExit, match="SkyRenderer ERROR"):
            cli.check_animate_args(_args(**bad))
    # --animate --bricks stays refused, with and without --sparse-keys: --bricks means stepping with SetVolumeBricks
    for extra in (dict(), dict(sparse_keys=True)):
        with pytest.raises(SystemExit, match="--animate and --bricks exclude each other"):
            cli.check_animate_args(_args(orbit=4, vdb=seq, animate=True, bricks=True, **extra))
    # the parser: a bad combination ends the run before anything touches the GPU (or a file)
    for argv in (["--sparse-keys"], ["--sparse-keys", "--vdb", "a.vdb", "b.vdb"], ["--sparse-keys", "--orbit", "4"],
                 ["--sparse-keys", "--bricks", "--vdb", "a.vdb", "b.vdb"], ["--animate", "--sparse-keys"],
                 ["--animate", "--sparse-keys", "--orbit", "4", "--vdb", "a.vdb", "b.vdb", "--bricks"]):
        with pytest.raises(SystemExit, match="SkyRenderer ERROR"):
            cli.main(argv)
    assert "--sparse-keys" in cli.__doc__ and "SetVolumeKeyBricks" in cli.__doc__


# ---------------------------------------------------------------------------------------------------------------- the surface
NEW_SYMBOLS = ["nrc_renderer_set_volume_key_bricks", "nrc_mc_renderer_set_volume_key_bricks", "nrc_renderer_volume_key_bytes",
               "nrc_mc_renderer_volume_key_bytes"]


def test_new_symbols_are_in_the_header_and_both_mirrors(api):
    header = open(os.path.join(ROOT, "include", "nrc_hpm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    hpp = open(os.path.join(ROOT, "include", "nrc_hpm.hpp")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), s
        assert s + "(" in hpp, s
        assert s in api.ABI_SYMBOLS, s
        assert hasattr(api.load_library(), s), s
    assert re.search(r"int nrc_renderer_set_volume_key_bricks\(nrc_renderer_t\* r, const uint32_t\* key_counts, const int32_t\* origins, const void\* bricks, "
                     r"uint32_t n_keys,\s*int format, int on_device\);", code)
    assert re.search(r"int nrc_mc_renderer_set_volume_key_bricks\(nrc_mc_renderer_t\* r, const uint32_t\* key_counts, const int32_t\* origins, "
                     r"const void\* bricks, uint32_t n_keys,\s*int format, int on_device\);", code)
    assert re.search(r"size_t nrc_renderer_volume_key_bytes\(nrc_renderer_t\* r\);", code)
    assert re.search(r"size_t nrc_mc_renderer_volume_key_bytes\(nrc_mc_renderer_t\* r\);", code)
    # the definition is in the header's text: the byte formula and the blend against 0
    text = " ".join(header.replace("*", " ").split())
    assert "512 (sum of key_counts) + 4 n_keys cells" in text and "n_keys nx ny nz" in text
    assert "blends against 0" in text and "NOT a copy of the brick" in text and "ALWAYS host memory" in text
    L = api.load_library()
    assert L.nrc_renderer_volume_key_bytes(None) == 0 and L.nrc_mc_renderer_volume_key_bytes(None) == 0
    assert L.nrc_renderer_set_volume_key_bricks(None, None, None, None, 0, 0, 0) == -1      # (no renderer)
    for cls in ("NrcHpmRenderer", "McHpmRenderer"):
        body = hpp.split("class %s {" % cls)[1].split("\n};")[0]
        for name in ("void SetVolumeKeyBricks(const uint32_t* keyCounts, const int32_t* origins, const void* bricks, uint32_t nKeys",
                     "size_t VolumeKeyBytes() const"):
            assert name in body, (cls, name)
        for name in ("SetVolumeKeyBricks", "VolumeKeyBytes"):
            assert callable(getattr(getattr(api, cls), name)), (cls, name)


def test_python_mirror_validates_before_the_library_is_called(api):
    calls = []

    def fn(*a):
        calls.append(a)
        return 0
    o, b = np.zeros((3, 3), np.int32), np.zeros((3, 8, 8, 8), np.uint8)
    api._set_volume_key_bricks(fn, None, [1, 0, 2], o, b)
    assert len(calls) == 1 and calls[0][4:] == (3, api.VOLUME_U8, 0)
    api._set_volume_key_bricks(fn, None, np.array([3], np.uint32), o, b.astype(np.float32))
    assert calls[1][4:] == (1, api.VOLUME_F32, 0)
    api._set_volume_key_bricks(fn, None, [0, 0], o[:0], b[:0])      # only empty keys: no pointers
    assert calls[2][2] is None and calls[2][3] is None and calls[2][4] == 2
    api._set_volume_key_bricks(fn, None, None, None, None)          # drops the sequence
    assert calls[3][1:5] == (None, None, None, 0)
    for bad in (([1, 1], o, b), ([3], o.astype(np.int64), b), ([3], o, b.astype(np.float64)), ([3], o, b[:2]), ([3], o[:, :2], b),
                ([-1, 4], o, b), ([1.5, 1.5], o, b), ([3], o[::-1], b), ([[3]], o, b), ([3], o, "bricks")):
        with pytest.raises(RuntimeError, match="SkyRenderer ERROR"):
            api._set_volume_key_bricks(fn, None, *bad)
    assert len(calls) == 4
