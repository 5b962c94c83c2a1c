"""The from-scratch VDB reader (nrc-hpm-renderer_amd/io_vdb.py; Texture3D::FromVDB semantics, src/Texture3D.cpp:12-82) on the
reference's own file, cut down: tests/golden/cloud_sixteenth_excerpt.vdb holds the leaves of data/volume/wdas_cloud_sixteenth.vdb in
the box (-16,-24,-16)..(32,0,24), four root children (origins (-4096,-4096,-4096), (-4096,-4096,0), (0,-4096,-4096), (0,-4096,0)), the
kept nodes' bytes unchanged (tests/golden/make_golden.py) -- 31 241 active voxels (= the `file_voxel_count` metadata make_golden.py
wrote), bounding box (-16,-19,-16)..(31,-1,23), and, quantised like src/Texture3D.cpp:106, a dense R8 volume equal byte for byte to
that block of the committed fixture of the whole file (cloud_sixteenth_u8.npz, 415 642 active voxels over (-66,-21,-90)..(59,64,63))."""
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VDB = os.path.join(GOLDEN, "cloud_sixteenth_excerpt.vdb")
BLOCK = (slice(74, 114), slice(2, 21), slice(50, 98))         # its block of cloud16 ([z][y][x], from (-66,-21,-90))


def test_vdb_reader_reproduces_the_fixture_and_the_files_voxel_count(sc, cloud16):
    from nrc_hpm_renderer_amd import io_vdb
    vol, info = io_vdb.from_vdb(VDB)
    assert info["active_voxels"] == 31241 == info["file_voxel_count"]
    assert tuple(info["bbox_min"]) == (-16, -19, -16) and tuple(info["bbox_max"]) == (31, -1, 23) and info["extent"] == (48, 19, 40)
    assert vol.dtype == np.float32 and vol.shape == (48, 19, 40) and float(vol.max()) == 1.0      # src/Texture3D.cpp:74
    u8 = sc.quantize_density(vol)
    assert cloud16.shape == (154, 86, 126) and u8.shape == (40, 19, 48) and np.array_equal(u8, cloud16[BLOCK])


def _build(name):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", name + ".cpp"), "-o", exe])
    return exe


def test_cpp_vdb_reader_equals_the_fixture(cloud16, tmp_path):
    """include/nrc_vdb.hpp -- the reader behind en::HpmScene(appConfig, "file.vdb") (src/HpmScene.cpp:44 -> Texture3D::FromVDB) -- on
    the reference's file cut down to four root children: the file's voxel count, its bounding box, and the dense R8 volume of that block
    of the committed fixture byte for byte"""
    import json
    import subprocess
    exe = _build("vdb_main")
    out = tmp_path / "cloud.u8"
    r = subprocess.run([exe, VDB, str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout)
    assert info["active_voxels"] == 31241 == info["file_voxel_count"] and info["max"] == 1.0 and info["grid"] == "density"
    assert (info["nx"], info["ny"], info["nz"]) == (48, 19, 40) and info["bbox_min"] == [-16, -19, -16] and info["bbox_max"] == [31, -1, 23]
    assert np.array_equal(np.fromfile(out, np.uint8), cloud16[BLOCK].reshape(-1))


def test_cpp_exr_reader_equals_the_python_reader(tmp_path):
    """include/nrc_exr.hpp -- what en::Reference loads its ground truth with (tinyexr's LoadEXR in src/Reference.cpp:617-631) -- on the
    reference's own ZIP-compressed images, the reference's compressed chunks byte for byte (tests/golden/make_golden.py): exr_{0,4}_rows.exr,
    32 rows through the middle of reference/{0,4}/0.exr, and exr_{0,4}_tail.exr, its last 24 rows -- one full 16-line chunk and the
    frame's short 8-line last chunk.  Bit-identical to io_exr.read_exr, and both equal to those rows of the full-size fixtures
    (exr_{0,4}_1920x1080.npz, whose statistics tests/golden/exr_stats.json pins)"""
    import subprocess
    from nrc_hpm_renderer_amd import io_exr
    exe = _build("exr_main")
    for sid in (0, 4):
        full = np.load(os.path.join(GOLDEN, "exr_%d_1920x1080.npz" % sid))
        for name, row0, rows in (("rows", 528, 32), ("tail", 1056, 24)):      # make_golden.py: EXR_ROW0, EXR_ROWS / EXR_TAIL0
            src = os.path.join(GOLDEN, "exr_%d_%s.exr" % (sid, name))
            out = tmp_path / ("ref%d_%s.f32" % (sid, name))
            r = subprocess.run([exe, src, str(out)], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
            assert json.loads(r.stdout) == {"width": 1920, "height": rows}
            a = np.fromfile(out, np.float32).reshape(rows, 1920, 4)
            py = io_exr.read_exr(src)
            assert py.shape == (rows, 1920, 4) and np.array_equal(a.view(np.uint32), py.view(np.uint32))
            for c in range(3):
                assert np.array_equal(py[..., c].view(np.uint32), full["L"][row0:row0 + rows].view(np.uint32))
            assert np.array_equal(py[..., 3].view(np.uint32), full["A"][row0:row0 + rows].view(np.uint32))


def _build_asan(name):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.join(root, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, name + "_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", name + ".cpp"), "-o", exe])
    return exe


def _mutations(data, rng, n):
    """truncations, bytes flipped in the header region, and 32/64-bit fields overwritten with huge / negative values"""
    out = [data[:k] for k in (0, 3, 8, 40, 100, len(data) // 2, len(data) - 1)]
    for _ in range(n):
        b = bytearray(data)
        pos = int(rng.integers(0, min(len(b), 600)))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            b[pos] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:
            b[pos:pos + 4] = (0xFFFFFFF0).to_bytes(4, "little")
        else:
            b[pos:pos + 8] = (0x7FFFFFFFFFFFFFF0).to_bytes(8, "little")
        out.append(bytes(b[:len(data)]))
    return out


def test_cpp_readers_reject_malformed_files_without_reading_out_of_bounds(tmp_path):
    """offsets and sizes the VDB / EXR readers take from the file are checked overflow-safely -- a truncated or corrupted
    file ends in `SkyRenderer ERROR` (exit 1) or is read (exit 0), never in an out-of-bounds access (the readers run under
    AddressSanitizer + UBSan here: a report aborts with another status)"""
    import subprocess
    from nrc_hpm_renderer_amd import io_exr
    rng = np.random.default_rng(3)
    img = rng.random((24, 20, 4), dtype=np.float32)
    good = tmp_path / "good.exr"
    io_exr.write_exr(str(good), img, compression="zip")
    exe = _build_asan("exr_main")
    r = subprocess.run([exe, str(good), str(tmp_path / "o.f32")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(np.fromfile(tmp_path / "o.f32", np.float32).reshape(24, 20, 4), img)
    data = good.read_bytes()
    seen = {0: 0, 1: 0}
    for k, m in enumerate(_mutations(data, rng, 150)):
        bad = tmp_path / "bad.exr"
        bad.write_bytes(m)
        r = subprocess.run([exe, str(bad), str(tmp_path / "o.f32")], capture_output=True, text=True, timeout=60)
        assert r.returncode in (0, 1), (k, r.returncode, r.stderr[-1500:])
        assert r.returncode == 0 or "SkyRenderer ERROR" in r.stderr, r.stderr[-500:]
        seen[r.returncode] += 1
    assert seen[1] > 20
    exe = _build_asan("vdb_main")
    data = open(VDB, "rb").read()
    seen = {0: 0, 1: 0}
    for k, m in enumerate(_mutations(data, rng, 40)):
        bad = tmp_path / "bad.vdb"
        bad.write_bytes(m)
        r = subprocess.run([exe, str(bad), str(tmp_path / "o.u8")], capture_output=True, text=True, timeout=120)
        assert r.returncode in (0, 1), (k, r.returncode, r.stderr[-1500:])
        assert r.returncode == 0 or "SkyRenderer ERROR" in r.stderr, r.stderr[-500:]
        seen[r.returncode] += 1
    assert seen[1] > 10
