"""The host's hot-tile search (csrc/nrc_hot_tiles.hpp: the capped RNG states' preimages under the hash, probed in a per-geometry index of
the pixels' seeds) against a scan of every pixel of the frame -- what the device pre-pass it replaces did.  Plain C++17 that nrc_api.hip
and the kernels include; tests/cpp/hot_tiles_main.cpp drives it on the CPU under ASan + UBSan (no recovery): 8x8, 64x40, 256x144 and
1920x1080, whole and as the column strips of a world of 2 and of 8, 1000 seeded frame randoms each with one and with eight capped states,
the pinned state-0 and pair frames of tests/test_gpu_integrator.py, more capped pixels than the list holds, and geometry changes."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nrc-hpm-renderer_amd", "csrc")
HEADER = "nrc_hot_tiles.hpp"
CASES = 9       # begin_case calls of hot_tiles_main.cpp


def test_the_header_compiles_without_rocm_and_the_library_depends_on_it():
    """on its own, warnings as errors; no HIP identifier outside comments and outside the definition of NRC_HOT_HD, the function
    qualifier that is `inline` for every compiler but the device's; a Makefile variable of its own, among the build id's sources and the prerequisites of both objects that include it"""
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-include", HEADER, "-x", "c++", os.devnull],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-4000:]
    code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, HEADER)).read())
    code, n = re.subn(r"#if defined\(__HIPCC__\)\n#define NRC_HOT_HD [^\n]*\n#else\n#define NRC_HOT_HD inline\n#endif\n", "", code)
    assert n == 1
    assert not re.search(r"hip|nccl|__device__|__host__", code, re.I)
    assert "nrc_common.hpp" not in code
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^HOT_HDRS = " + re.escape(HEADER) + "$", makefile, re.M)
    assert re.search(r"^\s+\$\(HOST_HDRS\) \$\(HOT_HDRS\)$", makefile, re.M)
    for obj in ("nrc_api.o", "nrc_integrator.o"):
        rule = re.search(r"^\$\(OUT\)/" + re.escape(obj) + r":([^\n]*)$", makefile, re.M)
        assert rule and "$(HOT_HDRS)" in rule.group(1), obj


def test_hot_list_equals_a_scan_of_every_pixel_under_the_sanitizers():
    build = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "hot_tiles_main")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "hot_tiles_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out and "FAILED" not in out, out[-4000:]
    m = re.search(r"^hot_tiles: (\d+) cases, (\d+) checks$", out, re.M)
    assert m, out[-4000:]
    assert int(m.group(1)) == CASES and int(m.group(2)) >= 150
