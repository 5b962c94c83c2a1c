"""Sanitizer run of the library's device-free host logic (VERDICT.md weak point 15): the schedule-cache text parser, the schedule key, the
event-pool bookkeeping and the schedule tuner (csrc/nrc_schedule.hpp), the checkpoint file reader / writer (nrc_checkpoint.hpp) and the
occupancy builders (nrc_occupancy.hpp), the move-only owners of handles and device memory (nrc_owned.hpp) and the renderers' frame
bookkeeping (nrc_frame_state.hpp: which random numbers a frame uses, when a sorted tile order takes effect) are plain C++17 that
nrc_api.hip includes; tests/cpp/host_logic_main.cpp drives them on the CPU under ASan + UBSan (no recovery) -- the tuner against a
scripted clock, reset in mid-trial and event-pool wrap included; the owners against an allocator of the program's own; the frame
bookkeeping against the conditions Renderer::render held before, frame by frame."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nrc-hpm-renderer_amd", "csrc")
HOST_HEADERS = ["nrc_fail.hpp", "nrc_owned.hpp", "nrc_schedule.hpp", "nrc_checkpoint.hpp", "nrc_occupancy.hpp"]
FRAME_HEADERS = ["nrc_frame_state.hpp"]
CASES = 32      # begin_case calls of host_logic_main.cpp


def test_host_headers_compile_without_rocm():
    """each on its own, warnings as errors, include/ the only include path; no HIP / RCCL identifier outside comments"""
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^HOST_HDRS = " + " ".join(HOST_HEADERS) + "$", makefile, re.M), "HOST_HEADERS here and HOST_HDRS of csrc/Makefile differ"
    assert re.search(r"^FRAME_HDRS = " + " ".join(FRAME_HEADERS) + "$", makefile, re.M), "FRAME_HEADERS here and FRAME_HDRS of csrc/Makefile differ"
    for h in HOST_HEADERS + FRAME_HEADERS:
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            "-include", h, "-x", "c++", os.devnull], capture_output=True, text=True, cwd=CSRC)
        assert r.returncode == 0, r.stderr[-4000:]
        text = open(os.path.join(CSRC, h)).read()
        code = re.sub(r"//[^\n]*", "", text)
        assert not re.search(r"hip|nccl", code, re.I), h
        assert "nrc_common.hpp" not in code, h


def test_host_logic_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    build = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "host_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "host_logic_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(tmp_path), os.path.join(ROOT, "nrc-hpm-renderer_amd", "schedules.txt")],
                       capture_output=True, text=True, timeout=900, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out and "FAILED" not in out, out[-4000:]
    m = re.search(r"^host_logic: (\d+) cases, (\d+) checks$", out, re.M)
    assert m, out[-4000:]
    assert int(m.group(1)) == CASES and int(m.group(2)) > 400
