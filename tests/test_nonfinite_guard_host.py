"""The training guard's surface without a GPU: the C header, the Python list of ABI symbols and the C++ mirror name the same three entry
points, the policy constants of api.py are the header's, and the command line has its switch."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nrc_cache_set_nonfinite_policy", "nrc_cache_get_nonfinite_policy", "nrc_cache_get_skipped_steps")


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_symbol_list_and_cpp_mirror_agree(api):
    header = re.sub(r"/\*.*?\*/", "", read("include", "nrc_hpm.h"), flags=re.S)
    mirror = read("include", "nrc_hpm.hpp")
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in api.ABI_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, mirror), name
    assert "void SetNonFinitePolicy(int policy)" in mirror and "GetSkippedSteps(" in mirror
    for method in ("SetNonFinitePolicy", "GetNonFinitePolicy", "GetSkippedSteps"):
        assert callable(getattr(api.NeuralRadianceCache, method)), method


def test_policy_constants_are_the_headers(api):
    header = read("include", "nrc_hpm.h")
    values = dict((k, int(v)) for k, v in re.findall(r"^#define (NRC_NONFINITE_[A-Z]+) (\d+)$", header, flags=re.M))
    assert values == dict(NRC_NONFINITE_PROPAGATE=0, NRC_NONFINITE_SKIP=1)
    for k, v in values.items():
        assert getattr(api, k) == v, k


def test_the_contract_is_stated_where_the_entry_points_are():
    """the step-number contract and the reason the table gradient is not scanned belong to the interface, not to a design note"""
    header = read("include", "nrc_hpm.h")
    doc = header[header.index("Training guard"):header.index("int nrc_cache_get_skipped_steps")]
    for phrase in ("A SKIPPED STEP IS A STEP WHOSE UPDATE IS THE IDENTITY", "COUNT ENQUEUED STEPS", "rule 1 covers it", "no further collective",
                   "Checkpoints do not carry the counter"):
        assert phrase in doc, phrase
    assert "skipped steps" in read("nrc-hpm-renderer_amd", "csrc", "nrc_checkpoint.hpp")


def test_cli_lists_the_switch():
    r = subprocess.run([sys.executable, "-m", "nrc_hpm_renderer_amd.cli", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--skip-nonfinite" in r.stdout
