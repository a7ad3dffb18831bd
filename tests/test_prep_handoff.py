"""The LR engine's prepare-ahead handoff (csrc/hip/prep_handoff.h) under sanitizers.

The header is host-only, so tools/prep_handoff_selftest.cpp drives the whole
protocol -- claim / prepare here / gather / failure / eviction / discard /
shutdown, one GPU and DP -- with a fake prep thread and fake actions, no GPU
and no Python extension.  Built twice with g++, like tests/test_host_sanitizers.py:
AddressSanitizer + UBSan and ThreadSanitizer; both must run clean.  The
scenario "re-prepare, failure" is the stranded-buffer defect the class fixes:
it is asserted here only (on the engine it would wait for ever).
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer", *flags,
           f"-I{CSRC}", os.path.join(ROOT, "tools", "prep_handoff_selftest.cpp"), "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(exe, env_extra):
    return subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, **env_extra))


def test_header_is_host_only(tmp_path):
    # plain g++, no ROCm include path: the protocol must not need HIP
    src = tmp_path / "only.cpp"
    src.write_text('#include "hip/prep_handoff.h"\nint main() { twtml::PrepHandoff h(true, false, nullptr); '
                   'return h.owns(0); }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", f"-I{CSRC}", str(src), "-o", str(tmp_path / "only"),
                        "-lpthread"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    text = open(os.path.join(CSRC, "hip", "prep_handoff.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


def test_prep_handoff_asan_ubsan(tmp_path):
    exe = _build(tmp_path, "handoff_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                            "-static-libasan"])
    r = _run(exe, {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr
    assert "prep handoff selftest ok" in r.stdout


def test_prep_handoff_tsan(tmp_path):
    exe = _build(tmp_path, "handoff_tsan", ["-fsanitize=thread", "-static-libtsan"])
    r = _run(exe, {"TSAN_OPTIONS": "halt_on_error=1:second_deadlock_stack=1"})
    if r.returncode != 0 and "unexpected memory mapping" in r.stderr:
        pytest.skip("ThreadSanitizer cannot map its shadow memory on this kernel")
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "WARNING: ThreadSanitizer" not in r.stderr
    assert "prep handoff selftest ok" in r.stdout
