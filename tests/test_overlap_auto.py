"""The handle's overlap decision (erasor_amd/csrc/overlap_auto.h: plain C++, no device) against synthetic period sequences: early exit
either way, the full schedule inside the margin, a linear drift, a hiccup sample, the re-measurement, skipped samples -- a stand-alone
program with its own main (tests/cpp/overlap_auto_check.cpp), once plain and once under the address and undefined-behaviour
sanitizers."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_overlap_decision_on_synthetic_periods(tmp_path, flags):
    exe = str(tmp_path / "overlap_auto_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(HERE, "cpp", "overlap_auto_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "OVERLAP-AUTO OK" in out.stdout, out.stdout + out.stderr


def test_the_decision_header_stands_alone():
    """overlap_auto.h takes no handle and makes no device call: nothing of the runtime's is named in it, and the library includes it"""
    src = open(os.path.join(ROOT, "erasor_amd", "csrc", "overlap_auto.h")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "hip" not in code.lower() and "erasor_hip_handle" not in code
    assert '#include "overlap_auto.h"' in open(os.path.join(ROOT, "erasor_amd", "csrc", "erasor_hip.hip")).read()
