"""The placement rule of the early stream (erasor_amd/csrc/stream_place.h: plain C++, no device) against pipe sequences: the order a
bare process with four queues deals its streams in, a free pipe on the first try, none in four tries, unknown pipes -- pads kept, the
candidate that holds the place, the give-up case.  A stand-alone program with its own main (tests/cpp/stream_place_check.cpp), once
plain and once under the address and undefined-behaviour sanitizers."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_placement_rule_on_pipe_sequences(tmp_path, flags):
    exe = str(tmp_path / "stream_place_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, os.path.join(HERE, "cpp", "stream_place_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "STREAM-PLACE OK" in out.stdout, out.stdout + out.stderr


def test_the_placement_header_stands_alone():
    """stream_place.h takes no handle and makes no device call: nothing of the runtime's is named in it, and the library includes it"""
    src = open(os.path.join(ROOT, "erasor_amd", "csrc", "stream_place.h")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "hip" not in code.lower() and "erasor_hip_handle" not in code
    assert '#include "stream_place.h"' in open(os.path.join(ROOT, "erasor_amd", "csrc", "erasor_hip.hip")).read()
