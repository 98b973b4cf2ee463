"""The pose refinement under the host sanitizers: tests/cpp/refine_sanitize_check.cpp, a stand-alone program with its own main, linked with
erasor_hip.hip compiled UNMODIFIED against the CPU stand-in of the HIP runtime (tests/cpp/simt_emu), both with
-fsanitize=address,undefined.  Device buffers are heap blocks and a workgroup's LDS arrays static arrays there: a kernel or a copy that
goes past one ends the program.  It refines frames of 0, 1, 63 .. 65, 255 .. 257, 511 .. 513 and 1025 points in one call with the rows in a
heap block of exactly n_frames entries, then without rows, without a summary, and against the handle's map.  No GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_the_pose_refinement_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "refine_sanitize_check")
    subprocess.check_call(["g++", "-O1", "-std=c++20", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(HERE, "cpp", "simt_emu"), "-o", exe,
                           os.path.join(HERE, "cpp", "refine_sanitize_check.cpp"), "-x", "c++", os.path.join(ROOT, "erasor_amd", "csrc", "erasor_hip.hip")],
                          stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
