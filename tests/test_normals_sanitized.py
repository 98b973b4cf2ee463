"""Surface normals, curvature and eigenvalues under the host sanitizers: tests/cpp/normals_sanitize_check.cpp, a stand-alone program with
its own main, linked with erasor_hip.hip compiled UNMODIFIED against the CPU stand-in of the HIP runtime (tests/cpp/simt_emu), both with
-fsanitize=address,undefined.  Device buffers are heap blocks and a workgroup's LDS arrays static arrays there: a kernel or a copy that
goes past one ends the program.  It runs a lattice with 300 copies of one point at k = 2, 8, 9, 32 with every combination of outputs
in exactly sized buffers, a cloud shorter than k, an empty one, and both orientation rules.  Host only: no GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_the_normals_are_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "normals_sanitize_check")
    subprocess.check_call(["g++", "-O1", "-std=c++20", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(HERE, "cpp", "simt_emu"), "-o", exe,
                           os.path.join(HERE, "cpp", "normals_sanitize_check.cpp"), "-x", "c++", os.path.join(ROOT, "erasor_amd", "csrc", "erasor_hip.hip")],
                          stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
