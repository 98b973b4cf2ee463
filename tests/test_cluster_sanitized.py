"""The clustering under the host sanitizers: tests/cpp/cluster_sanitize_check.cpp, a stand-alone program with its own main, linked
with erasor_hip.hip compiled UNMODIFIED against the CPU stand-in of the HIP runtime (tests/cpp/simt_emu), both with
-fsanitize=address,undefined.  Device buffers are heap blocks there: a kernel or a copy that goes past one ends the program.  It
clusters a shuffled 4 096-point chain and 300 identical points with every output, and a short row buffer.  No GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_the_clustering_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = str(tmp_path / "cluster_sanitize_check")
    subprocess.check_call(["g++", "-O1", "-std=c++20", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(HERE, "cpp", "simt_emu"), "-o", exe,
                           os.path.join(HERE, "cpp", "cluster_sanitize_check.cpp"), "-x", "c++", os.path.join(ROOT, "erasor_amd", "csrc", "erasor_hip.hip")],
                          stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
