"""Test infrastructure: the CPU stand-in of the HIP runtime (tests/cpp/simt_emu).  erasor_hip.hip -- and with it every header it includes,
the kernels and the analyses' host code -- compiled UNMODIFIED by g++ against the stand-in, and `-m gpu` test files re-run in a helper
process that loads that library (ERASOR_TEST_SIMT_LIB, see conftest.py).  A plain module like hooks.py: the test_*_on_cpu.py files call it."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build_simt_lib(dir, hooks=True):
    """liberasor_hip_simt.so in `dir` (hooks: with the library's test hooks); its path"""
    lib = os.path.join(str(dir), "liberasor_hip_simt.so")
    subprocess.check_call(["g++", "-x", "c++", "-O1", "-std=c++20", "-pthread", "-ffp-contract=off", "-fPIC", "-shared"] +
                          (["-DERASOR_HIP_TEST_HOOKS"] if hooks else []) +
                          ["-I" + os.path.join(HERE, "cpp", "simt_emu"), "-o", lib, os.path.join(ROOT, "erasor_amd", "csrc", "erasor_hip.hip")])
    return lib


def build_oracle():
    sys.path.insert(0, ROOT)
    from oracle import orc
    orc.build()


def run_gpu_tests_on_stand_in(lib, test_file, k_expr, min_passed, timeout=3000, no_skips=False):
    """`pytest tests/<test_file> -m gpu -x -k k_expr` against `lib` (test_file: one name or a list of names); at least min_passed tests
    must pass and none fail (no_skips: nor be skipped).  Returns the number passed."""
    files = [test_file] if isinstance(test_file, str) else list(test_file)
    env = dict(os.environ, ERASOR_TEST_SIMT_LIB=lib)
    out = subprocess.run([sys.executable, "-m", "pytest"] + [os.path.join(HERE, f) for f in files] + ["-m", "gpu", "-q", "-x", "-k", k_expr,
                         "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    tail = out.stdout[-1500:]
    sys.stdout.write(tail)
    assert out.returncode == 0 and " passed" in tail and "failed" not in tail, out.stdout[-4000:] + out.stderr[-2000:]
    assert not (no_skips and "skipped" in tail), tail
    n_passed = int(tail.split(" passed")[0].split()[-1])
    assert n_passed >= min_passed, tail
    return n_passed
