"""CPU sanitizers over the host side of the insertions and genotype entries: mgl_amd/csrc/sw_calls.cpp is built against the fake HIP
runtime (tests/cpp/fake_hip) with -fsanitize=address,undefined, and tests/cpp/calls_san_driver.cpp -- a program of its own, which stands
where the kernels stand -- calls every call-level refusal on both sides of its edge and accepted calls of both entries."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_calls_host_side_under_asan_ubsan():
    binary = os.path.join(CPP, "calls_san_asan")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "calls_san.mk", binary])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([binary], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "calls-san ok" in r.stdout and "ERROR: " not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
