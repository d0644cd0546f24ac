"""Runs the native tests of the cycle's fixed per-pod work (csrc/tests/assume_tests.cc):
FlexGPU placing a pod on the cycle's private copy before it is assumed, against
assume followed by Reserve, on two caches compared field by field; forget,
the informer's confirmation, Unreserve and a failing placement after the
fused path; the cycle number SchedulingQueue::pop hands out; append_int and
the joins against printf."""
import subprocess

from flex_gpu_scheduler_amd import build_ext


def test_native_assume_tests_pass():
    exe = build_ext.build_assume_tests(verbose=False)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
