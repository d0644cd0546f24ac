"""Runs the native tests of the lister's gang entries (csrc/tests/gang_tests.cc):
seeded random lister sequences checked after every step against the locked
lookups by name and a plain model, retired entries, instance counts, readers
on several threads, and the open gang record inside the entry."""
import subprocess

from flex_gpu_scheduler_amd import build_ext


def test_native_gang_tests_pass():
    exe = build_ext.build_gang_tests(verbose=False)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
