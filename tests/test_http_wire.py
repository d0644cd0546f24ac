"""Runs the native tests of the HTTP/1.1 wire layer (csrc/tests/wire_tests.cc):
lines, exact reads, buffer compaction, chunk sizes, chunked bodies with a
byte cap, the header scanner and its framing facts, send_all to a slow or
closed peer, and the failure record the REST client's retry rule reads."""
import subprocess

from flex_gpu_scheduler_amd import build_ext


def test_http_wire_tests_pass():
    exe = build_ext.build_wire_tests(verbose=False)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
