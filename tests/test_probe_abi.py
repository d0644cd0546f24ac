"""The C ABI of _hipprobe.so off the GPU: the xs_* symbols it exports are the
ones HipProbe binds, and every entry point of hbm_probe.hip refuses bad
arguments (-1000) and null or mis-aligned buffers (-1001) before it touches a
device. Only calls that must be refused are made: the pointers are made up, and
on a machine with a GPU a call that passed validation would be launched."""
import ctypes
import inspect
import re
import shutil
import subprocess

import pytest

from flex_gpu_scheduler_amd.ops import hip_probe

BAD_ARGS, BAD_BUFFER = -1000, -1001
P = 0x10000  # a made-up address, 16-byte aligned
MAX_GRID = 1 << 22


@pytest.fixture(scope="module")
def lib():
    try:
        return hip_probe.HipProbe()
    except (hip_probe.ProbeError, OSError) as e:
        pytest.skip(f"_hipprobe.so does not load here: {e}")


def test_exported_symbols_are_exactly_the_bound_ones(lib):
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm is not installed")
    out = subprocess.run([nm, "-D", "--defined-only", str(hip_probe._LIB)], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in out.stdout.splitlines() if line.split()}
    exported = {name for name in exported if name.startswith("xs_")}
    bound = set(re.findall(r"\bL\.(xs_\w+)\.(?:restype|argtypes)\b", inspect.getsource(hip_probe.HipProbe.__init__)))
    assert sorted(exported - bound) == [], "exported but not bound"
    assert sorted(bound - exported) == [], "bound but not exported"
    assert len(exported) == 57


def _fold():
    return (ctypes.c_ulonglong * 2)()


def stream(mode, a=P, b=P, c=P, nbytes=64, grid=0, fold=None):
    return "xs_stream_op", (0, mode, a, b, c, nbytes, 7, 3.0, 0, grid, fold)


def pinned(mode, src=P, dst=P, nbytes=64, mask=0x1, grid=0, fold=None):
    return "xs_pinned_op", (0, mode, src, dst, nbytes, mask, grid, fold)


def bandwidth(nbytes=1 << 20, mode=2):
    return "xs_hbm_bandwidth", (0, nbytes, 1, 0, mode, 0, None, None, None)


def bandwidth_xcd(nbytes=1 << 20, mask=0x1, mode=0):
    return "xs_hbm_bandwidth_xcd", (0, nbytes, 1, mask, mode, None, None, None)


def segment_access(mode=1, seg=128, stride=4096, touches=4):
    return "xs_segment_access", (0, mode, 0, seg, stride, touches, 1, (ctypes.c_double * 3)())


def segment_op(mode=1, seg=128, stride=4096, touches=4, buf=P, fold=None):
    return "xs_segment_op", (0, mode, 0, seg, stride, touches, buf, fold)


def pattern(buf=P, nbytes=64):
    return "xs_pattern_op", (0, buf, nbytes)


def checksum(buf=P, nbytes=64, out=True):
    return "xs_checksum_op", (0, buf, nbytes, ctypes.byref(ctypes.c_ulonglong()) if out else None)


REFUSED = {
    "stream mode 9": (stream(9), BAD_ARGS),
    "stream read without fold": (stream(0), BAD_ARGS),
    "stream write with fold": (stream(1, fold=_fold()), BAD_ARGS),
    "stream 0 bytes": (stream(1, nbytes=0), BAD_ARGS),
    "stream 24 bytes": (stream(1, nbytes=24), BAD_ARGS),
    "stream grid -1": (stream(1, grid=-1), BAD_ARGS),
    "stream grid above 2^22": (stream(1, grid=MAX_GRID + 1), BAD_ARGS),
    "stream mode 9 and null a": (stream(9, a=None), BAD_ARGS),  # bad arguments win over a bad buffer
    "stream null a": (stream(1, a=None), BAD_BUFFER),
    "stream copy null b": (stream(2, b=None), BAD_BUFFER),
    "stream triad null c": (stream(3, c=None), BAD_BUFFER),
    "stream a at 4 mod 16": (stream(1, a=P + 4), BAD_BUFFER),
    "pinned mode 9": (pinned(9), BAD_ARGS),
    "pinned read without fold": (pinned(0), BAD_ARGS),
    "pinned write with fold": (pinned(1, fold=_fold()), BAD_ARGS),
    "pinned 0 bytes": (pinned(1, nbytes=0), BAD_ARGS),
    "pinned 24 bytes": (pinned(1, nbytes=24), BAD_ARGS),
    "pinned grid -1": (pinned(1, grid=-1), BAD_ARGS),
    "pinned grid above 2^22": (pinned(1, grid=MAX_GRID + 1), BAD_ARGS),
    "pinned mask 0": (pinned(1, mask=0), BAD_ARGS),
    "pinned mask 0x100": (pinned(1, mask=0x100), BAD_ARGS),
    "pinned mask 0 and null dst": (pinned(1, mask=0, dst=None), BAD_ARGS),
    "pinned write null dst": (pinned(1, dst=None), BAD_BUFFER),
    "pinned copy null src": (pinned(2, src=None), BAD_BUFFER),
    "pinned read null src": (pinned(0, src=None, fold=_fold()), BAD_BUFFER),
    "pinned dst at 4 mod 16": (pinned(1, dst=P + 4), BAD_BUFFER),
    "bandwidth 8 bytes": (bandwidth(nbytes=8), BAD_ARGS),
    "bandwidth mode 4": (bandwidth(mode=4), BAD_ARGS),
    "bandwidth mode -1": (bandwidth(mode=-1), BAD_ARGS),
    "bandwidth_xcd 8 bytes": (bandwidth_xcd(nbytes=8), BAD_ARGS),
    "bandwidth_xcd mode 3": (bandwidth_xcd(mode=3), BAD_ARGS),
    "bandwidth_xcd mode -1": (bandwidth_xcd(mode=-1), BAD_ARGS),
    "bandwidth_xcd mask 0": (bandwidth_xcd(mask=0), BAD_ARGS),
    "bandwidth_xcd mask 0x1FF": (bandwidth_xcd(mask=0x1FF), BAD_ARGS),
    "pattern 0 bytes": (pattern(nbytes=0), BAD_ARGS),
    "pattern 6 bytes": (pattern(nbytes=6), BAD_ARGS),
    "pattern null buffer": (pattern(buf=None), BAD_BUFFER),
    "pattern buffer at 2 mod 4": (pattern(buf=P + 2), BAD_BUFFER),
    "checksum 0 bytes": (checksum(nbytes=0), BAD_ARGS),
    "checksum 6 bytes": (checksum(nbytes=6), BAD_ARGS),
    "checksum null out_sum": (checksum(out=False), BAD_ARGS),
    "checksum null buffer": (checksum(buf=None), BAD_BUFFER),
    "checksum buffer at 2 mod 4": (checksum(buf=P + 2), BAD_BUFFER),
    "segment_op read without fold": (segment_op(mode=0), BAD_ARGS),
    "segment_op write with fold": (segment_op(mode=1, fold=_fold()), BAD_ARGS),
    "segment_op null buffer": (segment_op(buf=None), BAD_BUFFER),
    "segment_op buffer at 4 mod 16": (segment_op(buf=P + 4), BAD_BUFFER),
}
for _name, _fn in (("segment_access", segment_access), ("segment_op", segment_op)):
    REFUSED.update({
        f"{_name} seg 8": (_fn(seg=8), BAD_ARGS),
        f"{_name} seg 24": (_fn(seg=24), BAD_ARGS),
        f"{_name} seg 1040": (_fn(seg=1040), BAD_ARGS),
        f"{_name} stride 100": (_fn(seg=64, stride=100), BAD_ARGS),
        f"{_name} stride below seg": (_fn(seg=256, stride=128), BAD_ARGS),
        f"{_name} 0 touches": (_fn(touches=0), BAD_ARGS),
        f"{_name} mode 2": (_fn(mode=2), BAD_ARGS),
    })


@pytest.mark.parametrize("case", list(REFUSED))
def test_bad_calls_are_refused_before_the_device_is_touched(lib, case):
    (symbol, args), want = REFUSED[case]
    assert getattr(lib.lib, symbol)(*args) == want
