"""ctypes front-end for the HIP/CDNA4 device probes: what the node agent runs
before it advertises an MI355X as schedulable.

Probes (csrc/hip/hbm_probe.hip, csrc/hip/mfma_probe.hip): device properties;
HBM streaming bandwidth, optionally with a partition-sized CU budget or on a
partition's XCDs; an XCD census that verifies the compute-partition mode; a
checksum health test; an exact-integer MFMA tile check of the matrix cores;
the dense bf16 MFMA throughput of the whole GPU or of one partition's XCDs.

Sweeps of every CU (csrc/hip/<name>.hip), each naming the XCD of a CU that fails:
  * cu_sweep: MFMA, VALU and LDS;
  * matrix_sweep: every matrix format (f16, f32, f64, fp8, bf8, i8 and the
    block-scaled MX fp8/fp6/fp4); names the formats;
  * regfile_sweep: every SIMD's whole VGPR/AGPR file; names the register
    file, the cells and the SIMDs;
  * lane_sweep: the cross-lane network (DPP, permlane swaps, readlane /
    writelane, the LDS crossbar) and the wide, sub-dword, transposed, atomic
    and DMA LDS paths; names the paths;
  * valu_sweep: every SIMD's vector ALU (float, packed, wide-integer,
    bit-field, dot, conversion and transcendental instructions); names the
    units and the steps;
  * mem_sweep: the path between a wave's registers and HBM (global, buffer
    and flat loads and stores of every width, the memory-side atomics, the
    vector L1, the XCD's L2 and the scalar data cache); names the routes.
    It is a library of its own, _hipmem.so;
  * scalar_sweep: every CU's scalar ALU (arithmetic, logic, bit, compare,
    branch, EXEC-mask and relative-move instructions) and the SGPRs a wave
    can name; names the parts. It is a library of its own, _hipscalar.so;
  * consensus_sweep: the instructions whose bits no document fixes (raw
    transcendentals, division helpers, stochastic roundings, NaN payloads and
    saturation, the narrow transposed LDS reads and float LDS atomics, the
    MFMA shapes the matrix sweep leaves out and the sparse SMFMAC family),
    judged not against the host but by a vote across the CUs of the GPU
    (vote_consensus); names the parts. A library of its own, _hipconsensus.so;
  * fetch_sweep: every CU's instruction fetch path and instruction cache
    (256 KiB of straight-line code, counted backward loops, computed jumps
    and calls, jump targets at every dword of a cache line and across a page,
    a refetch after s_icache_inv), the test data being the literals in the
    sweep's own code; names the parts. A library of its own, _hipfetch.so.
The matrix, lane, VALU and memory sweeps are sweeps over named parts:
PART_SWEEPS describes each, and one implementation serves the four and the
scalar sweep, whose row SCALAR_SWEEP stands beside the table, as do
CONSENSUS_SWEEP, the consensus sweep's, and FETCH_SWEEP, the fetch sweep's.

hbm_sweep (csrc/hip/hbm_sweep.hip): all free HBM under an address-keyed
pattern in both polarities; names the vectors and bits that read back wrong.
"""
from __future__ import annotations

import ctypes
import json
import struct
from dataclasses import dataclass
from pathlib import Path

_LIB = Path(__file__).resolve().parent / "_hipprobe.so"
# The memory sweep is a library of its own: _hipprobe.so's C ABI stays as it is.
_MEM_LIB = Path(__file__).resolve().parent / "_hipmem.so"
# So is the scalar sweep.
_SCALAR_LIB = Path(__file__).resolve().parent / "_hipscalar.so"
# And the consensus sweep.
_CONSENSUS_LIB = Path(__file__).resolve().parent / "_hipconsensus.so"
# And the fetch sweep.
_FETCH_LIB = Path(__file__).resolve().parent / "_hipfetch.so"
MODES = {"read": 0, "write": 1, "copy": 2, "triad": 3}


class ProbeError(RuntimeError):
    rc: int | None = None  # the C ABI's return code, where one caused the error


BAD_ARGS = -1000
# k_pinned: a selected XCD received no workgroup, so its slice of the buffer
# was never processed (xs_pinned_op, xs_hbm_bandwidth_xcd).
PINNED_UNDRAINED = -1002
# k_mfma_peak: a selected XCD ran no workgroup, so the rate would be that of
# fewer XCDs than asked for (xs_mfma_peak).
MFMA_IDLE_XCD = -1002
MFMA_PEAK_BLOCK = 256  # threads per k_mfma_peak workgroup: 4 waves
MFMA_PEAK_ACC = 4  # independent 32x32 accumulators per wave
MFMA_DID_NOT_RUN = 1 << 31  # xs_mfma_peak_op: flag of a workgroup that exited
MFMA_WORDING = {-1001: "null buffer"}  # return codes _probe_error words itself


@dataclass
class Bandwidth:
    """`gbps` / `ms_per_iter`: the median launch, each timed by its own event
    pair (what rocprofv3 reports as the dispatch time). `best_gbps`: the
    fastest launch. `batch_gbps`: back-to-back launches including the gaps
    between them."""
    mode: str
    bytes: int
    gbps: float
    ms_per_iter: float
    cu_limit: int
    best_gbps: float = 0.0
    batch_gbps: float = 0.0


# Working sets default to 1 GiB per array: 4x the MI355X's 256 MB Infinity
# Cache, so a streaming rate is HBM's, not the cache's.
DEFAULT_BYTES = 1 << 30

# k_cu_sweep (csrc/hip/cu_sweep.hip)
SWEEP_ENGINES = {1: "mfma", 2: "valu", 4: "lds"}  # fail bit -> digest of that engine
SWEEP_LDS_MAX = 160 << 10

# k_matrix_sweep (csrc/hip/matrix_sweep.hip): one 64-byte record per workgroup,
# {xcd, cu, simd_mask, fail, one digest per format, 0}.
MATRIX_RECORD_WORDS = 16

# k_regfile_sweep (csrc/hip/regfile_sweep.hip): one 64-byte record per
# workgroup, {xcd, cu, simd_mask, fail, bad_vgpr, bad_agpr, first, flip, digest,
# bad_simds, 0 x 6}.
REGFILE_RECORD_WORDS = 16
REGFILE_SEED = 0x5BD1E995
REGFILE_FILES = ["vgpr", "agpr"]  # fail bit order
REGFILE_CELLS = 512  # per lane: v0..v255 then a0..a255
REGFILE_NO_CELL = 0xFFFF  # `first` of a record without a mis-compare

# k_lane_sweep (csrc/hip/lane_sweep.hip): one 128-byte record per workgroup,
# {xcd, cu, simd_mask, fail, 8 bad counts, 8 digests, bad_simds, 0 x 11}.
LANE_RECORD_WORDS = 32
LANE_SEED = 0x1B873593
LANE_BLOCK = 256  # threads per workgroup: the last axis of a probe's dump

# k_valu_sweep (csrc/hip/valu_sweep.hip): one 128-byte record per workgroup;
# words 22..27 are bits over the global step index of the steps that mis-compared.
VALU_RECORD_WORDS = 32
VALU_SEED = 0x1B873593
VALU_ROUNDS = 2  # operand sets per step; measured in profiles/valu_sweep_defaults.md
VALU_BLOCK = 256

# k_mem_sweep (csrc/hip/mem_sweep.hip): one 128-byte record per workgroup,
# {xcd, cu, simd_mask, fail, 7 bad counts, 7 digests, bad_simds, 0 x 13}.
MEM_RECORD_WORDS = 32
MEM_SEED = 0x1B873593
MEM_BLOCK = 256
# xs_mem_sweep could not allocate its arena: nothing was launched. The GPU is
# unswept, never failed (the meaning HBM_UNSWEPT has).
MEM_UNSWEPT = -1003
# A guard band of the arena did not hold the host's sentinel after the launch:
# a store went astray. The library's last error names the first bad address.
MEM_STRAY_STORE = -1004
MEM_WORDING = {MEM_UNSWEPT: "no memory could be had for the arena: nothing was swept"}
# The C ABI of _hipmem.so.
MEM_SYMBOLS = ("xs_mem_sweep_last_error", "xs_mem_routes", "xs_mem_shape", "xs_mem_probe", "xs_mem_sweep_expected",
               "xs_mem_sweep_info", "xs_mem_sweep")

# k_scalar_sweep (csrc/hip/scalar_sweep.hip): one 128-byte record per workgroup,
# {xcd, cu, simd_mask, fail, 8 bad counts, 8 digests, bad_simds, 0, per SIMD the
# OR of its waves' raw HW_REG_GPR_ALLOC words and the OR of their complements, 0 x 2}.
SCALAR_RECORD_WORDS = 32
SCALAR_SEED = 0x1B873593
SCALAR_BLOCK = 1024
SCALAR_COVER_WORD = 22  # the first of the eight coverage words
# The C ABI of _hipscalar.so.
SCALAR_SYMBOLS = ("xs_scalar_sweep_last_error", "xs_scalar_parts", "xs_scalar_shape", "xs_scalar_probe",
                  "xs_scalar_sweep_expected", "xs_scalar_sweep_info", "xs_scalar_sweep")

# k_consensus_sweep (csrc/hip/consensus_sweep.hip): one 128-byte record per
# workgroup, {xcd, cu, simd_mask, fail = 0, 7 digests, 0 x 21}. The device does
# not judge; vote_consensus does.
CONSENSUS_RECORD_WORDS = 32
CONSENSUS_SEED = 0x1B873593
CONSENSUS_ROUNDS = 4  # operand sets per step; measured in profiles/consensus_sweep_defaults.md
CONSENSUS_BLOCK = 256
# The C ABI of _hipconsensus.so.
CONSENSUS_SYMBOLS = ("xs_consensus_sweep_last_error", "xs_consensus_parts", "xs_consensus_shape",
                     "xs_consensus_probe", "xs_consensus_operands", "xs_consensus_sweep_info", "xs_consensus_sweep")

# k_fetch_sweep (csrc/hip/fetch_sweep.hip): one 128-byte record per workgroup,
# {xcd, cu, simd_mask, fail, 5 bad counts, 5 digests, bad_simds, 0 x 17}. The
# device holds no expected words: `bad` counts an injection only.
FETCH_RECORD_WORDS = 32
FETCH_SEED = 0x1B873593
FETCH_ROUNDS = 2  # multiplies the loop trips and the call rounds; measured in profiles/fetch_sweep_defaults.md
FETCH_BLOCK = 256
FETCH_SEGMENTS = 32  # of 8 KiB: the rows of fetch_probe_clocks
# The C ABI of _hipfetch.so.
FETCH_SYMBOLS = ("xs_fetch_sweep_last_error", "xs_fetch_parts", "xs_fetch_shape", "xs_fetch_probe",
                 "xs_fetch_sweep_expected", "xs_fetch_sweep_info", "xs_fetch_sweep")


@dataclass(frozen=True)
class PartSweep:
    """A sweep over named parts: a bit mask selects parts, the selected ones run
    on every CU, a record's fail bits are part bits and it carries one digest
    per part. Its C ABI is xs_<prefix>_sweep(dev, blocks, mask, [seed,
    [rounds,]] inject xcd, cu, mask, records, n, ms), xs_<prefix>_sweep_expected(
    mask, [seed, [rounds,]] digests) and xs_<prefix>_shape(part, out)."""
    prefix: str
    names_symbol: str  # returns the part names, comma-separated, in bit order
    noun: str  # a part, in error messages
    summary_key: str  # the failed parts, in the summary
    selection: str  # the selected parts, in the summary
    record_words: int
    digests: int  # word offset of the first part's digest in a record; so the next three, where it has them
    bad: int | None = None  # a mismatch count per part
    bad_simds: int | None = None
    step_mask: int | None = None  # bits over the global step index


PART_SWEEPS = {
    "matrix": PartSweep("matrix", "xs_matrix_formats", "matrix format", "failed_formats", "formats",
                        MATRIX_RECORD_WORDS, digests=4),
    "lane": PartSweep("lane", "xs_lane_paths", "lane path", "failed_paths", "paths",
                      LANE_RECORD_WORDS, digests=12, bad=4, bad_simds=20),
    "valu": PartSweep("valu", "xs_valu_units", "VALU unit", "failed_units", "units",
                      VALU_RECORD_WORDS, digests=12, bad=4, bad_simds=20, step_mask=22),
    "mem": PartSweep("mem", "xs_mem_routes", "memory route", "failed_routes", "routes",
                     MEM_RECORD_WORDS, digests=11, bad=4, bad_simds=18),
}
MATRIX_SWEEP, LANE_SWEEP, VALU_SWEEP, MEM_SWEEP = PART_SWEEPS.values()
# The scalar sweep's row stands beside the table: same record head as the lane sweep's.
SCALAR_SWEEP = PartSweep("scalar", "xs_scalar_parts", "scalar part", "failed_parts", "parts", 32,
                         digests=12, bad=4, bad_simds=20)
# So does the consensus sweep's: a record is the four head words and the digests.
CONSENSUS_SWEEP = PartSweep("consensus", "xs_consensus_parts", "consensus part", "failed_parts", "parts",
                            CONSENSUS_RECORD_WORDS, digests=4)
# And the fetch sweep's: the lane sweep's head with five parts.
FETCH_SWEEP = PartSweep("fetch", "xs_fetch_parts", "fetch part", "failed_parts", "parts", FETCH_RECORD_WORDS,
                        digests=9, bad=4, bad_simds=14)

# k_hbm_fill / k_hbm_verify (csrc/hip/hbm_sweep.hip)
HBM_SWEEP_SEED = 0x5EED1E55
HBM_SWEEP_LOG_CAP = 32
HBM_SWEEP_STRIPES = 16
HBM_SWEEP_BAD_CHUNKS = 64
HBM_BAD_BUFFER = -1001
HBM_WORDING = {HBM_BAD_BUFFER: "null or mis-aligned buffer"}  # return codes _probe_error words itself
# xs_hbm_sweep could not allocate even its first chunk: nothing was tested.
# The GPU is unswept, never failed.
HBM_UNSWEPT = -1003
# From this size a sweep's reads come from HBM: 4x the 256 MiB Infinity Cache.
HBM_FROM_DRAM_BYTES = 1 << 30
HBM_NO_INJECT = (1 << 64) - 1


class _HbmLogEntry(ctypes.Structure):
    _fields_ = [("v", ctypes.c_uint64), ("expected", ctypes.c_uint32 * 4), ("actual", ctypes.c_uint32 * 4),
                ("xcd", ctypes.c_uint32), ("pass_", ctypes.c_uint32)]


class _HbmStripe(ctypes.Structure):
    _fields_ = [("vectors_read", ctypes.c_uint64), ("fold", ctypes.c_uint64), ("reserved", ctypes.c_uint64 * 14)]


class _HbmSweepResult(ctypes.Structure):
    # The waves of a launch spread their (vectors_read, fold) atomics over 16
    # stripes of one 128-byte line each: the count is their sum, the fold their XOR.
    _fields_ = [("stripe", _HbmStripe * HBM_SWEEP_STRIPES), ("bad_vectors", ctypes.c_uint64),
                ("bad_bits", ctypes.c_uint64), ("one_to_zero", ctypes.c_uint64), ("zero_to_one", ctypes.c_uint64),
                ("flip_or", ctypes.c_uint32 * 4), ("reader_xcd_mask", ctypes.c_uint32),
                ("log_claims", ctypes.c_uint32), ("log", _HbmLogEntry * HBM_SWEEP_LOG_CAP),
                ("pad", ctypes.c_uint8 * 72)]


class _HbmBadChunk(ctypes.Structure):
    _fields_ = [("chunk", ctypes.c_uint64), ("bad_vectors", ctypes.c_uint64)]


class _HbmSweepSummary(ctypes.Structure):
    _fields_ = [("bytes_requested", ctypes.c_uint64), ("bytes_tested", ctypes.c_uint64),
                ("chunk_bytes", ctypes.c_uint64), ("chunks", ctypes.c_uint32), ("short", ctypes.c_uint32),
                ("vectors_read", ctypes.c_uint64), ("fold", ctypes.c_uint64 * 2), ("bad_vectors", ctypes.c_uint64),
                ("bad_bits", ctypes.c_uint64), ("one_to_zero", ctypes.c_uint64), ("zero_to_one", ctypes.c_uint64),
                ("flip_or", ctypes.c_uint32 * 4), ("reader_xcd_mask", ctypes.c_uint32),
                ("log_entries", ctypes.c_uint32), ("ms", ctypes.c_double * 3), ("bad_chunks", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("bad_chunk", _HbmBadChunk * HBM_SWEEP_BAD_CHUNKS)]


assert ctypes.sizeof(_HbmLogEntry) == 48 and ctypes.sizeof(_HbmSweepResult) == 3712 and _HbmSweepResult.log.offset == 2104
assert ctypes.sizeof(_HbmSweepSummary) == 144 + 16 * HBM_SWEEP_BAD_CHUNKS


def _hbm_log(entries) -> list[dict]:
    return [{"v": int(e.v), "expected": [int(w) for w in e.expected], "actual": [int(w) for w in e.actual],
             "xcd": int(e.xcd), "pass": int(e.pass_)} for e in entries]


def _probe_error(last_error, rc: int, what: str, wording: dict | None = None) -> ProbeError:
    """The ProbeError of return code `rc` of `what`. `last_error` is the
    xs_*_last_error of the file that returned it, asked only for a code that
    neither BAD_ARGS nor `wording` ({rc: text}) puts into words."""
    detail = {BAD_ARGS: "bad arguments", **(wording or {})}.get(rc)
    if detail is None:
        detail = last_error().decode(errors="replace")
    e = ProbeError(f"{what} failed ({rc}): {detail}")
    e.rc = rc
    return e


def _name_mask(names: list[str], chosen, what: str) -> int:
    """The bits of `chosen` (one name, several, or None for all) in `names`' order."""
    if chosen is None:
        return (1 << len(names)) - 1
    mask = 0
    for f in [chosen] if isinstance(chosen, str) else chosen:
        if f not in names:
            raise ValueError(f"unknown {what} {f!r}; known: {', '.join(names)}")
        mask |= 1 << names.index(f)
    return mask


def _inject_target(t: tuple | None) -> tuple[int, int]:
    """(xcd, cu key) of an `inject` / `poison` tuple as the C ABI takes them:
    -1 for no XCD (no tuple) and for every CU of the XCD (None)."""
    return (-1, -1) if t is None else (int(t[0]), -1 if t[1] is None else int(t[1]))


def decode_part_record(kind: PartSweep, names: list[str], w, expected: dict, steps=()) -> dict:
    """The record of one workgroup of a sweep over named parts from its words
    `w`. `names`: the parts in bit order; `expected`: the host's digest per
    selected part; `steps`: the step names in the order of the step mask's
    bits. A digest that differs from the host's (0 for a part not selected) sets
    the part's fail bit, even if the device's comparator, on the same CU, passed it."""
    n = len(names)
    digests = w[kind.digests:kind.digests + n]
    rec = {"xcd": w[0], "cu": w[1], "simd_mask": w[2], "fail": w[3]}
    if kind.bad is not None:
        rec["bad"] = dict(zip(names, w[kind.bad:kind.bad + n]))
    rec["digests"] = dict(zip(names, digests))
    if kind.bad_simds is not None:
        rec["bad_simds"] = w[kind.bad_simds]
    if kind.step_mask is not None:
        mask = w[kind.step_mask:kind.step_mask + (len(steps) + 31) // 32]  # seldom set: walk the steps only then
        rec["bad_steps"] = [s for g, s in enumerate(steps) if mask[g // 32] >> (g % 32) & 1] if any(mask) else []
    for b, f in enumerate(names):
        if digests[b] != expected.get(f, 0):
            rec["fail"] |= 1 << b
    return rec


class HipProbe:
    def __init__(self, path: str | Path = _LIB, mem_path: str | Path = _MEM_LIB,
                 scalar_path: str | Path = _SCALAR_LIB, consensus_path: str | Path = _CONSENSUS_LIB,
                 fetch_path: str | Path = _FETCH_LIB):
        for built in (path, mem_path, scalar_path, consensus_path, fetch_path):
            if not Path(built).exists():
                raise ProbeError(f"{built} not built; run `python -m flex_gpu_scheduler_amd.build_ext --hip`")
        try:
            # torch's bundled libamdhip64.so.7 first, whatever the import order
            # of the caller: the probe library then resolves the same soname to
            # that copy, so one HIP runtime owns every device pointer and
            # stream in the process (tensors handed to the kernels included).
            import torch  # noqa: F401
        except ImportError:
            pass
        self.lib = ctypes.CDLL(str(path))
        L = self.lib
        L.xs_last_error.restype = ctypes.c_char_p
        L.xs_device_count.restype = ctypes.c_int
        L.xs_device_props.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.xs_hbm_bandwidth.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                       ctypes.POINTER(ctypes.c_double)]
        L.xs_hbm_bandwidth_xcd.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_double)]
        L.xs_xcd_census.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                    ctypes.POINTER(ctypes.c_int)]
        L.xs_health_check.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_ulonglong),
                                      ctypes.POINTER(ctypes.c_ulonglong)]
        L.xs_stream_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_size_t, ctypes.c_uint32, ctypes.c_float, ctypes.c_int, ctypes.c_int,
                                   ctypes.POINTER(ctypes.c_ulonglong)]
        L.xs_pinned_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                   ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong)]
        L.xs_checksum_op.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_ulonglong)]
        L.xs_segment_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t,
                                    ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong)]
        L.xs_segment_access.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t,
                                        ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
        L.xs_mfma_last_error.restype = ctypes.c_char_p
        L.xs_mfma_check.argtypes = [ctypes.c_int, ctypes.c_int]
        L.xs_mfma_peak.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int,
                                   ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                   ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint),
                                   ctypes.POINTER(ctypes.c_double)]
        L.xs_mfma_max_k.restype = ctypes.c_int
        L.xs_mfma_tile_op.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.xs_mfma_inputs.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.xs_mfma_compare.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        L.xs_mfma_peak_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint)]
        L.xs_pattern_op.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
        L.xs_health_verify.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                       ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_ulonglong)]
        L.xs_cu_sweep_last_error.restype = ctypes.c_char_p
        L.xs_cu_sweep_max_lds.argtypes = [ctypes.c_int]
        L.xs_cu_sweep_max_lds.restype = ctypes.c_size_t
        L.xs_cu_sweep_expected.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]
        L.xs_cu_sweep.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int,
                                  ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                                  ctypes.POINTER(ctypes.c_double)]
        L.xs_matrix_sweep_last_error.restype = ctypes.c_char_p
        L.xs_matrix_formats.restype = ctypes.c_char_p
        L.xs_matrix_shape.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.xs_matrix_inputs.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p]
        L.xs_matrix_tile.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.xs_matrix_sweep_expected.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        L.xs_matrix_sweep.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                                      ctypes.POINTER(ctypes.c_double)]
        L.xs_regfile_sweep_last_error.restype = ctypes.c_char_p
        L.xs_regfile_sweep_expected.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        L.xs_regfile_sweep_info.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.xs_regfile_sweep.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]
        L.xs_lane_sweep_last_error.restype = ctypes.c_char_p
        L.xs_lane_paths.restype = ctypes.c_char_p
        L.xs_lane_shape.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.xs_lane_probe.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]
        L.xs_lane_sweep_expected.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        L.xs_lane_sweep_info.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.xs_lane_sweep.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                    ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                                    ctypes.POINTER(ctypes.c_double)]
        L.xs_valu_sweep_last_error.restype = ctypes.c_char_p
        L.xs_valu_units.restype = ctypes.c_char_p
        L.xs_valu_steps.restype = ctypes.c_char_p
        L.xs_valu_steps.argtypes = [ctypes.c_int]
        L.xs_valu_shape.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.xs_valu_expected.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                       ctypes.c_size_t]
        L.xs_valu_probe.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                    ctypes.c_size_t]
        L.xs_valu_sweep_expected.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                             ctypes.POINTER(ctypes.c_uint32)]
        L.xs_valu_sweep_info.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        L.xs_valu_sweep.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                    ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p,
                                    ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]
        # mem_sweep.hip's library. Its functions are made attributes of
        # self.lib, where _call and _part_sweep look every xs_* up.
        self.mem_lib = ctypes.CDLL(str(mem_path))
        M = self.mem_lib
        M.xs_mem_sweep_last_error.restype = ctypes.c_char_p
        M.xs_mem_routes.restype = ctypes.c_char_p
        M.xs_mem_shape.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        M.xs_mem_probe.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]
        M.xs_mem_sweep_expected.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        M.xs_mem_sweep_info.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        M.xs_mem_sweep.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                                   ctypes.POINTER(ctypes.c_double)]
        for name in MEM_SYMBOLS:
            setattr(L, name, getattr(M, name))
        # scalar_sweep.hip's library, looked up through self.lib in the same way.
        self.scalar_lib = ctypes.CDLL(str(scalar_path))
        S = self.scalar_lib
        S.xs_scalar_sweep_last_error.restype = ctypes.c_char_p
        S.xs_scalar_parts.restype = ctypes.c_char_p
        S.xs_scalar_shape.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        S.xs_scalar_probe.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]
        S.xs_scalar_sweep_expected.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        S.xs_scalar_sweep_info.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        S.xs_scalar_sweep.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                                      ctypes.POINTER(ctypes.c_double)]
        for name in SCALAR_SYMBOLS:
            setattr(L, name, getattr(S, name))
        # consensus_sweep.hip's library, likewise.
        self.consensus_lib = ctypes.CDLL(str(consensus_path))
        C = self.consensus_lib
        C.xs_consensus_sweep_last_error.restype = ctypes.c_char_p
        C.xs_consensus_parts.restype = ctypes.c_char_p
        C.xs_consensus_shape.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        C.xs_consensus_probe.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]
        C.xs_consensus_operands.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]
        C.xs_consensus_sweep_info.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        C.xs_consensus_sweep.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                         ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p,
                                         ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]
        for name in CONSENSUS_SYMBOLS:
            setattr(L, name, getattr(C, name))
        # fetch_sweep.hip's library, likewise.
        self.fetch_lib = ctypes.CDLL(str(fetch_path))
        F = self.fetch_lib
        F.xs_fetch_sweep_last_error.restype = ctypes.c_char_p
        F.xs_fetch_parts.restype = ctypes.c_char_p
        F.xs_fetch_shape.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        F.xs_fetch_probe.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                     ctypes.c_size_t]
        F.xs_fetch_sweep_expected.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                              ctypes.POINTER(ctypes.c_uint32)]
        F.xs_fetch_sweep_info.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        F.xs_fetch_sweep.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p,
                                     ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]
        for name in FETCH_SYMBOLS:
            setattr(L, name, getattr(F, name))
        L.xs_hbm_sweep_last_error.restype = ctypes.c_char_p
        L.xs_hbm_sweep_pattern.argtypes = [ctypes.c_uint64, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int,
                                           ctypes.c_void_p]
        L.xs_hbm_sweep_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64,
                                      ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
        L.xs_hbm_sweep.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64,
                                   ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]

    def _call(self, file: str, what: str, *args, wording: dict | None = None, value: bool = False) -> int:
        """xs_<what>(*args), whose file's last error is xs_<file>_last_error
        (xs_last_error for "", hbm_probe.hip). A ProbeError unless it returns
        0 or, with `value`, a count of 0 or more, which is returned. `wording`
        as in _probe_error."""
        rc = getattr(self.lib, f"xs_{what}")(*args)
        if rc < 0 or (rc and not value):
            raise _probe_error(getattr(self.lib, f"xs_{file}_last_error" if file else "xs_last_error"), rc, what,
                               wording)
        return rc

    def device_count(self) -> int:
        return int(self.lib.xs_device_count())

    def props(self, dev: int = 0) -> dict:
        buf = ctypes.create_string_buffer(4096)
        self._call("", "device_props", dev, buf, len(buf), value=True)
        return json.loads(buf.value.decode())

    def _bandwidth(self, what: str, mode: str, nbytes: int, cus: int, *args) -> Bandwidth:
        """The Bandwidth of xs_<what>(*args, gbps, ms_per_iter, detail) over `cus` CUs."""
        g, ms = ctypes.c_double(), ctypes.c_double()
        d = (ctypes.c_double * 3)()
        self._call("", what, *args, ctypes.byref(g), ctypes.byref(ms), d)
        return Bandwidth(mode, nbytes, g.value, ms.value, cus, d[0], d[1])

    def hbm_bandwidth(self, dev: int = 0, nbytes: int = DEFAULT_BYTES, iters: int = 20, cu_limit: int = 0,
                      mode: str = "copy", variant: int = 0) -> Bandwidth:
        return self._bandwidth("hbm_bandwidth", mode, nbytes, cu_limit, dev, nbytes, iters, cu_limit, MODES[mode],
                               variant)

    @staticmethod
    def variant(unroll: int = 4, nontemporal: bool = True, blocks_per_cu: int = 8) -> int:
        """blocks_per_cu 0: the one-shot grid (one workgroup per 4 KiB x
        unroll, no loop) instead of a persistent one."""
        if blocks_per_cu == 0:
            return unroll | (0x100 if nontemporal else 0) | 0x200
        return unroll | (0x100 if nontemporal else 0) | (blocks_per_cu << 16)

    def hbm_bandwidth_variant(self, dev: int, nbytes: int, iters: int, mode: str, unroll: int, nontemporal: bool,
                              blocks_per_cu: int, cu_limit: int = 0) -> Bandwidth:
        return self.hbm_bandwidth(dev, nbytes, iters, cu_limit, mode,
                                  variant=self.variant(unroll, nontemporal, blocks_per_cu))

    def tune(self, dev: int = 0, mode: str = "copy", nbytes: int = DEFAULT_BYTES, iters: int = 10) -> dict:
        """Sweep unroll x cache policy x workgroups/CU; return the fastest."""
        results = []
        for unroll in (1, 4, 8):
            for nt in (True, False):
                for bpc in (0, 4, 8, 16):
                    bw = self.hbm_bandwidth_variant(dev, nbytes, iters, mode, unroll, nt, bpc)
                    results.append({"unroll": unroll, "nontemporal": nt, "blocks_per_cu": bpc,
                                    "GBps": round(bw.gbps, 1)})
        best = max(results, key=lambda r: r["GBps"])
        return {"mode": mode, "best": best, "all": results}

    # ------------------------------------------------ kernels on torch tensors
    # The streaming kernels run on caller-owned device buffers so the GPU tier
    # can check their output against a plain PyTorch fp32 reference. torch
    # must be imported before this library is loaded (one HIP runtime: both
    # resolve the soname libamdhip64.so.7 to the same copy).
    @staticmethod
    def _dev_buf(t, what: str, granule: int = 16) -> tuple[int, int]:
        """(pointer, bytes) of a device tensor whose size and address are
        multiples of `granule`; 0 leaves that check to the C ABI."""
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous device tensor")
        nbytes = t.numel() * t.element_size()
        if granule and (nbytes % granule or t.data_ptr() % granule):
            raise ValueError(f"{what}: {nbytes} bytes at {t.data_ptr():#x} is not {granule}-byte granular")
        return t.data_ptr(), nbytes

    # `grid` > 0 launches that many workgroups of 256 lanes instead of the
    # variant's own grid: small buffers then reach the unrolled loop bodies
    # and the grid-stride path that production sizes reach.
    def _stream(self, dev: int, mode: int, a, b, c, nbytes: int, seed: int = 7, scale: float = 3.0,
                variant: int = 0, grid: int = 0, fold=None) -> None:
        self._call("", "stream_op", dev, mode, a, b, c, nbytes, seed, scale, variant, grid, fold)

    def read_fold(self, src, variant: int = 0, grid: int = 0) -> tuple[int, int]:
        """k_read, checked instantiation: (XOR of every 32-bit word of `src`,
        number of 16-B loads the launch issued)."""
        p, n = self._dev_buf(src, "src")
        fold = (ctypes.c_ulonglong * 2)()
        self._stream(src.device.index or 0, MODES["read"], p, None, None, n, variant=variant, grid=grid, fold=fold)
        return int(fold[0]), int(fold[1])

    def write_pattern(self, dst, seed: int = 7, variant: int = 0, grid: int = 0) -> None:
        """k_write: every 16-B lane of `dst` <- (seed, seed^0x55555555, seed+1, ~seed) as uint32."""
        p, n = self._dev_buf(dst, "dst")
        self._stream(dst.device.index or 0, MODES["write"], p, None, None, n, seed=seed, variant=variant, grid=grid)

    def copy(self, dst, src, variant: int = 0, grid: int = 0) -> None:
        """k_copy: dst <- src (byte copy; equal sizes)."""
        pd, n = self._dev_buf(dst, "dst")
        ps, ns = self._dev_buf(src, "src")
        if n != ns:
            raise ValueError("copy: size mismatch")
        self._stream(dst.device.index or 0, MODES["copy"], ps, pd, None, n, variant=variant, grid=grid)

    def triad(self, a, b, c, scale: float = 3.0, variant: int = 0, grid: int = 0) -> None:
        """k_triad (STREAM): a <- b + scale*c on fp32 tensors."""
        import torch

        if not (a.dtype == b.dtype == c.dtype == torch.float32):
            raise ValueError("triad: fp32 tensors only")
        pa, n = self._dev_buf(a, "a")
        pb_, nb = self._dev_buf(b, "b")
        pc, nc = self._dev_buf(c, "c")
        if not n == nb == nc:
            raise ValueError("triad: size mismatch")
        self._stream(a.device.index or 0, MODES["triad"], pa, pb_, pc, n, scale=scale, variant=variant, grid=grid)

    def pinned(self, dst, src=None, xcd_mask: int = 0x1, grid: int = 0) -> None:
        """k_pinned on the XCDs of `xcd_mask`: copy src -> dst, or write the
        fill pattern (1, 2, 3, 4) into dst when src is None. Raises ProbeError
        with rc PINNED_UNDRAINED when a selected XCD received no workgroup
        (its slice is then untouched). `grid` > 0: that many workgroups
        instead of 8 per CU."""
        pd, n = self._dev_buf(dst, "dst")
        ps = 0
        if src is not None:
            ps, ns = self._dev_buf(src, "src")
            if ns != n:
                raise ValueError("pinned: size mismatch")
        self._call("", "pinned_op", dst.device.index or 0, 2 if src is not None else 1, ps or None, pd, n, xcd_mask,
                   grid, None)

    def pinned_read_fold(self, src, xcd_mask: int = 0x1, grid: int = 0) -> tuple[int, int]:
        """k_pinned's read mode, checked instantiation: (XOR of every 32-bit
        word of `src`, number of 16-B loads issued)."""
        ps, n = self._dev_buf(src, "src")
        fold = (ctypes.c_ulonglong * 2)()
        self._call("", "pinned_op", src.device.index or 0, 0, ps, None, n, xcd_mask, grid, fold)
        return int(fold[0]), int(fold[1])

    def checksum(self, buf) -> int:
        """k_checksum (the health check's kernel) over a device tensor: the
        sum of its 32-bit words."""
        p, n = self._dev_buf(buf, "buf", granule=4)
        out = ctypes.c_ulonglong()
        self._call("", "checksum_op", buf.device.index or 0, p, n, ctypes.byref(out))
        return int(out.value)

    def segment_op(self, buf, mode: str = "read", seg_bytes: int = 128, stride_bytes: int = 4096, touches: int = 1,
                   nontemporal: bool = False) -> tuple[int, int] | None:
        """One k_segments launch over `buf` (stride_bytes x touches bytes).
        "write" stores the fill (5, 6, 7, 8) into the first `seg_bytes` of
        every slot; "read" returns (XOR of the 32-bit words read, number of
        16-B loads issued)."""
        p, n = self._dev_buf(buf, "buf")
        if n != stride_bytes * touches:
            raise ValueError(f"segment_op: buf holds {n} bytes, not {stride_bytes} x {touches}")
        fold = (ctypes.c_ulonglong * 2)() if mode == "read" else None
        self._call("", "segment_op", buf.device.index or 0, MODES[mode], int(nontemporal), seg_bytes, stride_bytes,
                   touches, p, fold)
        return (int(fold[0]), int(fold[1])) if fold is not None else None

    def hbm_bandwidth_xcd(self, dev: int = 0, xcd_mask: int = 0x1, nbytes: int = DEFAULT_BYTES, iters: int = 10,
                          mode: str = "read") -> Bandwidth:
        return self._bandwidth("hbm_bandwidth_xcd", mode, nbytes, bin(xcd_mask).count("1") * 32, dev, nbytes, iters,
                               xcd_mask, MODES[mode])

    def partition_table(self, dev: int = 0, nbytes: int = DEFAULT_BYTES, iters: int = 10) -> dict:
        """HBM read/copy GB/s that the CUs of one compute partition pull, for
        each partition size of an MI355X (CPX = 1 XCD, QPX = 2, DPX = 4,
        SPX = 8), measured on the XCDs a partition of that size would own.
        The node agent publishes it with the GPU's health (gpu/telemetry)."""
        rows = {}
        for mode_name, xcds in (("CPX", 1), ("QPX", 2), ("DPX", 4), ("SPX", 8)):
            row = {"xcds": xcds, "cus": xcds * 32}
            rows[mode_name] = row
            if xcds == 8:
                # An SPX partition is the whole GPU, dispatched as any kernel
                # is: measured with the full-device streaming kernels, not the
                # XCD-pinned one (whose per-XCD work queues cost ~16% at 8 XCDs).
                r = self.hbm_bandwidth(dev, nbytes, iters, mode="read")
                c = self.hbm_bandwidth(dev, nbytes, iters, mode="copy")
                kernel = "k_read / k_copy (full device)"
            else:
                mask = (1 << xcds) - 1
                kernel = "k_pinned (workgroups on the partition's XCDs)"
                try:
                    r = self.hbm_bandwidth_xcd(dev, mask, nbytes, iters, "read")
                    c = self.hbm_bandwidth_xcd(dev, mask, nbytes, iters, "copy")
                except ProbeError as e:
                    if e.rc != PINNED_UNDRAINED:
                        raise
                    # Not every XCD of this set took work (a partitioned
                    # device, or other tenants held it): no rate for bytes
                    # that were not moved; the other rows stand.
                    row.update(read_GBps=None, copy_GBps=None, read_ms=None, kernel=kernel, unmeasured=str(e))
                    continue
            row.update(read_GBps=round(r.gbps, 1), copy_GBps=round(c.gbps, 1), read_ms=round(r.ms_per_iter, 4),
                       kernel=kernel)
        return {"bytes": nbytes, "timing": "median of per-launch event pairs", "partitions": rows}

    def segment_access(self, dev: int = 0, mode: str = "read", seg_bytes: int = 128, stride_bytes: int = 4096,
                       touches: int = 1 << 18, iters: int = 5, nontemporal: bool = False) -> dict:
        """k_segments: `touches` segments of `seg_bytes`, one per
        `stride_bytes` slot -- a dispatch of known bytes and 128-B lines, for
        calibrating rocprofv3's L2 request counters (scripts/pmc_calibrate.sh)."""
        out = (ctypes.c_double * 3)()
        self._call("", "segment_access", dev, MODES[mode], int(nontemporal), seg_bytes, stride_bytes, touches, iters,
                   out)
        return {"kernel": "k_segments", "mode": mode, "nontemporal": nontemporal, "seg_bytes": seg_bytes,
                "stride_bytes": stride_bytes, "touches": touches, "ms": round(out[0], 4),
                "bytes_per_dispatch": int(out[1]), "lines128_per_dispatch": int(out[2])}

    def xcd_census(self, dev: int = 0, blocks: int = 4096) -> dict:
        hist = (ctypes.c_int * 8)()
        cus = ctypes.c_int()
        rc = self._call("", "xcd_census", dev, blocks, hist, ctypes.byref(cus), value=True)
        return {"distinct_xcds": rc, "blocks_per_xcd": list(hist), "distinct_cu_slots": cus.value}

    def health(self, dev: int = 0, nbytes: int = 64 << 20) -> dict:
        d, h = ctypes.c_ulonglong(), ctypes.c_ulonglong()
        rc = self._call("", "health_check", dev, nbytes, ctypes.byref(d), ctypes.byref(h), value=True)
        return {"healthy": rc == 0, "device_sum": d.value, "host_sum": h.value}

    def pattern(self, buf) -> None:
        """k_pattern (the health check's fill) over a device tensor: 32-bit
        word i <- uint32(i * 2654435761) ^ 0xa5a5a5a5."""
        p, n = self._dev_buf(buf, "buf", granule=0)
        self._call("", "pattern_op", buf.device.index or 0, p, n)

    def health_verify(self, buf) -> dict:
        """The health check's verdict over a device tensor: k_checksum's sum
        of its words against the host's sum of the pattern for that size."""
        p, n = self._dev_buf(buf, "buf", granule=0)
        d, h = ctypes.c_ulonglong(), ctypes.c_ulonglong()
        rc = self._call("", "health_verify", buf.device.index or 0, p, n, ctypes.byref(d), ctypes.byref(h), value=True)
        return {"healthy": rc == 0, "device_sum": d.value, "host_sum": h.value}

    def mfma_check(self, dev: int = 0, k: int = 64) -> dict:
        """C[32x32] = A·B through v_mfma_f32_32x32x16_bf16 on exact integers.
        `k`: a positive multiple of 16, at most mfma_max_k() (ProbeError with
        rc BAD_ARGS otherwise)."""
        rc = self._call("mfma", "mfma_check", dev, k, wording=MFMA_WORDING, value=True)
        return {"healthy": rc == 0, "mismatches": int(rc), "k": k}

    def mfma_max_k(self) -> int:
        return int(self.lib.xs_mfma_max_k())

    def mfma_inputs(self, k: int = 64):
        """The check's operands as integers: (A [32, k], B [k, 32]), int32. No device call."""
        import numpy as np

        a, b = np.zeros((32, max(k, 0)), np.int32), np.zeros((max(k, 0), 32), np.int32)
        self._call("mfma", "mfma_inputs", k, a.ctypes.data, b.ctypes.data, wording=MFMA_WORDING)
        return a, b

    def mfma_compare(self, k: int, c, cap: int = 32) -> tuple[int, list[int]]:
        """The check's comparator over a caller's C [32, 32] (fp32): the number
        of elements that differ from the integer product of mfma_inputs(k) and
        the flat indices of the first `cap` of them. No device call."""
        import numpy as np

        c = np.ascontiguousarray(c, np.float32)
        if c.shape != (32, 32):
            raise ValueError(f"mfma_compare: C is {c.shape}, not (32, 32)")
        idx = np.full(max(cap, 1), -1, np.int32)
        rc = self._call("mfma", "mfma_compare", k, c.ctypes.data, idx.ctypes.data, cap, wording=MFMA_WORDING, value=True)
        return int(rc), [int(i) for i in idx[:min(rc, cap)]]

    def mfma_tile(self, a_bits, b_bits, dev: int = 0):
        """k_mfma_tile as the check launches it, on the caller's operands:
        `a_bits` [32, K] and `b_bits` [K, 32] are uint16 bf16 bit patterns;
        returns C [32, 32] as fp32. K is taken from `a_bits` and refused by the
        C ABI unless a positive multiple of 16 up to mfma_max_k()."""
        import numpy as np

        a = np.ascontiguousarray(a_bits, np.uint16)
        b = np.ascontiguousarray(b_bits, np.uint16)
        if a.ndim != 2 or a.shape[0] != 32 or b.shape != (a.shape[1], 32):
            raise ValueError(f"mfma_tile: A {a.shape} and B {b.shape} are not [32, K] and [K, 32]")
        c = np.zeros((32, 32), np.float32)
        self._call("mfma", "mfma_tile_op", dev, a.ctypes.data, b.ctypes.data, a.shape[1], c.ctypes.data,
                   wording=MFMA_WORDING)
        return c

    def mfma_peak_op(self, dev: int = 0, xcd_mask: int = 0xFF, iters: int = 1, blocks: int = 0) -> dict:
        """One launch of k_mfma_peak's checked instantiation. `acc`: fp32
        [blocks, 256, 4, 16], every lane's accumulators (all-ones bit patterns
        where the workgroup did not run); `xcd`: the XCD of every workgroup;
        `ran`: whether it ran; `active_per_xcd`: the kernel's eight counters."""
        import numpy as np

        n = blocks if blocks > 0 else 8 * int(self.props(dev)["computeUnits"])
        acc = np.zeros((n, MFMA_PEAK_BLOCK, MFMA_PEAK_ACC, 16), np.float32)
        xcd = np.zeros(n, np.uint32)
        per = (ctypes.c_uint * 8)()
        self._call("mfma", "mfma_peak_op", dev, iters, xcd_mask, n, acc.ctypes.data, xcd.ctypes.data, per,
                   wording=MFMA_WORDING)
        return {"acc": acc, "xcd": (xcd & 0xF).astype(np.int64), "ran": (xcd & MFMA_DID_NOT_RUN) == 0,
                "raw_xcd": xcd, "active_per_xcd": [int(v) for v in per], "iters": iters, "xcd_mask": xcd_mask}

    def mfma_peak(self, dev: int = 0, xcd_mask: int = 0xFF, iters: int = 4096, blocks: int = 0) -> dict:
        """Dense bf16 MFMA TFLOP/s on the XCDs of `xcd_mask` (1..0xFF). `flops`
        is what the timed dispatch is credited with: active_blocks x 4 waves x
        4 accumulators x iters x 2*32*32*16. Raises ProbeError with rc
        MFMA_IDLE_XCD when a selected XCD ran no workgroup."""
        tf, ms, act, fl = ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
        per = (ctypes.c_uint * 8)()
        self._call("mfma", "mfma_peak", dev, iters, xcd_mask, blocks, ctypes.byref(tf), ctypes.byref(ms),
                   ctypes.byref(act), per, ctypes.byref(fl), wording=MFMA_WORDING)
        return {"tflops": tf.value, "ms": ms.value, "active_blocks": act.value, "xcd_mask": xcd_mask,
                "active_per_xcd": [int(v) for v in per], "flops": fl.value, "iters": iters if iters > 0 else 4096}

    # ------------------------------------------------------ the per-CU sweeps
    def _sweep_until_covered(self, name: str, dev: int, blocks: int, max_rounds: int, words: int, launch, expected,
                             decode, summarize, wording: dict | None = None) -> dict:
        """The launch policy of every per-CU sweep. A launch whose grid could
        cover the device (`blocks` 0 = 4 per CU) is repeated while some CU has
        not been seen, at most `max_rounds` launches in all; records accumulate.

        `launch(blocks, buf, n, ms)` calls xs_<name> into `buf` (`words` uint32
        per record) and returns its code; `expected()` is the host's digests,
        asked for once, after the first launch; `decode(w, expected)` makes the
        record of one workgroup's words, failing it where a digest differs
        from the host's even if the device-side comparator (on the same CU)
        passed it; `summarize(records, compute_units)` is the verdict; `wording`
        as in _probe_error.
        Returns {"records", "summary": the verdict plus rounds, ms, blocks}."""
        cus = int(self.props(dev)["computeUnits"])
        n_blocks = blocks if blocks != 0 else 4 * cus
        want = None
        records: list[dict] = []
        total_ms, rounds = 0.0, 0
        summary: dict = {}
        for _ in range(max(1, max_rounds if n_blocks >= cus else 1)):
            buf = (ctypes.c_uint32 * (words * max(1, n_blocks)))()
            n, ms = ctypes.c_int(), ctypes.c_double()
            rc = launch(n_blocks, buf, ctypes.byref(n), ctypes.byref(ms))
            if rc != 0:
                raise _probe_error(getattr(self.lib, f"xs_{name}_last_error"), rc, name, wording)
            if want is None:
                want = expected()
            rounds += 1
            total_ms += ms.value
            # struct splits the buffer into one tuple of words per record far
            # faster than slicing the ctypes array does.
            rows = struct.iter_unpack(f"{words}I", bytes(buf)[:4 * words * n.value])
            records += [decode(w, want) for w in rows]
            summary = summarize(records, cus)
            if summary["covered"]:
                break
        summary.update(rounds=rounds, ms=total_ms, blocks=n_blocks)
        return {"records": records, "summary": summary}

    # ------------------------------------------------------------- CU sweep
    def cu_sweep_max_lds(self, dev: int = 0) -> int:
        """Bytes of LDS one sweep workgroup can cover on `dev` (160 KiB on an MI355X)."""
        n = int(self.lib.xs_cu_sweep_max_lds(dev))
        if n <= 0:
            raise ProbeError(f"cu_sweep_max_lds failed: {self.lib.xs_cu_sweep_last_error().decode(errors='replace')}")
        return n

    def cu_sweep_expected(self, k: int = 64, lds_bytes: int = SWEEP_LDS_MAX) -> dict:
        """The digests a healthy CU leaves, computed on the host."""
        out = (ctypes.c_uint32 * 3)()
        self._call("cu_sweep", "cu_sweep_expected", k, lds_bytes, out)
        return {"mfma": out[0], "valu": out[1], "lds": out[2]}

    def cu_sweep(self, dev: int = 0, blocks: int = 0, k: int = 64, lds_bytes: int | None = None,
                 inject: tuple | None = None, max_rounds: int = 4) -> dict:
        """k_cu_sweep: MFMA, VALU and LDS checked on every CU a workgroup lands
        on. `lds_bytes` None: all of a CU's LDS. `inject` = (xcd, cu key or
        None for every CU of that XCD, engine bits): those workgroups flip one
        bit of what they computed (tests the comparator on a healthy GPU).

        A launch whose grid could cover the device (blocks 0 = 4 per CU) is
        repeated while some CU has not been seen, at most `max_rounds`
        launches in all; records accumulate. Returns {"records": [...],
        "summary": summarize_sweep(...) plus rounds, ms, blocks}."""
        if lds_bytes is None:
            lds_bytes = self.cu_sweep_max_lds(dev)
        (ix, ic), ie = _inject_target(inject), 0 if inject is None else int(inject[2])

        def decode(w, expected):
            rec = {"xcd": w[0], "cu": w[1], "simd_mask": w[2], "fail": w[3], "mfma": w[4], "valu": w[5], "lds": w[6]}
            for bit, name in SWEEP_ENGINES.items():
                if rec[name] != expected[name]:
                    rec["fail"] |= bit
            return rec

        out = self._sweep_until_covered(
            "cu_sweep", dev, blocks, max_rounds, 8,
            lambda nb, *out: self.lib.xs_cu_sweep(dev, nb, k, lds_bytes, ix, ic, ie, *out),
            lambda: self.cu_sweep_expected(k, lds_bytes), decode, summarize_sweep)
        out["summary"].update(k=k, lds_bytes=lds_bytes)
        return out

    # ---------------------------------------------- sweeps over named parts
    def _part_names(self, kind: PartSweep) -> list[str]:
        return getattr(self.lib, kind.names_symbol)().decode().split(",")

    def _part_mask(self, kind: PartSweep, chosen) -> int:
        return _name_mask(self._part_names(kind), chosen, kind.noun)

    def _part_shape(self, kind: PartSweep, name: str, fields: int):
        out = (ctypes.c_int * fields)()
        self._part_mask(kind, [name])  # ValueError for a name the sweep does not have
        self._call(f"{kind.prefix}_sweep", f"{kind.prefix}_shape", self._part_names(kind).index(name), out)
        return out

    def _part_expected(self, kind: PartSweep, chosen, *args) -> dict:
        names = self._part_names(kind)
        mask = self._part_mask(kind, chosen)
        out = (ctypes.c_uint32 * len(names))()
        self._call(f"{kind.prefix}_sweep", f"{kind.prefix}_sweep_expected", mask, *args, out)
        return {n: out[i] for i, n in enumerate(names) if mask >> i & 1}

    def _sweep_info(self, name: str, dev: int, fields: tuple) -> dict:
        """xs_<name>_info: what the runtime reports for the sweep's kernel, under `fields`."""
        out = (ctypes.c_int * len(fields))()
        self._call(name, f"{name}_info", dev, out)
        return dict(zip(fields, out))

    def _part_sweep(self, kind: PartSweep, summarize, dev: int, blocks: int, chosen, inject, max_rounds: int,
                    args: tuple = (), report: dict | None = None, steps=(), wording: dict | None = None,
                    tail=None) -> dict:
        """One sweep over the `chosen` parts (None: all), its verdict being
        summarize(records, compute_units, names). `args` stand between the mask
        and the injection in the C call and behind the mask in that of the
        expected digests; `report` goes into the summary before the selection;
        `wording` as in _probe_error; `tail(w)` is what a record holds besides
        decode_part_record's fields."""
        names = self._part_names(kind)
        mask = self._part_mask(kind, chosen)
        selected = [f for i, f in enumerate(names) if mask >> i & 1]
        (ix, ic), im = _inject_target(inject), 0 if inject is None else self._part_mask(kind, inject[2])
        sweep = getattr(self.lib, f"xs_{kind.prefix}_sweep")
        out = self._sweep_until_covered(
            f"{kind.prefix}_sweep", dev, blocks, max_rounds, kind.record_words,
            lambda nb, *out: sweep(dev, nb, mask, *args, ix, ic, im, *out),
            lambda: self._part_expected(kind, selected, *args),
            lambda w, expected: {**decode_part_record(kind, names, w, expected, steps), **(tail(w) if tail else {})},
            lambda records, cus: summarize(records, cus, names), wording)
        out["summary"].update(report or {}, **{kind.selection: selected})
        return out

    # --------------------------------------------------------- matrix sweep
    def matrix_formats(self) -> list[str]:
        """Format names of the matrix sweep; the index is the format's bit."""
        return self._part_names(MATRIX_SWEEP)

    def _matrix_mask(self, formats) -> int:
        return self._part_mask(MATRIX_SWEEP, formats)

    def matrix_shape(self, fmt: str) -> dict:
        """`tile` (the result is tile x tile), `k` (both K-steps), `blocks`
        (32-element scale blocks along K; 0 when not block-scaled),
        `accumulator` and `frac` (every result is a multiple of 2^-frac)."""
        out = self._part_shape(MATRIX_SWEEP, fmt, 5)
        return {"tile": out[0], "k": out[1], "blocks": out[2], "accumulator": ("f32", "f64", "i32")[out[3]],
                "frac": out[4]}

    def matrix_inputs(self, fmt: str) -> dict:
        """The operand encodings of one format, as the kernels build them:
        `a` [tile, k] and `b` [k, tile] (uint64 bit patterns: IEEE bits for
        f16/f32/f64, one byte for fp8/bf8/i8, the 6- or 4-bit code for the MX
        fp6/fp4 rows) and, for the block-scaled rows, the E8M0 scale bytes
        `a_scale` [tile, k/32] and `b_scale` [k/32, tile] (else None)."""
        import numpy as np

        sh = self.matrix_shape(fmt)
        t, k, nb = sh["tile"], sh["k"], sh["blocks"]
        a, b = np.zeros((t, k), np.uint64), np.zeros((k, t), np.uint64)
        sa = np.zeros((t, nb), np.uint8) if nb else None
        sb = np.zeros((nb, t), np.uint8) if nb else None
        self._call("matrix_sweep", "matrix_inputs", self.matrix_formats().index(fmt), a.ctypes.data, b.ctypes.data,
                   sa.ctypes.data if nb else None, sb.ctypes.data if nb else None)
        return {"a": a, "b": b, "a_scale": sa, "b_scale": sb, **sh}

    def matrix_tile(self, dev: int, fmt: str):
        """k_matrix_tile: one wave computes the format's product; the whole
        result tile as float64 (int64 for i8)."""
        import numpy as np

        sh = self.matrix_shape(fmt)
        out = np.zeros((sh["tile"], sh["tile"]), np.float64)
        self._call("matrix_sweep", "matrix_tile", dev, self.matrix_formats().index(fmt), out.ctypes.data)
        return out.astype(np.int64) if sh["accumulator"] == "i32" else out

    def matrix_sweep_expected(self, formats=None) -> dict:
        """The workgroup digest a healthy CU leaves per selected format,
        computed on the host from the decoded operand encodings."""
        return self._part_expected(MATRIX_SWEEP, formats)

    def matrix_sweep(self, dev: int = 0, formats=None, blocks: int = 0, inject: tuple | None = None,
                     max_rounds: int = 4) -> dict:
        """k_matrix_sweep: every selected matrix format (None: all) run on
        every CU a workgroup lands on. `inject` = (xcd, cu key or None for
        every CU of that XCD, [format names]): those workgroups flip one bit
        of one result element of those formats (tests the comparator on a
        healthy GPU). `blocks` 0: 4 per CU.

        Relaunched while some CU has not been seen, as cu_sweep does. Returns
        {"records": [...], "summary": summarize_matrix_sweep(...) plus rounds,
        ms, blocks, formats}."""
        return self._part_sweep(MATRIX_SWEEP, summarize_matrix_sweep, dev, blocks, formats, inject, max_rounds)

    # -------------------------------------------------- register-file sweep
    def regfile_sweep_expected(self, seed: int = REGFILE_SEED) -> int:
        """The workgroup digest a healthy CU leaves, computed on the host."""
        out = ctypes.c_uint32()
        self._call("regfile_sweep", "regfile_sweep_expected", seed, ctypes.byref(out))
        return int(out.value)

    def regfile_sweep_info(self, dev: int = 0) -> dict:
        """What the runtime reports for k_regfile_sweep: `num_regs`,
        `scratch_bytes` per lane and `blocks_per_cu` (256-thread workgroups
        that fit on a CU at once)."""
        return self._sweep_info("regfile_sweep", dev, ("num_regs", "scratch_bytes", "blocks_per_cu"))

    def regfile_sweep(self, dev: int = 0, blocks: int = 0, seed: int = REGFILE_SEED, inject: tuple | None = None,
                      poison: tuple | None = None, max_rounds: int = 4) -> dict:
        """k_regfile_sweep: all 512 VGPR/AGPR entries of every lane of every
        SIMD written and read back in both polarities on every CU a workgroup
        lands on. `inject` = (xcd, cu key or None for every CU of that XCD,
        cell 0..511, bit 0..31): those workgroups flip that bit of what they
        read back from that cell in pass 0 (tests the comparator on a healthy
        GPU). `poison` = (xcd, cu key or None, VGPR 0..255): those workgroups
        complement that physical register through the index mode between pass
        0's writes and reads (tests that the read-back names the register it
        reads). Given together they select the same workgroups. `blocks` 0:
        4 per CU.

        Relaunched while some CU has not been seen, as cu_sweep does. Returns
        {"records": [...], "summary": summarize_regfile_sweep(...) plus rounds,
        ms, blocks, seed}."""
        (ix, ic), ir, ib, pr = _inject_target(inject), -1, 0, -1
        if inject is not None:
            ir, ib = int(inject[2]), int(inject[3])
        if poison is not None:
            px, pc = _inject_target(poison)
            if inject is not None and (px, pc) != (ix, ic):
                raise ValueError("regfile_sweep: inject and poison select different workgroups")
            ix, ic, pr = px, pc, int(poison[2])

        def decode(w, expected):
            rec = {"xcd": w[0], "cu": w[1], "simd_mask": w[2], "fail": w[3], "bad_vgpr": w[4], "bad_agpr": w[5],
                   "first": w[6], "flip": w[7], "digest": w[8], "bad_simds": w[9]}
            # With no cell named, a digest that differs is a failure of both files.
            if not rec["fail"] and rec["digest"] != expected:
                rec["fail"] = 3
            return rec

        out = self._sweep_until_covered(
            "regfile_sweep", dev, blocks, max_rounds, REGFILE_RECORD_WORDS,
            lambda nb, *out: self.lib.xs_regfile_sweep(dev, nb, seed, ix, ic, ir, ib, pr, *out),
            lambda: self.regfile_sweep_expected(seed), decode, summarize_regfile_sweep)
        out["summary"].update(seed=seed)
        return out

    # ----------------------------------------------------------- lane sweep
    def lane_paths(self) -> list[str]:
        """Path names of the lane sweep; the index is the path's bit."""
        return self._part_names(LANE_SWEEP)

    def _lane_mask(self, paths) -> int:
        return self._part_mask(LANE_SWEEP, paths)

    def lane_shape(self, path: str) -> dict:
        """`steps` of one path and the `words` every thread receives per step."""
        out = self._part_shape(LANE_SWEEP, path, 2)
        return {"steps": out[0], "words": out[1]}

    def lane_probe(self, dev: int, path: str, seed: int = LANE_SEED):
        """k_lane_probe: one workgroup runs `path` and stores every value it
        received: uint32 [steps, words, 256] (thread = 64 x wave + lane)."""
        import numpy as np

        sh = self.lane_shape(path)
        out = np.zeros((sh["steps"], sh["words"], LANE_BLOCK), np.uint32)
        self._call("lane_sweep", "lane_probe", dev, self.lane_paths().index(path), seed, out.ctypes.data, out.size)
        return out

    def lane_sweep_expected(self, paths=None, seed: int = LANE_SEED) -> dict:
        """The workgroup digest a healthy CU leaves per selected path,
        computed on the host from the lane maps."""
        return self._part_expected(LANE_SWEEP, paths, seed)

    def lane_sweep_info(self, dev: int = 0) -> dict:
        """What the runtime reports for k_lane_sweep: `num_regs`,
        `scratch_bytes` per lane, `lds_bytes` per workgroup and `blocks_per_cu`
        (workgroups that fit on a CU at once)."""
        return self._sweep_info("lane_sweep", dev, ("num_regs", "scratch_bytes", "lds_bytes", "blocks_per_cu"))

    def lane_sweep(self, dev: int = 0, blocks: int = 0, paths=None, seed: int = LANE_SEED,
                   inject: tuple | None = None, max_rounds: int = 4) -> dict:
        """k_lane_sweep: every selected path (None: all) of the cross-lane
        network and the LDS access paths run on every CU a workgroup lands on.
        `inject` = (xcd, cu key or None for every CU of that XCD, [path
        names]): those workgroups flip one bit of one received value of those
        paths (tests the comparator on a healthy GPU). `blocks` 0: 4 per CU.

        Relaunched while some CU has not been seen, as cu_sweep does. Returns
        {"records": [...], "summary": summarize_lane_sweep(...) plus rounds,
        ms, blocks, paths, seed}."""
        return self._part_sweep(LANE_SWEEP, summarize_lane_sweep, dev, blocks, paths, inject, max_rounds, (seed,),
                                {"seed": seed})

    # --------------------------------------------------------- memory sweep
    def mem_routes(self) -> list[str]:
        """Route names of the memory-path sweep; the index is the route's bit."""
        return self._part_names(MEM_SWEEP)

    def mem_shape(self, route: str) -> dict:
        """`steps` of one route and the `words` every thread receives per step."""
        out = self._part_shape(MEM_SWEEP, route, 2)
        return {"steps": out[0], "words": out[1]}

    def mem_probe(self, dev: int, route: str, seed: int = MEM_SEED):
        """k_mem_probe: one workgroup runs `route` and stores every value it
        received: uint32 [steps, words, 256] (thread = 64 x wave + lane)."""
        import numpy as np

        sh = self.mem_shape(route)
        out = np.zeros((sh["steps"], sh["words"], MEM_BLOCK), np.uint32)
        self._call("mem_sweep", "mem_probe", dev, self.mem_routes().index(route), seed, out.ctypes.data, out.size,
                   wording=MEM_WORDING)
        return out

    def mem_sweep_expected(self, routes=None, seed: int = MEM_SEED) -> dict:
        """The workgroup digest a healthy CU leaves per selected route,
        computed on the host from the ISA's rules and the address maps."""
        return self._part_expected(MEM_SWEEP, routes, seed)

    def mem_sweep_info(self, dev: int = 0) -> dict:
        """What the runtime reports for k_mem_sweep: `num_regs`, `scratch_bytes`
        per lane, `lds_bytes` per workgroup, `blocks_per_cu` (workgroups that
        fit on a CU at once), and the `arena_bytes` of HBM a workgroup's slab
        and its guard bands take."""
        return self._sweep_info("mem_sweep", dev,
                                ("num_regs", "scratch_bytes", "lds_bytes", "blocks_per_cu", "arena_bytes"))

    def mem_sweep(self, dev: int = 0, blocks: int = 0, routes=None, seed: int = MEM_SEED,
                  inject: tuple | None = None, max_rounds: int = 4) -> dict:
        """k_mem_sweep: every selected route (None: all) between a wave's
        registers and HBM run on every CU a workgroup lands on, each workgroup
        in a slab of its own (`mem_sweep_info()["arena_bytes"]` per workgroup,
        held while the launch runs). `inject` = (xcd, cu key or None for every
        CU of that XCD, [route names]): those workgroups flip one bit of one
        received value of those routes (tests the comparator on a healthy
        GPU). `blocks` 0: 4 per CU.

        Raises ProbeError with rc MEM_UNSWEPT when the arena could not be had
        (nothing ran) and MEM_STRAY_STORE when a guard band was written.
        Relaunched while some CU has not been seen, as cu_sweep does. Returns
        {"records": [...], "summary": summarize_mem_sweep(...) plus rounds,
        ms, blocks, routes, seed}."""
        return self._part_sweep(MEM_SWEEP, summarize_mem_sweep, dev, blocks, routes, inject, max_rounds, (seed,),
                                {"seed": seed}, wording=MEM_WORDING)

    # --------------------------------------------------------- scalar sweep
    def scalar_parts(self) -> list[str]:
        """Part names of the scalar sweep; the index is the part's bit."""
        return self._part_names(SCALAR_SWEEP)

    def scalar_shape(self, part: str) -> dict:
        """`steps` of one part and the `words` every thread holds after it."""
        out = self._part_shape(SCALAR_SWEEP, part, 2)
        return {"steps": out[0], "words": out[1]}

    def scalar_probe(self, dev: int, part: str, seed: int = SCALAR_SEED, raw: bool = False):
        """k_scalar_probe: one workgroup of 1,024 threads runs `part` and stores
        every word it received: uint32 [words, 1024] (thread = 64 x wave +
        lane). With `raw`, (that, the HW_REG_GPR_ALLOC word of every thread,
        the HW_REG_HW_ID word of every thread): where each wave ran and which
        SGPRs it was given, as the hardware reports them."""
        import numpy as np

        words = self.scalar_shape(part)["words"]
        out = np.zeros((words + 2, SCALAR_BLOCK), np.uint32)
        self._call("scalar_sweep", "scalar_probe", dev, self.scalar_parts().index(part), seed, out.ctypes.data,
                   out.size)
        return (out[:words], out[words], out[words + 1]) if raw else out[:words]

    def scalar_sweep_expected(self, parts=None, seed: int = SCALAR_SEED) -> dict:
        """The workgroup digest a healthy CU leaves per selected part, computed
        on the host from the ISA's definitions."""
        return self._part_expected(SCALAR_SWEEP, parts, seed)

    def scalar_sweep_info(self, dev: int = 0) -> dict:
        """What the runtime reports for k_scalar_sweep: `num_regs`,
        `scratch_bytes` per lane, `lds_bytes` per workgroup, `blocks_per_cu`
        (workgroups that fit on a CU at once)."""
        return self._sweep_info("scalar_sweep", dev, ("num_regs", "scratch_bytes", "lds_bytes", "blocks_per_cu"))

    def scalar_sweep(self, dev: int = 0, blocks: int = 0, parts=None, seed: int = SCALAR_SEED,
                     inject: tuple | None = None, max_rounds: int = 4) -> dict:
        """k_scalar_sweep: every selected part (None: all) of the scalar unit
        run on every CU a workgroup lands on. `inject` = (xcd, cu key or None
        for every CU of that XCD, [part names]): those workgroups flip one bit
        of one received value of those parts (tests the comparator on a healthy
        GPU). `blocks` 0: 4 per CU. It allocates nothing but its records.

        Relaunched while some CU has not been seen, as cu_sweep does. Returns
        {"records": [...], "summary": summarize_scalar_sweep(...) plus rounds,
        ms, blocks, parts, seed}."""
        return self._part_sweep(SCALAR_SWEEP, summarize_scalar_sweep, dev, blocks, parts, inject, max_rounds,
                                (seed,), {"seed": seed}, tail=scalar_record_tail)

    # ------------------------------------------------------ consensus sweep
    def consensus_parts(self) -> list[str]:
        """Part names of the consensus sweep; the index is the part's bit."""
        return self._part_names(CONSENSUS_SWEEP)

    def consensus_shape(self, part: str) -> dict:
        """`steps` of one part, the result `words` every thread gets per round
        and the `operand_words` it is given per round."""
        out = self._part_shape(CONSENSUS_SWEEP, part, 3)
        return {"steps": out[0], "words": out[1], "operand_words": out[2]}

    def consensus_operands(self, part: str, seed: int = CONSENSUS_SEED, rounds: int = CONSENSUS_ROUNDS):
        """The operand words of one workgroup, computed on the host: uint32
        [rounds, operand_words, 256], per step the words of operand 0, then 1,
        2 and 3, in the step table's order. No device call."""
        import numpy as np

        out = np.zeros((max(int(rounds), 0), self.consensus_shape(part)["operand_words"], CONSENSUS_BLOCK), np.uint32)
        self._call("consensus_sweep", "consensus_operands", self.consensus_parts().index(part), seed, out.ctypes.data,
                   out.size)
        return out

    def consensus_probe(self, dev: int, part: str, seed: int = CONSENSUS_SEED, rounds: int = CONSENSUS_ROUNDS):
        """k_consensus_probe: one workgroup runs `part` and stores every word
        it received: uint32 [rounds, words, 256] (thread = 64 x wave + lane)."""
        import numpy as np

        out = np.zeros((max(int(rounds), 0), self.consensus_shape(part)["words"], CONSENSUS_BLOCK), np.uint32)
        self._call("consensus_sweep", "consensus_probe", dev, self.consensus_parts().index(part), seed,
                   out.ctypes.data, out.size)
        return out

    def consensus_sweep_info(self, dev: int = 0) -> dict:
        """What the runtime reports for k_consensus_sweep: `num_regs`,
        `scratch_bytes` per lane, `lds_bytes` per workgroup and `blocks_per_cu`
        (workgroups that fit on a CU at once)."""
        return self._sweep_info("consensus_sweep", dev, ("num_regs", "scratch_bytes", "lds_bytes", "blocks_per_cu"))

    def consensus_sweep(self, dev: int = 0, parts=None, blocks: int = 0, seed: int = CONSENSUS_SEED,
                        rounds: int = CONSENSUS_ROUNDS, inject: tuple | None = None, inject_parts=None,
                        max_rounds: int = 4) -> dict:
        """k_consensus_sweep: every selected part (None: all) runs `rounds`
        operand sets per step on every CU a workgroup lands on and leaves one
        digest per part; the device judges nothing. The verdict is the vote of
        vote_consensus: a CU fails a part when its records disagree among
        themselves or with the digest that more than half of the CUs hold.
        `inject` = (xcd, cu key or None for every CU of that XCD[, part
        names]) with `inject_parts` (default: the names in `inject`, else all
        selected): those workgroups flip one bit of one result of those parts
        (tests the vote on a healthy GPU). `blocks` 0: 4 per CU.

        Relaunched (at most `max_rounds` launches) while some CU has not been
        seen, as cu_sweep does. Returns {"records": [...], "summary":
        summarize_consensus_sweep(...) plus rounds (launches), ms, blocks,
        parts, operand_rounds, seed}."""
        kind = CONSENSUS_SWEEP
        names = self._part_names(kind)
        mask = self._part_mask(kind, parts)
        selected = [f for i, f in enumerate(names) if mask >> i & 1]
        ix, ic = _inject_target(inject)
        if inject is None:
            im = 0
        else:
            chosen = inject_parts if inject_parts is not None else inject[2] if len(inject) > 2 else selected
            im = self._part_mask(kind, chosen)
        out = self._sweep_until_covered(
            "consensus_sweep", dev, blocks, max_rounds, kind.record_words,
            lambda nb, *out: self.lib.xs_consensus_sweep(dev, nb, mask, seed, rounds, ix, ic, im, *out),
            lambda: {},  # no host digests: the vote is the reference
            lambda w, _: {"xcd": w[0], "cu": w[1], "simd_mask": w[2], "fail": w[3],
                          "digests": dict(zip(names, w[kind.digests:kind.digests + len(names)]))},
            lambda records, cus: summarize_consensus_sweep(records, cus, names, selected))
        out["summary"].update(seed=seed, parts=selected, operand_rounds=rounds)
        return out

    # ---------------------------------------------------------- fetch sweep
    def fetch_parts(self) -> list[str]:
        """Part names of the fetch sweep; the index is the part's bit."""
        return self._part_names(FETCH_SWEEP)

    def fetch_shape(self, part: str, rounds: int = FETCH_ROUNDS) -> dict:
        """`rows` of 256 words one part hands over at `rounds`: `fixed_rows`
        whatever the rounds plus `rows_per_round` for each."""
        out = self._part_shape(FETCH_SWEEP, part, 2)
        return {"fixed_rows": out[0], "rows_per_round": out[1], "rows": out[0] + out[1] * max(int(rounds), 0)}

    def fetch_probe(self, dev: int, parts=None, seed: int = FETCH_SEED, rounds: int = FETCH_ROUNDS) -> dict:
        """k_fetch_probe: one workgroup runs the selected parts (one name,
        several, None: all) in one launch and stores every word it hands over:
        {part: uint32 [rows, 256]} (thread = 64 x wave + lane)."""
        import numpy as np

        names = self.fetch_parts()
        mask = self._part_mask(FETCH_SWEEP, parts)
        selected = [f for i, f in enumerate(names) if mask >> i & 1]
        rows = [self.fetch_shape(f, rounds)["rows"] for f in selected]
        out = np.zeros((sum(rows), FETCH_BLOCK), np.uint32)
        self._call("fetch_sweep", "fetch_probe", dev, mask, seed, rounds, out.ctypes.data, out.size)
        ends = np.cumsum(rows)
        return {f: out[e - n:e] for f, n, e in zip(selected, rows, ends)}

    def fetch_probe_clocks(self, dev: int, repeats: int = 8):
        """k_fetch_probe's timing mode: for k = 1..32 one workgroup calls the
        stream segments 0..k-1 (8 k KiB of code) once untimed and `repeats`
        times between two s_memtime reads. Returns float64 [32, 256]: every
        thread's clocks per byte of code at each footprint."""
        import numpy as np

        out = np.zeros((FETCH_SEGMENTS, FETCH_BLOCK), np.uint32)
        self._call("fetch_sweep", "fetch_probe", dev, 1 << len(self.fetch_parts()), 0, repeats, out.ctypes.data,
                   out.size)
        nbytes = 8192.0 * repeats * np.arange(1, FETCH_SEGMENTS + 1)
        return out / nbytes[:, None]

    def fetch_sweep_expected(self, parts=None, seed: int = FETCH_SEED, rounds: int = FETCH_ROUNDS) -> dict:
        """The workgroup digest a healthy CU leaves per selected part, computed
        on the host from the region and step tables."""
        return self._part_expected(FETCH_SWEEP, parts, seed, rounds)

    def fetch_sweep_info(self, dev: int = 0) -> dict:
        """What the runtime reports for k_fetch_sweep: `num_regs`,
        `scratch_bytes` per lane, `lds_bytes` per workgroup, `blocks_per_cu`
        (workgroups that fit on a CU at once)."""
        return self._sweep_info("fetch_sweep", dev, ("num_regs", "scratch_bytes", "lds_bytes", "blocks_per_cu"))

    def fetch_sweep(self, dev: int = 0, blocks: int = 0, parts=None, seed: int = FETCH_SEED,
                    rounds: int = FETCH_ROUNDS, inject: tuple | None = None, max_rounds: int = 4) -> dict:
        """k_fetch_sweep: every selected part (None: all) of the instruction
        fetch path run on every CU a workgroup lands on; `rounds` multiplies
        the loop trips and the call rounds. `inject` = (xcd, cu key or None for
        every CU of that XCD, [part names]): those workgroups flip one bit of
        one word of those parts (tests the comparator on a healthy GPU).
        `blocks` 0: 4 per CU. It allocates nothing but its records.

        Relaunched (at most `max_rounds` launches) while some CU has not been
        seen, as cu_sweep does. Returns {"records": [...], "summary":
        summarize_fetch_sweep(...) plus rounds (launches), ms, blocks, parts,
        code_rounds, seed}."""
        out = self._part_sweep(FETCH_SWEEP, summarize_fetch_sweep, dev, blocks, parts, inject, max_rounds,
                               (seed, rounds), {"seed": seed})
        out["summary"].update(code_rounds=rounds)
        return out

    # ----------------------------------------------------------- VALU sweep
    def valu_units(self) -> list[str]:
        """Unit names of the VALU sweep; the index is the unit's bit."""
        return self._part_names(VALU_SWEEP)

    def _valu_mask(self, units) -> int:
        return self._part_mask(VALU_SWEEP, units)

    def valu_steps(self, unit: str | None = None) -> list[str]:
        """Step names of one unit in order; None: of every unit, in the order
        of the record's step bits."""
        if unit is None:
            return [s for u in self.valu_units() for s in self.valu_steps(u)]
        self._valu_mask([unit])
        return self.lib.xs_valu_steps(self.valu_units().index(unit)).decode().split(",")

    def valu_shape(self, unit: str) -> dict:
        """`steps` of one unit and the result `words` every thread gets per round."""
        out = self._part_shape(VALU_SWEEP, unit, 2)
        return {"steps": out[0], "words": out[1]}

    def _valu_dump(self, what: str, before: tuple, unit: str, seed: int, rounds: int):
        import numpy as np

        sh = self.valu_shape(unit)
        out = np.zeros((max(int(rounds), 0), sh["words"], VALU_BLOCK), np.uint32)
        self._call("valu_sweep", what, *before, self.valu_units().index(unit), seed, rounds, out.ctypes.data, out.size)
        return out

    def valu_expected(self, unit: str, seed: int = VALU_SEED, rounds: int = VALU_ROUNDS):
        """What every thread of a healthy SIMD gets from `unit`, computed on
        the host: uint32 [rounds, words, 256]. No device call."""
        return self._valu_dump("valu_expected", (), unit, seed, rounds)

    def valu_probe(self, dev: int, unit: str, seed: int = VALU_SEED, rounds: int = VALU_ROUNDS):
        """k_valu_probe: one workgroup runs `unit` and stores every result:
        uint32 [rounds, words, 256] (thread = 64 x wave + lane)."""
        return self._valu_dump("valu_probe", (dev,), unit, seed, rounds)

    def valu_sweep_expected(self, units=None, seed: int = VALU_SEED, rounds: int = VALU_ROUNDS) -> dict:
        """The workgroup digest a healthy CU leaves per selected unit,
        computed on the host from the step table."""
        return self._part_expected(VALU_SWEEP, units, seed, rounds)

    def valu_sweep_info(self, dev: int = 0) -> dict:
        """What the runtime reports for k_valu_sweep: `num_regs`,
        `scratch_bytes` per lane, `lds_bytes` per workgroup and `blocks_per_cu`
        (workgroups that fit on a CU at once)."""
        return self._sweep_info("valu_sweep", dev, ("num_regs", "scratch_bytes", "lds_bytes", "blocks_per_cu"))

    def valu_sweep(self, dev: int = 0, blocks: int = 0, units=None, seed: int = VALU_SEED,
                   rounds: int = VALU_ROUNDS, inject: tuple | None = None, max_rounds: int = 4) -> dict:
        """k_valu_sweep: every selected unit (None: all) of the vector ALU
        runs `rounds` operand sets per step on every CU a workgroup lands on.
        `inject` = (xcd, cu key or None for every CU of that XCD, [unit
        names]): those workgroups flip one bit of one result of those units
        (tests the comparator on a healthy GPU). `blocks` 0: 4 per CU.

        Relaunched (at most `max_rounds` launches) while some CU has not been
        seen, as cu_sweep does. Returns {"records": [...], "summary":
        summarize_valu_sweep(...) plus rounds (launches), ms, blocks, units,
        operand_rounds, seed}."""
        out = self._part_sweep(VALU_SWEEP, summarize_valu_sweep, dev, blocks, units, inject, max_rounds,
                               (seed, rounds), {"seed": seed}, self.valu_steps())
        out["summary"].update(operand_rounds=rounds)
        return out

    # ------------------------------------------------------------ HBM sweep
    def hbm_sweep_pattern(self, first_vec: int, nvec: int, seed: int = HBM_SWEEP_SEED, inverted: bool = False):
        """The sweep's pattern for 16-byte vectors [first_vec, first_vec +
        nvec), computed on the host: uint32 [nvec, 4]. No device call."""
        import numpy as np

        out = np.zeros((nvec, 4), np.uint32)
        self._call("hbm_sweep", "hbm_sweep_pattern", first_vec, nvec, seed, int(inverted), out.ctypes.data,
                   wording=HBM_WORDING)
        return out

    def hbm_sweep_op(self, buf, pass_: int, first_vec: int = 0, seed: int = HBM_SWEEP_SEED,
                     grid: int = 0) -> dict | None:
        """One pass of the HBM sweep over the device tensor `buf`, whose first
        16-byte vector has global index `first_vec`: 0 fills the pattern, 1
        checks it and writes the complement of the expected value, 2 checks
        the complement. `grid` > 0: that many workgroups instead of 8 per CU.
        Passes 1 and 2 return the launch's result: vectors_read, fold,
        bad_vectors, bad_bits, one_to_zero, zero_to_one, flip_or [4],
        reader_xcd_mask, log_claims and log (at most 32 entries). Size and
        alignment are the C ABI's to refuse (ProbeError, rc -1000 / -1001)."""
        p, n = self._dev_buf(buf, "buf", granule=0)
        res = _HbmSweepResult()
        self._call("hbm_sweep", "hbm_sweep_op", buf.device.index or 0, pass_, p, n, first_vec, seed, grid,
                   ctypes.addressof(res) if pass_ != 0 else None, wording=HBM_WORDING)
        if pass_ == 0:
            return None
        fold = 0
        for st in res.stripe:
            fold ^= int(st.fold)
        return {"vectors_read": sum(int(st.vectors_read) for st in res.stripe), "fold": fold,
                "bad_vectors": int(res.bad_vectors),
                "bad_bits": int(res.bad_bits), "one_to_zero": int(res.one_to_zero),
                "zero_to_one": int(res.zero_to_one), "flip_or": [int(w) for w in res.flip_or],
                "reader_xcd_mask": int(res.reader_xcd_mask), "log_claims": int(res.log_claims),
                "log": _hbm_log(res.log[:min(int(res.log_claims), HBM_SWEEP_LOG_CAP)])}

    def hbm_sweep(self, dev: int = 0, nbytes: int = 0, chunk_bytes: int = 1 << 30, seed: int = HBM_SWEEP_SEED,
                  inject: tuple | None = None) -> dict:
        """The whole HBM sweep: fill, verify + invert, verify over `nbytes` of
        HBM (0: all free HBM less a 2 GiB reserve) held in `chunk_bytes`
        allocations until the last pass is done. `inject` = (global vector,
        word 0..3, bit mask, after pass 0 or 1): the host flips those bits in
        the sweep's own buffer between passes (tests the comparator on healthy
        memory). Raises ProbeError with rc HBM_UNSWEPT when no memory could be
        had: nothing was tested. Returns {"raw": the C summary as a dict,
        "summary": summarize_hbm_sweep(raw)}."""
        iv, iw, im, ip = HBM_NO_INJECT, 0, 0, 0
        if inject is not None:
            iv, iw, im, ip = (int(x) for x in inject)
        s = _HbmSweepSummary()
        log = (_HbmLogEntry * HBM_SWEEP_LOG_CAP)()
        self._call("hbm_sweep", "hbm_sweep", dev, nbytes, chunk_bytes, seed, iv, iw, im, ip, ctypes.addressof(s),
                   ctypes.addressof(log), wording=HBM_WORDING)
        raw = {"bytes_requested": int(s.bytes_requested), "bytes_tested": int(s.bytes_tested),
               "chunk_bytes": int(s.chunk_bytes), "chunks": int(s.chunks), "short": bool(s.short),
               "vectors_read": int(s.vectors_read), "fold": [int(f) for f in s.fold],
               "bad_vectors": int(s.bad_vectors),
               "bad_bits": int(s.bad_bits), "one_to_zero": int(s.one_to_zero), "zero_to_one": int(s.zero_to_one),
               "flip_or": [int(w) for w in s.flip_or], "reader_xcd_mask": int(s.reader_xcd_mask),
               "ms": [float(t) for t in s.ms], "bad_chunk_count": int(s.bad_chunks),
               "bad_chunks": {int(b.chunk): int(b.bad_vectors)
                              for b in s.bad_chunk[:min(int(s.bad_chunks), HBM_SWEEP_BAD_CHUNKS)]},
               "log": _hbm_log(log[:int(s.log_entries)])}
        return {"raw": raw, "summary": summarize_hbm_sweep(raw)}


def summarize_hbm_sweep(raw: dict) -> dict:
    """The verdict of one HBM sweep from xs_hbm_sweep's counters (`raw`:
    bytes_tested, short, vectors_read, bad_vectors, bad_bits, one_to_zero,
    zero_to_one, flip_or [4 words, word 0 = bytes 0..3 of a vector],
    reader_xcd_mask, bad_chunks {chunk: bad vectors}, log, ms [3]).

    `from_dram`: the sweep was large enough (1 GiB, 4x the Infinity Cache)
    that its reads came from HBM. `flip_mask`: the 128 bits of a vector that
    flipped anywhere, as hex (bit 0 = lowest bit of byte 0). `faults`: the
    logged vectors by index, each with its byte offset into the sweep and the
    flipped bits (0..127) by direction; at most 32 are logged, `bad_vectors`
    counts them all. `GBps`: bytes moved over time per pass (pass 1 reads and
    writes). `reader_xcds` are the XCDs whose waves read a bad vector, not
    where the memory sits."""
    tested = int(raw["bytes_tested"])
    flip = 0
    for j, w in enumerate(raw.get("flip_or", (0, 0, 0, 0))):
        flip |= int(w) << (32 * j)
    faults = []
    for e in sorted(raw.get("log", ()), key=lambda e: (int(e["v"]), int(e["pass"]))):
        exp = sum(int(w) << (32 * j) for j, w in enumerate(e["expected"]))
        act = sum(int(w) << (32 * j) for j, w in enumerate(e["actual"]))
        d = exp ^ act
        faults.append({"v": int(e["v"]), "offset": int(e["v"]) * 16, "pass": int(e["pass"]), "xcd": int(e["xcd"]),
                       "expected": [int(w) for w in e["expected"]], "actual": [int(w) for w in e["actual"]],
                       "bits": [b for b in range(128) if d >> b & 1],
                       "one_to_zero": [b for b in range(128) if (d & exp) >> b & 1],
                       "zero_to_one": [b for b in range(128) if (d & ~exp) >> b & 1]})
    ms = [float(t) for t in raw.get("ms", (0.0, 0.0, 0.0))]
    moved = (tested, 2 * tested, tested)
    mask = int(raw.get("reader_xcd_mask", 0))
    bad = int(raw["bad_vectors"])
    return {"bytes_tested": tested, "short": bool(raw.get("short", False)), "from_dram": tested >= HBM_FROM_DRAM_BYTES,
            "vectors_read": int(raw["vectors_read"]), "bad_vectors": bad, "bad_bits": int(raw["bad_bits"]),
            "one_to_zero": int(raw["one_to_zero"]), "zero_to_one": int(raw["zero_to_one"]),
            "flip_mask": f"{flip:032x}", "reader_xcds": [x for x in range(32) if mask >> x & 1],
            "bad_chunks": {int(c): int(n) for c, n in sorted(raw.get("bad_chunks", {}).items())},
            "faults": faults, "unlogged": max(0, bad - len(faults)), "ms": [round(t, 4) for t in ms],
            "GBps": [round(b / (t * 1e-3) / 1e9, 1) if t > 0 else 0.0 for b, t in zip(moved, ms)],
            "healthy": bad == 0}


def summarize_sweep(records: list[dict], compute_units: int) -> dict:
    """Aggregate k_cu_sweep records ({"xcd", "cu", "fail", ...}; one per
    workgroup, a CU may appear many times) into a verdict per XCD.

    A CU is failed when any of its records has a fail bit; an XCD is bad when
    it has a failed CU. CUs no workgroup reached are `uncovered`, never failed
    (other tenants may hold them)."""
    seen: dict[int, set[int]] = {}
    failed: dict[int, dict[int, int]] = {}
    for r in records:
        x, c = int(r["xcd"]), int(r["cu"])
        seen.setdefault(x, set()).add(c)
        if int(r.get("fail", 0)):
            failed.setdefault(x, {})[c] = failed.get(x, {}).get(c, 0) | int(r["fail"])
    expected = compute_units // len(seen) if seen else 0
    xcds, uncovered = {}, {}
    for x in sorted(seen):
        bits = 0
        for b in failed.get(x, {}).values():
            bits |= b
        xcds[x] = {"cus_seen": len(seen[x]), "cus_expected": expected, "failed_cus": sorted(failed.get(x, {})),
                   "fail_bits": bits}
        uncovered[x] = max(0, expected - len(seen[x]))
    return {"xcds": xcds, "bad_xcds": sorted(failed), "covered": bool(seen) and not any(uncovered.values()),
            "uncovered": uncovered, "cus_seen": sum(len(v) for v in seen.values())}


def _name_fail_bits(s: dict, key: str, names: list[str]) -> dict:
    """Adds to a summarize_sweep verdict, under `key`, the names of the fail
    bits that are set (`names` in bit order): per XCD and overall."""
    def named(bits: int) -> list[str]:
        return [f for b, f in enumerate(names) if bits >> b & 1]

    every = 0
    for v in s["xcds"].values():
        v[key] = named(v["fail_bits"])
        every |= v["fail_bits"]
    s[key] = named(every)
    return s


def summarize_matrix_sweep(records: list[dict], compute_units: int, formats: list[str]) -> dict:
    """summarize_sweep over k_matrix_sweep records, whose fail bits are format
    bits (`formats` names them in bit order): adds `failed_formats` per XCD
    and overall."""
    return _name_fail_bits(summarize_sweep(records, compute_units), MATRIX_SWEEP.summary_key, formats)


def summarize_regfile_sweep(records: list[dict], compute_units: int) -> dict:
    """summarize_sweep over k_regfile_sweep records, whose fail bits are
    register files (bit 0 VGPR, bit 1 AGPR). Adds per XCD and overall:
    `failed_files`, `bad_cells` (mis-compared (cell, lane) pairs; of the worst
    record of a CU that ran more than one workgroup) and `flip_mask` (hex, the
    bits that flipped); per XCD also `bad_simds` = {cu: [SIMD id, ...]}."""
    s = _name_fail_bits(summarize_sweep(records, compute_units), "failed_files", REGFILE_FILES)
    cells: dict[tuple[int, int], int] = {}
    flips: dict[int, int] = {}
    simds: dict[int, dict[int, int]] = {}
    for r in records:
        if not int(r.get("fail", 0)):
            continue
        x, c = int(r["xcd"]), int(r["cu"])
        cells[x, c] = max(cells.get((x, c), 0), int(r.get("bad_vgpr", 0)) + int(r.get("bad_agpr", 0)))
        flips[x] = flips.get(x, 0) | int(r.get("flip", 0))
        per = simds.setdefault(x, {})
        per[c] = per.get(c, 0) | int(r.get("bad_simds", 0))
    for x, v in s["xcds"].items():
        v["bad_cells"] = sum(n for (xx, _), n in cells.items() if xx == x)
        v["flip_mask"] = f"0x{flips.get(x, 0):08x}"
        v["bad_simds"] = {c: [i for i in range(4) if m >> i & 1] for c, m in sorted(simds.get(x, {}).items())}
    s["bad_cells"] = sum(cells.values())
    flip = 0
    for f in flips.values():
        flip |= f
    s["flip_mask"] = f"0x{flip:08x}"
    return s


def summarize_lane_sweep(records: list[dict], compute_units: int, paths: list[str]) -> dict:
    """summarize_sweep over k_lane_sweep records, whose fail bits are path
    bits (`paths` names them in bit order): adds `failed_paths` per XCD and
    overall."""
    return _name_fail_bits(summarize_sweep(records, compute_units), LANE_SWEEP.summary_key, paths)


def summarize_mem_sweep(records: list[dict], compute_units: int, routes: list[str]) -> dict:
    """summarize_sweep over k_mem_sweep records, whose fail bits are route
    bits (`routes` names them in bit order): adds `failed_routes` per XCD and
    overall."""
    return _name_fail_bits(summarize_sweep(records, compute_units), MEM_SWEEP.summary_key, routes)


def scalar_record_tail(w) -> dict:
    """`gpr_alloc` of a k_scalar_sweep record: per SIMD, (OR, AND) of the raw
    HW_REG_GPR_ALLOC words its waves read; (0, 0xffffffff) for a SIMD without a
    wave. The register's layout on the MI355X is not the documented GFX9 one,
    so nothing is derived from it (csrc/hip/scalar_sweep.hip)."""
    c = w[SCALAR_COVER_WORD:SCALAR_COVER_WORD + 8]
    return {"gpr_alloc": [(int(c[2 * q]), ~int(c[2 * q + 1]) & 0xFFFFFFFF) for q in range(4)]}


def summarize_scalar_sweep(records: list[dict], compute_units: int, parts: list[str]) -> dict:
    """summarize_sweep over k_scalar_sweep records, whose fail bits are part
    bits (`parts` names them in bit order): adds `failed_parts` per XCD and
    overall. There is no figure for the SGPR rows reached: see scalar_record_tail."""
    return _name_fail_bits(summarize_sweep(records, compute_units), SCALAR_SWEEP.summary_key, parts)


def summarize_fetch_sweep(records: list[dict], compute_units: int, parts: list[str]) -> dict:
    """summarize_sweep over k_fetch_sweep records, whose fail bits are part
    bits (`parts` names them in bit order): adds `failed_parts` per XCD and
    overall. The record names the CU that ran, not the neighbour that shares
    its instruction cache."""
    return _name_fail_bits(summarize_sweep(records, compute_units), FETCH_SWEEP.summary_key, parts)


def vote_consensus(records: list[dict], parts: list[str]) -> dict:
    """The vote over k_consensus_sweep records ({"xcd", "cu", "digests": {part:
    digest}, ...}; a CU may appear many times) on the selected `parts`. Per part:
    a CU votes once, with the digest all its records share; a CU whose records
    disagree casts no vote and fails the part. The consensus is the digest held
    by strictly more than half of the CUs seen (those without a vote count in
    the denominator); a CU that does not hold it fails the part. With fewer
    than 3 CUs seen or no strict majority the part is undecided and nobody
    fails it. A part outside `parts` is never judged.

    Returns {"fail": one word of fail bits per record, in order (bit = the
    part's position in the record's digests), "consensus": {part: "0x..."} of
    the decided parts, "undecided": [part, ...]}. Nothing is changed in place."""
    fail = [0] * len(records)
    by_cu: dict[tuple[int, int], list[int]] = {}
    for i, r in enumerate(records):
        by_cu.setdefault((int(r["xcd"]), int(r["cu"])), []).append(i)
    consensus: dict[str, str] = {}
    undecided: list[str] = []
    for part in parts:
        votes: dict[tuple[int, int], int | None] = {}
        for cu, rows in by_cu.items():
            held = {int(records[i]["digests"][part]) for i in rows}
            votes[cu] = held.pop() if len(held) == 1 else None
        count: dict[int, int] = {}
        for v in votes.values():
            if v is not None:
                count[v] = count.get(v, 0) + 1
        top = max(count, key=count.get) if count else None
        if len(votes) < 3 or top is None or 2 * count[top] <= len(votes):
            undecided.append(part)
            continue
        consensus[part] = f"0x{top:08x}"
        for cu, v in votes.items():
            if v != top:
                for i in by_cu[cu]:
                    fail[i] |= 1 << list(records[i]["digests"]).index(part)
    return {"fail": fail, "consensus": consensus, "undecided": undecided}


def summarize_consensus_sweep(records: list[dict], compute_units: int, names: list[str],
                              parts: list[str] | None = None) -> dict:
    """The verdict of a consensus sweep: vote_consensus over the selected
    `parts` (None: all of `names`, the parts in bit order) writes every
    record's `fail` bits, the device having left them 0; then summarize_sweep
    and the part names, as for the other sweeps over named parts: `failed_parts`
    per XCD and overall, `bad_xcds`, `covered`, `uncovered`. Adds `consensus`
    ({part: "0x..."}, to compare GPUs and nodes by) and `undecided`."""
    vote = vote_consensus(records, list(names) if parts is None else parts)
    for r, bits in zip(records, vote["fail"]):
        r["fail"] = bits
    s = _name_fail_bits(summarize_sweep(records, compute_units), CONSENSUS_SWEEP.summary_key, names)
    s.update(consensus=vote["consensus"], undecided=vote["undecided"])
    return s


def summarize_valu_sweep(records: list[dict], compute_units: int, units: list[str]) -> dict:
    """summarize_sweep over k_valu_sweep records, whose fail bits are unit
    bits (`units` names them in bit order): adds `failed_units` per XCD and
    overall, and `failed_steps` (the names in the records' `bad_steps`, in
    first-seen order) per XCD and overall."""
    s = _name_fail_bits(summarize_sweep(records, compute_units), VALU_SWEEP.summary_key, units)
    steps: dict[int, list[str]] = {}
    for r in records:
        if int(r.get("fail", 0)):
            steps.setdefault(int(r["xcd"]), []).extend(r.get("bad_steps", []))
    for x, v in s["xcds"].items():
        v["failed_steps"] = list(dict.fromkeys(steps.get(x, [])))
    s["failed_steps"] = list(dict.fromkeys(n for x in sorted(steps) for n in steps[x]))
    return s


_probe: HipProbe | None = None


def probe() -> HipProbe:
    global _probe
    if _probe is None:
        _probe = HipProbe()
    return _probe
