"""k_fetch_sweep's code object, compiled for gfx950 without a GPU. The sweep's
test data is its code, so this ties the bytes a CU will fetch to the reference:
every instruction of every region, in address order, is the one
tests/fetch_sweep_ref.py expects, with its literal; the regions have the sizes
and alignments the header of csrc/hip/fetch_sweep.hip claims; every backward
branch of the sweep's asm counts down from an immediate; nothing spills and
there is no scratch."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

import fetch_sweep_ref as ref
from flex_gpu_scheduler_amd.build_ext import CSRC, ROCM

SRC = CSRC / "hip" / "fetch_sweep.hip"
LLVM = ROCM / "llvm" / "bin"


def tool(name: str) -> str | None:
    return shutil.which(name) or (str(LLVM / name) if (LLVM / name).exists() else None)


HIPCC = shutil.which("hipcc") or (str(ROCM / "bin" / "hipcc") if (ROCM / "bin" / "hipcc").exists() else None)
pytestmark = pytest.mark.skipif(HIPCC is None or tool("llvm-readelf") is None or tool("llvm-objdump") is None,
                                reason="hipcc and the LLVM binary tools are needed")

ROT = ("v_alignbit_b32", "rot")  # v_alignbit_b32 v, v, v, 27
NOP, RET = ("s_nop", 0), ("s_setpc_b64", "s[22:23]")


@pytest.fixture(scope="module")
def built(tmp_path_factory) -> Path:
    d = tmp_path_factory.mktemp("fetch")
    out = d / "fetch_sweep.o"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "--no-gpu-bundle-output",
           f"-I{CSRC}", "-c", str(SRC), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


class Code:
    """k_fetch_sweep: its instructions by address and the labels of its asm, both relative to the kernel's symbol."""

    def __init__(self, obj: Path):
        syms = subprocess.run([tool("llvm-readelf"), "-sW", str(obj)], capture_output=True, text=True, check=True).stdout
        rows = [l.split() for l in syms.splitlines() if re.match(r"\s*\d+:", l)]
        kernel = {(int(r[1], 16), int(r[2])) for r in rows if r[3] == "FUNC" and "k_fetch_sweep" in r[7]}
        assert len(kernel) == 1  # .dynsym and .symtab agree
        (self.address, self.size), = kernel
        self.labels = {}
        for r in rows:
            m = re.match(r"(xs_fetch_\w+?)_\d+$", r[7]) if len(r) > 7 else None
            at = int(r[1], 16) - self.address
            if m and 0 <= at <= self.size:
                assert self.labels.get(m.group(1), at) == at, f"{m.group(1)} stands twice: a statement was duplicated"
                self.labels[m.group(1)] = at
        sections = subprocess.run([tool("llvm-readelf"), "-SW", str(obj)], capture_output=True, text=True,
                                  check=True).stdout
        text = [l.split() for l in sections.splitlines() if re.search(r"\s\.text\s", l)]
        assert len(text) == 1
        self.text_align = int(text[0][-1])
        dis = subprocess.run([tool("llvm-objdump"), "-d", str(obj)], capture_output=True, text=True, check=True).stdout
        self.insns = {}  # offset -> (mnemonic, operand text, bytes)
        self.first_dword = {}
        for line in dis.splitlines():
            m = re.match(r"\s+(\S+)\s*(.*?)\s*// ([0-9A-F]+): ((?:[0-9A-F]{8} ?)+)", line)
            if not m:
                continue
            at = int(m.group(3), 16) - self.address
            if 0 <= at < self.size:
                self.insns[at] = (m.group(1), m.group(2), 4 * len(m.group(4).split()))
                self.first_dword[at] = int(m.group(4).split()[0], 16)
        self.order = sorted(self.insns)

    def between(self, lo: int, hi: int) -> list:
        return [(at, *self.insns[at]) for at in self.order if lo <= at < hi]

    def tokens(self, lo: int, hi: int) -> list:
        """The instructions of [lo, hi) as the reference names them."""
        out = []
        for at, op, args, size in self.between(lo, hi):
            a = [x.strip() for x in args.split(",")]
            if op == "v_alignbit_b32" and len(a) == 4 and a[0] == a[1] == a[2] and a[3] == "27":
                out.append(ROT)
            elif op == "v_xor_b32_e32" and a[0] == a[2] and a[1].startswith("0x"):
                out.append(("V", int(a[1], 16)))
            elif op == "s_xor_b32" and a[:2] == ["s25", "s26"]:
                out.append(("S", int(a[2], 16)))
            elif op == "s_addk_i32" and a[0] == "s25":
                out.append(("K", int(a[1], 16) & 0xFFFF))
            elif op == "v_xor_b32_e32" and a[0] == a[2] and a[1] == "s25":
                out.append(("fold", "s25"))
            elif op == "v_xad_u32" and a[0] == a[1] and a[2] == "s26":
                out.append(("X", "s26"))
            elif op == "s_nop":
                out.append(("s_nop", int(a[0])))
            else:
                out.append((op, args))
        return out

    def branch_target(self, at: int) -> int:
        simm = self.first_dword[at] & 0xFFFF  # SOPP and s_call_b64 (SOPK): a count of dwords from the next one
        return at + 4 + 4 * (simm - 0x10000 if simm & 0x8000 else simm)


def expected_steps(region: int, steps: list, nops: int, ret: bool) -> list:
    out = []
    for j, i in enumerate(steps):
        lit = ref.literal(region, i)
        out.append(ROT)
        k = ref.kind(j)
        if k == "V":
            out.append(("V", lit))
        elif k == "S":
            out += [("S", lit), ("fold", "s25")]
        elif k == "K":
            out += [("K", lit & 0xFFFF), ("fold", "s25")]
        else:
            out.append(("X", "s26"))
    return out + [NOP] * nops + ([RET] if ret else [])


@pytest.fixture(scope="module")
def code(built) -> Code:
    return Code(built)


def test_kernels_spill_nothing_and_use_no_scratch(built, code):
    notes = subprocess.run([tool("llvm-readelf"), "--notes", str(built)], capture_output=True, text=True, check=True).stdout
    for kernel in ("k_fetch_sweep", "k_fetch_probe"):
        ks = [k for k in re.split(r"\n\s+- \.agpr_count:", "\n" + notes) if kernel in k]
        assert len(ks) == 1, kernel
        k = ".agpr_count:" + ks[0]

        def field(name: str) -> int:
            m = re.search(rf"\.{name}:\s+(\d+)", k)
            assert m, name
            return int(m.group(1))

        assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
        assert field("private_segment_fixed_size") == 0
        assert field("max_flat_workgroup_size") == 256
        assert field("group_segment_fixed_size") == 0  # the LDS is dynamic: the launch sizes it to own the CU
        assert field("vgpr_count") <= 128
    assert not any(op.startswith("scratch_") for op, _, _ in code.insns.values())


def test_the_kernel_is_page_aligned_and_holds_every_statement_once(code):
    assert code.address % 4096 == 0 and code.text_align >= 4096
    want = {"xs_fetch_stream_pc", "xs_fetch_stream", "xs_fetch_stream_out", "xs_fetch_stream_end",
            "xs_fetch_call_pc", "xs_fetch_extra", "xs_fetch_call", "xs_fetch_call_end",
            "xs_fetch_align_pc", "xs_fetch_tramp", "xs_fetch_align_end", "xs_fetch_inv",
            *(f"xs_fetch_t{k}" for k in range(17)),
            *(f"xs_fetch_loop{b}{e}" for b in range(4) for e in ("", "_end"))}
    assert set(code.labels) == want  # Code() refuses a label that stands twice


def test_stream_is_32_segments_of_8_kib_with_the_references_literals(code):
    base, end = code.labels["xs_fetch_stream"], code.labels["xs_fetch_stream_end"]
    assert base % 4096 == 0 and end - base == 32 * 8192 == 256 << 10
    runs = ref.run_steps(ref.STREAM)
    lits = []
    for s in range(32):
        got = code.tokens(base + 8192 * s, base + 8192 * (s + 1))
        assert got == expected_steps(ref.STREAM, runs[s], ref.SEGMENT_NOPS, True), s
        assert code.insns[base + 8192 * s + 8188][0] == "s_setpc_b64"  # the segment's last dword
        lits += [v for k, v in got if k in "VSK"]
    assert lits == ref.region_literals(ref.STREAM) and len(lits) == 32 * 361


def test_the_computed_jumps_are_bounded(code):
    for pc, base, n, shift in (("xs_fetch_stream_pc", "xs_fetch_stream", 32, 13),
                               ("xs_fetch_call_pc", "xs_fetch_call", 256, 6),
                               ("xs_fetch_align_pc", "xs_fetch_tramp", 32, 6)):
        at = code.labels[pc]
        assert code.labels[base] % (1 << shift) == 0 or shift == 13  # `stream`: 4 KiB, what a loaded page keeps
        assert code.insns[at - 4][:2] == ("s_getpc_b64", "s[20:21]")
        def numbered(op, args):  # the last operand as a number, however the disassembler writes it
            a = [x.strip() for x in args.split(",")]
            return (op, *a[:-1], int(a[-1], 0) if re.fullmatch(r"-?(0x)?[0-9a-f]+", a[-1]) else a[-1])

        got = [numbered(*code.insns[a][:2]) for a in code.order if at <= a][:7]
        index = got[0][2]
        assert re.fullmatch(r"s\d+", index) and index not in ("s20", "s21", "s22", "s23", "s24", "s25", "s26")
        assert got == [("s_and_b32", "s24", index, n - 1), ("s_lshl_b32", "s24", "s24", shift),
                       ("s_add_u32", "s20", "s20", "s24"), ("s_addc_u32", "s21", "s21", 0),
                       ("s_add_u32", "s20", "s20", code.labels[base] - at),  # the label difference, folded
                       ("s_addc_u32", "s21", "s21", 0), ("s_swappc_b64", "s[22:23]", "s[20:21]")], pc


def test_the_loop_bodies_and_their_countdowns(code):
    for b in range(4):
        lo, hi = code.labels[f"xs_fetch_loop{b}"], code.labels[f"xs_fetch_loop{b}_end"]
        assert lo % 64 == 0 and hi - lo == ref.LOOP_BYTES[b]
        steps = ref.run_steps(ref.LOOP0 + b)[0]
        got = code.tokens(lo, hi)
        assert got == expected_steps(ref.LOOP0 + b, steps, ref.LOOP_NOPS[b], False), b
        assert [v for k, v in got if k in "VSK"] == ref.region_literals(ref.LOOP0 + b)
        # The countdown: an SGPR the statement set from an immediate, and the one backward branch.
        tail = code.between(hi, hi + 12)
        assert [(op, args.split("//")[0].strip()) for _, op, args, _ in tail[:2]] == [
            ("s_sub_u32", "s24, s24, 1"), ("s_cmp_lg_u32", "s24, 0")]
        assert tail[2][1] == "s_cbranch_scc1" and code.branch_target(tail[2][0]) == lo
        head = [(op, args) for _, op, args, _ in code.between(lo - 64, lo) if op == "s_movk_i32"]
        trips = [int(args.split(",")[1], 16) for op, args in head if args.startswith("s24,")]
        assert trips == ([ref.LOOP_TRIPS[b]] if b < 3 else [ref.LOOP_TRIPS[3], 1]), (b, head)


def test_every_backward_branch_of_the_asm_is_one_of_the_four_countdowns(code):
    spans = [(code.labels["xs_fetch_stream_pc"], code.labels["xs_fetch_stream_end"]),
             (code.labels["xs_fetch_call_pc"], code.labels["xs_fetch_call_end"]),
             (code.labels["xs_fetch_align_pc"], code.labels["xs_fetch_align_end"]),
             *((code.labels[f"xs_fetch_loop{b}"] - 16, code.labels[f"xs_fetch_loop{b}_end"] + 12) for b in range(4))]
    backward = []
    for lo, hi in spans:
        for at, op, args, _ in code.between(lo, hi):
            if (op.startswith("s_cbranch") or op in ("s_branch", "s_call_b64")) and code.branch_target(at) <= at:
                backward.append((op, code.branch_target(at)))
    assert sorted(backward) == sorted(("s_cbranch_scc1", code.labels[f"xs_fetch_loop{b}"]) for b in range(4))


def test_the_call_blocks(code):
    base, end, extra = code.labels["xs_fetch_call"], code.labels["xs_fetch_call_end"], code.labels["xs_fetch_extra"]
    assert base % 64 == 0 and extra % 64 == 0 and end - base == 256 * 64 and base - extra == 64
    runs = ref.run_steps(ref.CALL)  # the extra block first
    lits = []
    for n, at in enumerate([extra, *(base + 64 * b for b in range(256))]):
        got = code.tokens(at, at + 64)
        assert got == expected_steps(ref.CALL, runs[n], ref.BLOCK_NOPS, True), n
        lits += [v for k, v in got if k in "VSK"]
    assert lits == ref.region_literals(ref.CALL)
    # Behind the computed call: the direct call of the extra block and the branch over it.
    pc = code.labels["xs_fetch_call_pc"]
    after = 4 + next(at for at, op, _, _ in code.between(pc, pc + 64) if op == "s_swappc_b64")
    (a0, op0, args0, _), (a1, op1, _, _) = code.between(after, after + 8)
    assert op0 == "s_call_b64" and args0.startswith("s[22:23],") and code.branch_target(a0) == extra
    assert op1 == "s_branch" and code.branch_target(a1) == end


def test_the_align_targets_begin_at_every_dword_of_a_line_and_one_crosses_a_page(code):
    tramp = code.labels["xs_fetch_tramp"]
    assert tramp % 64 == 0
    for j in range(32):
        at = tramp + 64 * j
        assert code.insns[at][0] == "s_branch"
        assert code.branch_target(at) == code.labels[f"xs_fetch_t{ref.target_of(j)}"], j
        assert all(t == NOP for t in code.tokens(at + 4, at + 64))
    lits = []
    for k in range(17):
        at = code.labels[f"xs_fetch_t{k}"]
        assert at % 64 == 4 * k if k < 16 else at % 4096 == 4092, k
        op, _, size = code.insns[at]
        assert op == "v_xor_b32_e32" and size == 8  # opcode dword and literal
        got = code.tokens(at, at + 20)
        assert got == [("V", ref.literal(ref.ALIGN, k)), ROT, RET], k
        lits.append(got[0][1])
        if k:  # s_nop fill from the line's start (the page's, for target 16)
            fill = code.tokens(at - (at % 64 if k < 16 else 4092), at)
            assert fill and all(t == NOP for t in fill)
    assert lits == ref.region_literals(ref.ALIGN)
    t15, t16 = code.labels["xs_fetch_t15"], code.labels["xs_fetch_t16"]
    assert t15 // 64 != (t15 + 4) // 64 and t16 // 4096 != (t16 + 4) // 4096  # opcode and literal in two lines / pages


def test_the_refill_statement(code):
    at = code.labels["xs_fetch_inv"]
    got = [(op, args.split("//")[0].strip()) for _, op, args, _ in code.between(at - 19 * 4, at)]
    assert got[0] == ("s_icache_inv", "") and got[1:17] == [("s_nop", "0")] * 16
    assert got[17][0] == "s_branch" and code.branch_target(at - 8) == at


def test_the_mnemonics_are_in_the_code(code):
    ops = {op for op, _, _ in code.insns.values()}
    assert {"s_getpc_b64", "s_swappc_b64", "s_setpc_b64", "s_call_b64", "s_icache_inv", "s_cbranch_scc1", "s_branch",
            "s_movk_i32", "s_xor_b32", "s_addk_i32", "v_xad_u32", "v_alignbit_b32", "v_readfirstlane_b32"} <= ops
    assert "s_setreg_b32" not in ops and "s_setreg_imm32_b32" not in ops  # the MODE register is never written
