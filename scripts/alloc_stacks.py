"""Symbolize the `stack` lines of the counting stress driver
(build_ext --stress-count, run with XSCHED_ALLOC_STACKS=1): per stack, the
allocations per pod and the project's own frames, innermost first.

    python scripts/alloc_stacks.py REPORT EXE [TOP]
"""
import re
import subprocess
import sys


def main() -> None:
    report, exe = sys.argv[1], sys.argv[2]
    top = int(sys.argv[3]) if len(sys.argv) > 3 else 60
    rows = []
    for line in open(report):
        if not line.startswith("stack "):
            continue
        head, frames = line.split(" :", 1)
        per_pod = float(re.search(r"per_pod=([0-9.]+)", head).group(1))
        avg = float(re.search(r"avg_bytes=([0-9.]+)", head).group(1))
        rows.append((per_pod, avg, frames.split()))
    rows = rows[:top]
    exe_name = exe.rsplit("/", 1)[-1]
    addrs = sorted({f.rsplit("+", 1)[1] for _, _, fr in rows for f in fr if f.rsplit("+", 1)[0] in (exe_name, "xsched_stress_count")})
    # return addresses: look up the call instruction (pc - 1)
    q = [hex(int(a, 16) - 1) for a in addrs]
    out = subprocess.run(["addr2line", "-f", "-C", "-i", "-a", "-e", exe, *q], capture_output=True, text=True).stdout
    sym: dict[str, list[str]] = {}
    cur = None
    lines = out.splitlines()
    i = 0
    while i < len(lines):
        if lines[i].startswith("0x"):
            cur = hex(int(lines[i], 16) + 1)
            sym[cur] = []
            i += 1
            continue
        fn, loc = lines[i], lines[i + 1] if i + 1 < len(lines) else "?"
        i += 2
        loc = loc.split(" (")[0]
        if "/csrc/" in loc:
            loc = loc.split("/csrc/")[1]
            fn = re.sub(r"\(.*", "", fn)
            sym[cur].append(f"{fn} {loc}")
    total = 0.0
    for per_pod, avg, frames in rows:
        total += per_pod
        own = []
        for f in frames:
            mod, off = f.rsplit("+", 1)
            own.extend(sym.get(hex(int(off, 16)), []))
        print(f"{per_pod:7.3f}/pod {avg:6.0f} B  " + " <- ".join(own[:5]))
    print(f"{total:7.3f}/pod in the {len(rows)} stacks shown")


if __name__ == "__main__":
    main()
