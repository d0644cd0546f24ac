"""GPU-side checks on a real MI355X (run by `pytest -m gpu` on the GPU box).

The HIP probe is native code that must load and run (no fallback): device
properties, XCD census (partition-mode verification), checksum health, and
HBM streaming bandwidth against the device's ~8 TB/s HBM3E."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pr():
    from flex_gpu_scheduler_amd import build_ext

    build_ext.build_hip(verbose=False)
    from flex_gpu_scheduler_amd.ops.hip_probe import HipProbe

    p = HipProbe()
    assert p.device_count() >= 1
    return p


def test_device_props_mi355x(pr):
    props = pr.props(0)
    assert props["gcnArchName"].startswith("gfx950"), props
    assert props["warpSize"] == 64
    assert props["computeUnits"] >= 32  # 256 in SPX, 32 per XCD in CPX
    assert props["totalGlobalMem"] > (16 << 30)


def test_health_checksum(pr):
    h = pr.health(0, 256 << 20)
    assert h["healthy"], h


def test_xcd_census_matches_partition_mode(pr):
    c = pr.xcd_census(0, 4096)
    props = pr.props(0)
    assert 1 <= c["distinct_xcds"] <= 8
    # SPX exposes all 8 XCDs (256 CUs) to one device; CPX one XCD (32 CUs).
    expected = max(1, props["computeUnits"] // 32)
    assert c["distinct_xcds"] == expected, (c, props["computeUnits"])
    assert sum(c["blocks_per_xcd"]) == 4096


@pytest.mark.parametrize("mode", ["read", "copy", "triad"])
def test_hbm_bandwidth(pr, mode):
    bw = pr.hbm_bandwidth(0, 1 << 30, iters=10, mode=mode)
    # HBM3E: 8 TB/s peak; a streaming kernel that reaches < 3 TB/s over a
    # 1 GiB working set (4x the Infinity Cache) on a full device is broken.
    assert bw.gbps > 3000, bw
    # The median launch is never faster than the fastest one, and the
    # back-to-back batch rate (launch gaps included) is not above it.
    assert bw.best_gbps >= bw.gbps >= bw.batch_gbps * 0.98, bw


def test_xcd_pinned_probe_partition_bandwidth(pr):
    # Work executed only by workgroups on XCD 0 (a CPX partition's CUs) pulls
    # less HBM bandwidth than all 8 XCDs; the kernel drains either way.
    if pr.xcd_census(0, 2048)["distinct_xcds"] < 8:
        pytest.skip("device is already partitioned")
    one = pr.hbm_bandwidth_xcd(0, 0x01, 1 << 30, iters=5, mode="read")
    all8 = pr.hbm_bandwidth_xcd(0, 0xFF, 1 << 30, iters=5, mode="read")
    assert 50 < one.gbps < all8.gbps, (one, all8)


def test_partition_bandwidth_table(pr):
    """The node agent's table: CPX/QPX/DPX/SPX XCD sets, read and copy; more
    XCDs pull more bandwidth (up to the HBM limit)."""
    if pr.xcd_census(0, 2048)["distinct_xcds"] < 8:
        pytest.skip("device is already partitioned")
    t = pr.partition_table(0, 1 << 30, iters=5)
    rows = t["partitions"]
    assert list(rows) == ["CPX", "QPX", "DPX", "SPX"]
    reads = [rows[m]["read_GBps"] for m in rows]
    assert all(r > 100 for r in reads), t
    assert reads[0] < reads[1] < reads[3], t
    assert all(rows[m]["copy_GBps"] > 100 for m in rows), t


def test_tuned_variants_run(pr):
    r = pr.tune(0, "write", 256 << 20, 3)
    assert len(r["all"]) == 24 and r["best"]["GBps"] > 1000
    assert any(row["blocks_per_cu"] == 0 for row in r["all"])  # the one-shot grid


def test_segment_access_counts(pr):
    # The counter-calibration kernel: known bytes and 128-B lines per dispatch.
    for mode, seg in (("read", 64), ("write", 1024)):
        r = pr.segment_access(0, mode, seg, 4096, 1 << 12, 2)
        assert r["bytes_per_dispatch"] == (1 << 12) * seg
        assert r["lines128_per_dispatch"] == (1 << 12) * ((seg + 127) // 128)
        assert r["ms"] > 0


def test_smoke_entry():
    r = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.smoke()"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["smoke"] == "ok"


@pytest.mark.timeout(400)
def test_bench_one_gpu_json_contract():
    # The open-loop search, scenarios and service mode are exercised by the
    # bench runs themselves (and CPU tests); here the line and the placement.
    r = subprocess.run([sys.executable, "bench.py", "--full", "--steps", "3", "--warmup", "1", "--nodes", "16",
                        "--no-open-loop", "--no-scenarios", "--no-service-mode"], cwd=ROOT, capture_output=True,
                       text=True, timeout=380)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in line
    assert line["value"] > 0 and line["config"]["gpu"]["name"].startswith("gfx950")
    assert line["n_gpus"] == 1
    pl = line["config"]["rccl_placement"]
    assert pl["source"] == "live sysfs/KFD", pl
    assert pl["gangs"][0]["gang"] == 1 and pl["gangs"][0]["ordinals"] == [0], pl


def test_placement_resolves_to_the_visible_gpu():
    """Live discovery -> scheduler -> device-plugin Allocate -> HIP ordinal:
    the 1-rank gang lands on the GPU this process holds (every other GPU of
    the box is occupied by tenant pods), and the render node Allocate returns
    is that GPU's, matched by PCI address."""
    import torch

    from flex_gpu_scheduler_amd.gpu.discovery import discover_host
    from flex_gpu_scheduler_amd.parallel.dist import DistContext
    from flex_gpu_scheduler_amd.parallel.placement import validate_placement

    host = discover_host()
    assert host.gpus, "no amdgpu devices in sysfs"
    r = validate_placement(DistContext(rank=0, local_rank=0, world_size=1, backend="none", cuda=True))
    assert "error" not in r, r
    g = r["gangs"][0]
    assert g["gang"] == 1 and g["ordinals"] == [0]
    p = torch.cuda.get_device_properties(0)
    bdf = f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}.0"
    assert host.gpus[g["gpus"][0]].bdf == bdf, (g, bdf)
    assert g["xsched_gpu_index"] == [str(g["gpus"][0])]


@pytest.mark.gpu
def test_mfma_tile_exact():
    """v_mfma_f32_32x32x16_bf16 on exact integers matches the integer GEMM
    bit for bit (A/B fragment and C/D lane maps of gfx950)."""
    from flex_gpu_scheduler_amd.ops.hip_probe import probe
    for k in (16, 64, 256):
        r = probe().mfma_check(0, k)
        assert r["mismatches"] == 0, r


@pytest.mark.gpu
def test_mfma_peak_scales_with_xcds():
    from flex_gpu_scheduler_amd.ops.hip_probe import probe
    p = probe()
    full = p.mfma_peak(0, 0xFF, iters=8192)
    one = p.mfma_peak(0, 0x01, iters=8192)
    assert full["active_blocks"] == 8 * p.props(0)["computeUnits"]
    # Dense bf16 after a clock-ramping warm-up: near the 2.5 PF issue rate
    # (2.40-2.49 PF measured, profiles/r4z_mfma_sweep.jsonl), never above it.
    assert 1800.0 < full["tflops"] < 2600.0, full
    # One XCD is an eighth of the chip (CPX partition budget).
    ratio = one["tflops"] / full["tflops"]
    assert 0.08 < ratio < 0.2, (one, full)


def test_amdsmi_telemetry_sees_hbm_load():
    """The native amd-smi sampler (csrc/telemetry/amdsmi_sampler.cc) reads the
    live MI355X: 8 XCCs, 7 xGMI links up, idle near 0%, and a device copy
    loop drives GFX and HBM-controller activity and power up."""
    # Own process: this module's HIP probe runtime and torch's must not share one.
    out = subprocess.run([sys.executable, "-m", "flex_gpu_scheduler_amd.tools.amdsmi_probe", "--seconds", "1.5"],
                         cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["available"], r
    assert r["gpu0"]["xcc"] == 8 and r["gpu0"]["links_up"] >= 1, r
    assert r["load"]["max_gfx"] >= 50 and r["load"]["max_umc"] >= 20, r
    assert r["load"]["max_umc"] > r["idle"]["max_umc"] and r["load"]["max_power_w"] > r["idle"]["max_power_w"], r


def test_trimaran_tlp_on_live_gpu_load():
    """TargetLoadPacking scores nodes from live amd-smi telemetry: a GPU kept
    >50% busy by a device copy loop scores differently from the same GPU
    sampled idle, and the first GPU pod lands where explain() predicts
    (tools/tlp_live.py; TLP target 40%, so the busy node scores 0)."""
    out = subprocess.run([sys.executable, "-m", "flex_gpu_scheduler_amd.tools.tlp_live", "--seconds", "2"],
                         cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    from flex_gpu_scheduler_amd.tools.tlp_live import BUSY, IDLE

    assert r["gpu_source"] == "amdsmi", r
    assert r["gpu_busy_avg"][BUSY] > 50 and r["gpu_busy_avg"][IDLE] < 20, r
    assert r["tlp_scores"][IDLE] != r["tlp_scores"][BUSY], r
    assert r["tlp_scores"][IDLE] > r["tlp_scores"][BUSY], r
    assert r["predicted"] == r["landed"] == IDLE, r


def test_node_agent_sampler_uses_amdsmi_on_the_box():
    from flex_gpu_scheduler_amd.gpu.telemetry import HostSampler, NodeTelemetry

    hs = HostSampler()
    assert hs.gpu_source == "amdsmi"
    nt = NodeTelemetry("box", hs)
    nt.sample()
    s = nt.sample()
    assert s.gpu is not None and s.hbm_bandwidth is not None
    assert {"GPU", "GPUMemory", "GPUMemoryBandwidth"} <= {m["type"] for m in nt.metrics()}
