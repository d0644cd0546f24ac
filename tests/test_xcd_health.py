"""XCD-granular GPU health: the CU sweep's host-side verdict
(summarize_sweep), the node agent and device plugin fencing the compute
partitions that hold a bad XCD (`xcdFaults`), and the scheduler's GPU ledger
declining to place work on a fenced partition."""
import json
import time

from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.device_plugin import GpuDevicePlugin
from flex_gpu_scheduler_amd.control.deviceplugin_api import HEALTHY, UNHEALTHY
from flex_gpu_scheduler_amd.control.node_agent import UNHEALTHY_TAINT, GpuHealth, NodeAgent
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import GPU, GPU_MEMORY, GPU_XCD, TOPOLOGY_ANNOTATION, make_pod, mi355x_node
from flex_gpu_scheduler_amd.ops.hip_probe import summarize_sweep
from helpers import FLEXGPU_PLUGINS, annotations, coscheduling_config, create_all, placements, start, wait_bound


# ----------------------------------------------------------- summarize_sweep
def cu_key(c: int) -> int:
    """SE in bits 7:5, CU id in bits 3:0: 4 SEs x 8 CUs, as HW_ID lays them out."""
    return (c // 8) << 5 | c % 8


def records(xcds=8, cus=32, skip=()):
    return [{"xcd": x, "cu": cu_key(c), "simd_mask": 15, "fail": 0, "mfma": 1, "valu": 2, "lds": 3}
            for x in range(xcds) for c in range(cus) if (x, c) not in skip]


def test_summarize_clean_sweep_is_covered():
    s = summarize_sweep(records(), 256)
    assert s["covered"] and s["bad_xcds"] == []
    assert sorted(s["xcds"]) == list(range(8))
    assert all(v == {"cus_seen": 32, "cus_expected": 32, "failed_cus": [], "fail_bits": 0} for v in s["xcds"].values())
    assert not any(s["uncovered"].values())


def test_summarize_names_the_failed_cu_and_its_xcd():
    recs = records()
    bad = next(r for r in recs if r["xcd"] == 5 and r["cu"] == cu_key(17))
    bad["fail"] = 1
    s = summarize_sweep(recs, 256)
    assert s["bad_xcds"] == [5]
    assert s["xcds"][5]["failed_cus"] == [cu_key(17)] and s["xcds"][5]["fail_bits"] == 1
    assert all(v["failed_cus"] == [] for x, v in s["xcds"].items() if x != 5)
    assert s["covered"]


def test_summarize_counts_a_cu_once():
    recs = records() + [dict(r) for _ in range(3) for r in records() if r["cu"] == cu_key(3)]
    s = summarize_sweep(recs, 256)
    assert all(v["cus_seen"] == 32 for v in s["xcds"].values()) and s["covered"]
    # the fail bits of one CU's records are OR-ed into one entry
    same_cu = [r for r in recs if (r["xcd"], r["cu"]) == (2, cu_key(3))]
    assert len(same_cu) == 4
    same_cu[1]["fail"], same_cu[3]["fail"] = 2, 4
    s = summarize_sweep(recs, 256)
    assert s["xcds"][2]["failed_cus"] == [cu_key(3)] and s["xcds"][2]["fail_bits"] == 6
    assert s["bad_xcds"] == [2]


def test_summarize_uncovered_is_not_failed():
    s = summarize_sweep(records(skip={(6, 0), (6, 9), (6, 31)}), 256)
    assert s["covered"] is False
    assert s["uncovered"][6] == 3 and sum(s["uncovered"].values()) == 3
    assert s["bad_xcds"] == [] and s["xcds"][6]["cus_seen"] == 29
    assert summarize_sweep([], 256)["covered"] is False


# ------------------------------------------------- node agent + device plugin
def agent_on(store, host, health_fn):
    client = LocalClient(store)
    agent = NodeAgent(client, "n", host_fn=lambda: host, publish_metrics=False, health_fn=health_fn)
    agent.device_plugins = [GpuDevicePlugin(r, host, client, "n") for r in (GPU_XCD, GPU_MEMORY)]
    agent.sync()
    node = store.get("nodes", "", "n")
    return agent, node, json.loads(node["metadata"]["annotations"][TOPOLOGY_ANNOTATION])


def xcd5_bad_on_gpu0(dev):
    return GpuHealth(False, {5}) if dev == 0 else True


def test_agent_fences_one_cpx_partition(store):
    agent, node, topo = agent_on(store, fake_host(2, "CPX"), xcd5_bad_on_gpu0)
    assert topo["xcdFaults"] == {"0": [5]}
    assert node["status"]["allocatable"][GPU_XCD] == "15" and node["status"]["capacity"][GPU_XCD] == "16"
    assert node["status"]["allocatable"][GPU_MEMORY] == str(2 * 288 - 36)
    assert node["status"]["capacity"][GPU_MEMORY] == str(2 * 288)
    assert agent.unhealthy == set() and topo["unhealthy"] == []
    assert agent.unhealthy_xcds == {0: {5}}
    assert UNHEALTHY_TAINT not in (node.get("spec") or {}).get("taints", [])
    xcd_plugin, mem_plugin = agent.device_plugins
    health = {d.ID: d.health for d in xcd_plugin.devices()}
    assert len(health) == 16
    assert [i for i, h in health.items() if h == UNHEALTHY] == ["xcd-0-5"]
    assert sum(h == HEALTHY for h in health.values()) == 15
    mem = [d for d in mem_plugin.devices() if d.health == UNHEALTHY]
    assert len(mem) == 36 and all(d.ID.startswith("mem-0-") for d in mem)
    # the owning NUMA zone loses the same share; capacity reports the hardware
    nrt = store.get("noderesourcetopologies", "", "n")
    z0 = {r["name"]: r for r in nrt["zones"][0]["resources"]}
    z1 = {r["name"]: r for r in nrt["zones"][1]["resources"]}
    assert (z0[GPU_XCD]["allocatable"], z0[GPU_XCD]["available"], z0[GPU_XCD]["capacity"]) == ("7", "7", "8")
    assert z0[GPU_MEMORY]["allocatable"] == str(288 - 36) and z1[GPU_XCD]["allocatable"] == "8"


def test_agent_fences_the_qpx_partition_that_owns_the_xcd(store):
    agent, node, topo = agent_on(store, fake_host(2, "QPX"), xcd5_bad_on_gpu0)
    assert topo["xcdFaults"] == {"0": [5]}
    assert node["status"]["allocatable"][GPU_XCD] == "14" and node["status"]["capacity"][GPU_XCD] == "16"
    assert agent.unhealthy == set()
    bad = [d.ID for d in agent.device_plugins[0].devices() if d.health == UNHEALTHY]
    assert bad == ["xcd-0-4", "xcd-0-5"]


def test_agent_withholds_an_spx_gpu_with_a_bad_xcd(store):
    agent, node, topo = agent_on(store, fake_host(2), xcd5_bad_on_gpu0)
    assert agent.unhealthy == {0} and topo["unhealthy"] == [0]
    assert topo["xcdFaults"] == {"0": [5]}
    _, as_false, topo_false = agent_on(store, fake_host(2), lambda dev: dev != 0)
    assert node["status"]["allocatable"] == as_false["status"]["allocatable"]
    assert "xcdFaults" not in topo_false


def test_bool_callback_publishes_no_xcd_faults(store):
    agent, node, topo = agent_on(store, fake_host(2, "CPX"), lambda dev: True)
    assert "xcdFaults" not in topo and agent.unhealthy_xcds == {}
    plain = NodeAgent(LocalClient(store), "n", host_fn=lambda: fake_host(2, "CPX"), publish_metrics=False)
    want = plain.build_node(fake_host(2, "CPX"))["metadata"]["annotations"][TOPOLOGY_ANNOTATION]
    assert node["metadata"]["annotations"][TOPOLOGY_ANNOTATION] == want  # byte-identical to today's
    assert all(d.health == HEALTHY for d in agent.device_plugins[0].devices())


def test_xcd_fault_change_triggers_a_resync(store):
    verdict = {"v": True}
    agent, _, topo = agent_on(store, fake_host(2, "CPX"), lambda dev: verdict["v"])
    assert "xcdFaults" not in topo
    verdict["v"] = GpuHealth(False, {1})
    agent._heartbeat_and_resync()
    topo = json.loads(store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION])
    assert topo["xcdFaults"] == {"0": [1], "1": [1]}


# ------------------------------------------------------------------- ledger
def faulty_node(mode: str, faults: dict | None, xcds: int, mem: int = 288):
    node = mi355x_node("n", n_gpus=1, mode=mode)
    if faults is not None:
        topo = json.loads(node["metadata"]["annotations"][TOPOLOGY_ANNOTATION])
        topo["xcdFaults"] = faults
        node["metadata"]["annotations"][TOPOLOGY_ANNOTATION] = json.dumps(topo)
        node["status"]["allocatable"][GPU_XCD] = str(xcds)  # as the agent lowers them
        node["status"]["allocatable"][GPU_MEMORY] = str(mem)
    return node


def cfg():
    return coscheduling_config(FLEXGPU_PLUGINS)


def test_ledger_never_places_on_a_fenced_cpx_partition(store):
    store.create("nodes", faulty_node("cpx", {"0": [5]}, 7, 252))
    s = start(store, cfg())
    try:
        g = s.node_info("n")["gpu"]
        assert g["fenced"] == [[p == 5 for p in range(8)]] and g["free_xcds"] == 7
        assert g["free_memory"] == 252 and g["mem_per_gpu"] == 288
        create_all(store, "pods", [make_pod(f"x{i}", limits={GPU_XCD: "1"}) for i in range(7)])
        wait_bound(s, 7)
        parts = sorted(annotations(store, f"x{i}")["amd.com/gpu-partitions"] for i in range(7))
        assert parts == [f"0:{p}" for p in range(8) if p != 5]
        store.create("pods", make_pod("x7", limits={GPU_XCD: "1"}))
        time.sleep(0.3)
        assert placements(store)["x7"] == ""
        assert s.node_info("n")["gpu"]["free_xcds"] == 0
    finally:
        s.stop()


def test_memory_slices_avoid_a_fenced_partition(store):
    store.create("nodes", faulty_node("cpx", {"0": [5]}, 7, 252))
    s = start(store, cfg())
    try:
        # 36 GiB per CPX partition: seven 30 GiB slices need seven partitions.
        create_all(store, "pods", [make_pod(f"m{i}", limits={GPU_MEMORY: "30"}) for i in range(7)])
        wait_bound(s, 7)
        parts = sorted(annotations(store, f"m{i}")["amd.com/gpu-partitions"] for i in range(7))
        assert parts == [f"0:{p}" for p in range(8) if p != 5]
        store.create("pods", make_pod("m7", limits={GPU_MEMORY: "30"}))
        time.sleep(0.3)
        assert placements(store)["m7"] == ""
    finally:
        s.stop()


def test_qpx_fault_fences_two_xcds(store):
    store.create("nodes", faulty_node("qpx", {"0": [5]}, 6, 216))
    s = start(store, cfg())
    try:
        g = s.node_info("n")["gpu"]
        assert g["free_xcds"] == 6 and g["fenced"] == [[False, False, True, False]]
        assert g["free_memory"] == 216
    finally:
        s.stop()


def test_spx_gpu_with_a_fault_takes_no_whole_gpu_pod(store):
    store.create("nodes", faulty_node("spx", {"0": [5]}, 8))
    s = start(store, cfg())
    try:
        g = s.node_info("n")["gpu"]
        assert g["free_gpus"] == 0 and g["free_xcds"] == 0
        store.create("pods", make_pod("whole", limits={GPU: "1"}))
        time.sleep(0.3)
        assert placements(store)["whole"] == ""
    finally:
        s.stop()


def test_faults_of_a_withheld_gpu_fence_nothing(store):
    # What the agent publishes for two SPX GPUs when GPU 0 has a bad XCD: GPU 0
    # is withheld (one GPU allocatable) and its entry must not fence the other.
    agent = NodeAgent(LocalClient(store), "n", host_fn=lambda: fake_host(2), publish_metrics=False,
                      health_fn=xcd5_bad_on_gpu0)
    agent.sync()
    s = start(store, cfg())
    try:
        g = s.node_info("n")["gpu"]
        assert g["gpu_count"] == 1 and g["free_gpus"] == 1 and g["fenced"] == [[False]]
        store.create("pods", make_pod("whole", limits={GPU: "1"}))
        wait_bound(s, 1)
    finally:
        s.stop()


def test_node_without_faults_is_unchanged(store):
    store.create("nodes", faulty_node("cpx", None, 8))
    s = start(store, cfg())
    try:
        g = s.node_info("n")["gpu"]
        assert g["fenced"] == [[False] * 8] and g["free_xcds"] == 8 and g["free_memory"] == 288
        assert all(len(t) == 3 for t in g["slots"][0])
        create_all(store, "pods", [make_pod(f"x{i}", limits={GPU_XCD: "1"}) for i in range(8)])
        wait_bound(s, 8)
    finally:
        s.stop()


def test_malformed_fault_entries_are_ignored(store):
    store.create("nodes", faulty_node("cpx", {"0": [8, -1, "x", 2], "9": [1], "zz": 3}, 7, 252))
    s = start(store, cfg())
    try:
        assert s.node_info("n")["gpu"]["fenced"] == [[p == 2 for p in range(8)]]
    finally:
        s.stop()
