"""MI355X node agent: advertises a GPU node to the scheduler.

Plays the roles the reference delegates to the NVIDIA device plugin + the NRT
exporter + metrics-server:
  * discovers the box from sysfs (gpu/discovery.py) — GPUs, compute/memory
    partition modes, HBM, NUMA locality, xGMI hive;
  * registers/updates the Node: allocatable `amd.com/gpu` (whole SPX GPUs),
    `amd.com/gpu-xcd` (XCD slices), `amd.com/gpu-memory` (HBM GiB), the
    compute-partition label and the `amd.com/gpu-topology` annotation FlexGPU
    reads (csrc/plugins/flexgpu.cc), plus a Ready heartbeat condition;
  * publishes the NodeResourceTopology CR (one zone per CPU socket holding its
    GPUs) for NodeResourceTopologyMatch;
  * optionally runs the HIP health probe (ops/hip_probe.py: pattern write +
    checksum per GPU) and withholds unhealthy GPUs from allocatable, tainting
    the node when none are healthy; a verdict that names bad XCDs (GpuHealth,
    e.g. from the CU sweep) fences only the compute partitions holding them
    on a DPX/QPX/CPX GPU (`xcdFaults` in the topology annotation), and the
    matrix formats such an XCD gets wrong are published as `matrixFaults`
    and the register files it reads back wrong as `registerFaults` and the
    cross-lane and LDS paths it moves data wrongly through as `laneFaults`
    and the vector-ALU units it mis-computes as `valuFaults` and the parts
    of the scalar unit it gets wrong as `scalarFaults` and the parts of
    the consensus sweep on which one of its CUs disagrees with the majority
    of the GPU's CUs as `consensusFaults` and the parts of the fetch
    sweep (its own code, fetched wrongly) as `fetchFaults` and the routes
    between registers and HBM it corrupts data on as `memFaults`;
    a verdict that carries an HBM fault (the HBM sweep) withholds the whole
    GPU, partitioned or not, and is published as `hbmFaults`;
  * samples load (gpu/telemetry.py) and publishes its WatcherMetrics document
    for the Trimaran plugins.
"""
from __future__ import annotations

import json
import logging
import threading
import time
from dataclasses import dataclass, field
from datetime import datetime, timezone
from typing import Callable

from ..gpu.discovery import HostInfo, discover_host
from ..gpu.telemetry import HostSampler, NodeTelemetry, publish
from ..models.mi355x import (GPU, GPU_MEMORY, GPU_XCD, TOPOLOGY_ANNOTATION, XCDS_PER_GPU, fenced_partitions,
                             mi355x_node, mi355x_nrt)
from .client import Client, is_conflict

log = logging.getLogger(__name__)

# Per-GPU HBM bandwidth by compute-partition size (NodeAgent.measure_bandwidth).
BANDWIDTH_ANNOTATION = "amd.com/gpu-hbm-bandwidth"
UNHEALTHY_TAINT = {"key": "amd.com/gpu-unhealthy", "value": "true", "effect": "NoSchedule"}
MEMORY_PARTITION_LABEL = "amd.com/gpu.memory-partition"
HIVE_LABEL = "amd.com/xgmi.hive"


@dataclass(frozen=True)
class FaultKind:
    """How one kind of fault in GpuHealth.detail travels to the topology
    annotation, where it stands under the same key. `per_xcd`: the value is
    {XCD id: list or dict} (int keys in the agent, strings in the annotation)
    and an XCD's empty entry is dropped; otherwise it is one dict for the GPU.
    `withholds_gpu`: a GPU that has one is withheld as a whole."""
    per_xcd: bool
    withholds_gpu: bool = False


def _register_fault(v: dict) -> dict:
    return {"files": list(v["failed_files"]), "cells": int(v["bad_cells"]), "flipMask": v["flip_mask"],
            "simds": sum(len(sm) for sm in v["bad_simds"].values())} if v["failed_files"] else {}


@dataclass(frozen=True)
class SweepKind:
    """One per-CU sweep of hip_health_fn, whose parameter `enabled_by` switches
    it on, <enabled_by>_args being the keywords of the probe's `method` and
    <enabled_by>_<selection> the parts for its keyword `selection`. `label`
    starts its log line; `summary_key` and `faults_key` are the keys of the
    verdict's detail for the summary and for {xcd: fault}; `fault_of` reads
    one XCD's fault (empty: none) from its entry of the summary. The CU sweep
    names no fault kind: its log line shows the bad XCDs."""
    enabled_by: str
    method: str
    label: str
    summary_key: str
    selection: str | None = None
    faults_key: str | None = None
    fault_of: Callable[[dict], "list | dict"] | None = None


# In the order they run; hip_health_fn's docstring has the shape of each fault.
SWEEP_KINDS = (
    SweepKind("sweep", "cu_sweep", "cu", "sweep"),
    SweepKind("matrix", "matrix_sweep", "matrix", "matrixSweep", "formats", "matrixFaults",
              lambda v: list(v["failed_formats"])),
    SweepKind("regfile", "regfile_sweep", "register", "registerSweep", None, "registerFaults", _register_fault),
    SweepKind("lane", "lane_sweep", "lane", "laneSweep", "paths", "laneFaults", lambda v: list(v["failed_paths"])),
    SweepKind("valu", "valu_sweep", "valu", "valuSweep", "units", "valuFaults", lambda v: list(v["failed_units"])),
)
# The memory-path sweep runs after them, through the same code. It stands
# apart because, like the HBM sweep, it holds HBM while it runs and can find
# none to hold: its GPU is then unswept, which is no verdict at all.
MEM_SWEEP_KIND = SweepKind("mem", "mem_sweep", "mem", "memSweep", "routes", "memFaults",
                           lambda v: list(v["failed_routes"]))
# The scalar sweep runs after the VALU sweep and before the memory sweep,
# through the same code. It stands beside SWEEP_KINDS because its fault is one
# dict for the GPU, as the memory sweep's is. It allocates nothing but its
# records, so it has no "unswept" outcome.
SCALAR_SWEEP_KIND = SweepKind("scalar", "scalar_sweep", "scalar", "scalarSweep", "parts", "scalarFaults",
                              lambda v: list(v["failed_parts"]))
# The consensus sweep runs after the scalar sweep and before the memory sweep,
# through the same code, and stands beside SWEEP_KINDS for the same reason. Its
# reference is the majority of the GPU's own CUs: a part without a majority is
# undecided, which is logged and is no verdict at all.
CONSENSUS_SWEEP_KIND = SweepKind("consensus", "consensus_sweep", "consensus", "consensusSweep", "parts",
                                 "consensusFaults", lambda v: list(v["failed_parts"]))
# The fetch sweep runs after the consensus sweep and before the memory sweep,
# through the same code, and stands beside SWEEP_KINDS for the same reason. It
# allocates nothing but its records, so it has no "unswept" outcome.
FETCH_SWEEP_KIND = SweepKind("fetch", "fetch_sweep", "fetch", "fetchSweep", "parts", "fetchFaults",
                             lambda v: list(v["failed_parts"]))

FAULT_KINDS = {
    # What the per-CU sweeps found on a faulty XCD. Informational: the XCD is
    # fenced through xcdFaults; these are for operators and RMA tooling.
    **{k.faults_key: FaultKind(per_xcd=True) for k in SWEEP_KINDS if k.faults_key},
    # What the HBM sweep found on the GPU. The sweep knows a fault by its
    # virtual address, which cannot be tied to the HBM slice of one compute
    # partition, so there is no partial fence for memory.
    "hbmFaults": FaultKind(per_xcd=False, withholds_gpu=True),
    # What the memory-path sweep found on the GPU: one dict, {XCD id: [route,
    # ...]}, of the XCDs with a fault. Informational like the first group; the
    # XCD is fenced through xcdFaults.
    MEM_SWEEP_KIND.faults_key: FaultKind(per_xcd=False),
    # What the scalar sweep found on the GPU: {XCD id: [part, ...]}, likewise.
    SCALAR_SWEEP_KIND.faults_key: FaultKind(per_xcd=False),
    # What the consensus sweep found on the GPU: {XCD id: [part, ...]}, likewise.
    CONSENSUS_SWEEP_KIND.faults_key: FaultKind(per_xcd=False),
    # What the fetch sweep found on the GPU: {XCD id: [part, ...]}, likewise.
    FETCH_SWEEP_KIND.faults_key: FaultKind(per_xcd=False),
}


def _fault_value(v):
    return dict(v) if isinstance(v, dict) else list(v)


def _now() -> str:
    return datetime.now(timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ")


@dataclass(frozen=True)
class GpuHealth:
    """A health verdict finer than one boolean: `bad_xcds` are the GPU's
    physical XCD ids (0-7) that hold a faulty CU. An SPX GPU with a bad XCD is
    withheld like an unhealthy one; on a DPX/QPX/CPX GPU only the compute
    partitions that contain a bad XCD are fenced. `ok` False with no bad XCD
    is a whole-GPU failure, and so is a verdict whose detail["hbmFaults"] is
    not empty, whatever XCDs it names."""
    ok: bool
    bad_xcds: frozenset = frozenset()
    detail: dict = field(default_factory=dict, compare=False)

    def __post_init__(self):
        object.__setattr__(self, "bad_xcds", frozenset(int(x) for x in self.bad_xcds if 0 <= int(x) < XCDS_PER_GPU))

    def __bool__(self) -> bool:
        return bool(self.ok) and not self.bad_xcds


class NodeAgent:
    def __init__(self, client: Client, node_name: str, *, host_fn: Callable[[], HostInfo] | None = None,
                 root: str = "/", labels: dict | None = None, reserved_cpu: int = 0, reserved_memory_gib: int = 0,
                 heartbeat: float = 10.0, telemetry_period: float = 60.0, publish_metrics: bool = True,
                 health_fn: Callable[[int], "bool | GpuHealth"] | None = None, sampler=None,
                 kubelet_managed: bool = False, bandwidth_fn: Callable[[int], dict] | None = None):
        self.client, self.name = client, node_name
        self.host_fn = host_fn or (lambda: discover_host(root))
        self.labels = dict(labels or {})
        self.reserved_cpu, self.reserved_memory_gib = reserved_cpu, reserved_memory_gib
        self.heartbeat, self.telemetry_period = heartbeat, telemetry_period
        self.health_fn = health_fn
        # HBM bandwidth per compute-partition size, per GPU (ops/hip_probe.py
        # partition_table): measured once per GPU and published with the node.
        self.bandwidth_fn = bandwidth_fn
        self.bandwidth: dict[int, dict] = {}
        # A GPU whose probe failed is not probed again on every heartbeat
        # (each attempt streams GiBs through a GPU that may be serving
        # tenants): GPU index -> time.monotonic() of the next attempt.
        self.bandwidth_retry_s = 600.0
        self._bandwidth_retry_at: dict[int, float] = {}
        self.publish_metrics = publish_metrics
        self._sampler = sampler
        self._root = root
        self.telemetry: NodeTelemetry | None = None
        self.unhealthy: set[int] = set()
        # GPU index -> physical XCD ids a GpuHealth verdict named as bad.
        self.unhealthy_xcds: dict[int, set[int]] = {}
        # Annotation key of FAULT_KINDS -> {GPU index: that kind's value}, from
        # the GpuHealth.detail of the last probe; {} for a kind with no fault.
        self.faults: dict[str, dict[int, dict]] = {k: {} for k in FAULT_KINDS}
        self._stop = threading.Event()
        self._threads: list[threading.Thread] = []
        self.host: HostInfo | None = None
        # With a kubelet on the node, the device plugins advertise amd.com/*
        # capacity; the agent must not write those fields (kubelet owns them).
        self.kubelet_managed = kubelet_managed
        self.device_plugins: list = []

    # --------------------------------------------------------------- objects
    def check_health(self, host: HostInfo) -> set[int]:
        return self.probe_health(host)[0]

    def probe_health(self, host: HostInfo) -> tuple[set[int], dict[int, set[int]]]:
        """(GPUs to withhold, bad XCDs per GPU). A `bool` from health_fn means
        the whole GPU; a GpuHealth with bad XCDs withholds an SPX GPU and only
        marks the XCDs of a partitioned one."""
        return self._probe_health(host)[:2]

    def _probe_health(self, host: HostInfo) -> tuple[set[int], dict[int, set[int]], dict[str, dict[int, dict]]]:
        """probe_health plus the faults of every kind of FAULT_KINDS per GPU.

        A kind that withholds the GPU (an HBM fault) does so whether the GPU
        is partitioned or not, and even when the same verdict names bad XCDs."""
        faults: dict[str, dict[int, dict]] = {k: {} for k in FAULT_KINDS}
        if self.health_fn is None:
            return set(), {}, faults
        bad: set[int] = set()
        xcds: dict[int, set[int]] = {}
        # HIP ordinals follow the KFD node order of the GPUs this process can
        # open; GPUs whose KFD node is hidden (other containers' devices) are
        # not probed. With no KFD info at all (fake hosts) use the index.
        visible = sorted((g for g in host.gpus if g.kfd_node is not None), key=lambda g: g.kfd_node)
        targets = [(i, g) for i, g in enumerate(visible)] if visible else [(g.index, g) for g in host.gpus]
        for ordinal, g in targets:
            try:
                r = self.health_fn(ordinal)
                withheld = False
                for key, kind in FAULT_KINDS.items() if isinstance(r, GpuHealth) else ():
                    v = r.detail.get(key) or {}
                    v = {int(x): _fault_value(f) for x, f in v.items() if f} if kind.per_xcd else dict(v)
                    if v:
                        faults[key][g.index] = v
                        withheld |= kind.withholds_gpu
                if isinstance(r, GpuHealth) and r.bad_xcds:
                    xcds[g.index] = set(r.bad_xcds)
                    if g.partitions == 1 or withheld:
                        bad.add(g.index)
                elif withheld:
                    bad.add(g.index)
                elif not (r.ok if isinstance(r, GpuHealth) else r):
                    bad.add(g.index)
            except Exception as e:  # noqa: BLE001
                log.warning("health probe GPU %d failed: %s", g.index, e)
                bad.add(g.index)
        return bad, xcds, faults

    @staticmethod
    def _fenced(gpus, xcd_faults) -> dict[int, tuple[int, int]]:
        """GPU index -> (XCDs, HBM GiB) in the partitions fenced by `xcd_faults`
        on the partitioned GPUs among `gpus`."""
        out = {}
        for g in gpus:
            parts = fenced_partitions(g.partitions, (xcd_faults or {}).get(g.index, ()))
            if g.partitions > 1 and parts:
                out[g.index] = (len(parts) * XCDS_PER_GPU // g.partitions, len(parts) * g.hbm_gib // g.partitions)
        return out

    def measure_bandwidth(self, host: HostInfo) -> None:
        """Partition bandwidth table per healthy GPU (HIP ordinal order, as
        check_health), measured the first time a GPU is seen."""
        if self.bandwidth_fn is None:
            return
        visible = sorted((g for g in host.gpus if g.kfd_node is not None), key=lambda g: g.kfd_node)
        targets = [(i, g) for i, g in enumerate(visible)] if visible else [(g.index, g) for g in host.gpus]
        now = time.monotonic()
        for ordinal, g in targets:
            if g.index in self.bandwidth or g.index in self.unhealthy:
                continue
            if now < self._bandwidth_retry_at.get(g.index, 0.0):
                continue
            try:
                self.bandwidth[g.index] = self.bandwidth_fn(ordinal)
                self._bandwidth_retry_at.pop(g.index, None)
            except Exception as e:  # noqa: BLE001
                log.warning("bandwidth probe GPU %d failed (next try in %.0f s): %s", g.index,
                            self.bandwidth_retry_s, e)
                self._bandwidth_retry_at[g.index] = now + self.bandwidth_retry_s

    def build_node(self, host: HostInfo, unhealthy: set[int] = frozenset(),
                   xcd_faults: dict[int, set[int]] | None = None,
                   faults: dict[str, dict[int, dict]] | None = None) -> dict:
        healthy = [g for g in host.gpus if g.index not in unhealthy]
        infos = [g.to_gpu_info() for g in healthy]
        mem_kib = max(0, host.memory_bytes // 1024 - self.reserved_memory_gib * (1 << 20))
        labels = dict(self.labels)
        parts = {g.memory_partition for g in host.gpus}
        if len(parts) == 1:
            labels[MEMORY_PARTITION_LABEL] = parts.pop()
        if host.xgmi_hive:
            labels[HIVE_LABEL] = f"{host.xgmi_hive:x}"
        node = mi355x_node(self.name, gpus=infos, cpu=str(max(1, host.cpus - self.reserved_cpu)),
                           memory=f"{mem_kib}Ki", pods=max(110, host.cpus), labels=labels,
                           taints=[UNHEALTHY_TAINT] if host.gpus and not healthy else None)
        if not host.gpus:  # a CPU-only node carries no GPU identity labels
            for k in ("amd.com/gpu.compute-partition", "amd.com/gpu.product", "amd.com/gpu.family"):
                node["metadata"]["labels"].pop(k, None)
        topo = json.loads(node["metadata"]["annotations"][TOPOLOGY_ANNOTATION])
        by_index = {g.index: g for g in healthy}
        for i, entry in enumerate(topo["gpus"]):
            g = by_index[infos[i].index]
            entry.update(bdf=g.bdf, uniqueId=g.unique_id, memoryPartition=g.memory_partition,
                         computePartition=g.compute_partition, xgmiLinks=len(g.xgmi_links),
                         xgmiLinkMBps=max((lk.bandwidth_mbps for lk in g.xgmi_links), default=0))
        topo["unhealthy"] = sorted(unhealthy)
        fenced_xcds = {str(i): sorted(x) for i, x in sorted((xcd_faults or {}).items()) if x}
        if fenced_xcds:
            topo["xcdFaults"] = fenced_xcds
        for key, kind in FAULT_KINDS.items():
            per_gpu = {}
            for i, v in sorted((faults or {}).get(key, {}).items()):
                v = {str(x): _fault_value(f) for x, f in sorted(v.items()) if f} if kind.per_xcd else dict(v)
                if v:
                    per_gpu[str(i)] = v
            if per_gpu:
                topo[key] = per_gpu
        node["metadata"]["annotations"][TOPOLOGY_ANNOTATION] = json.dumps(topo, sort_keys=True)
        if self.bandwidth:
            node["metadata"]["annotations"][BANDWIDTH_ANNOTATION] = json.dumps(
                {str(i): t for i, t in sorted(self.bandwidth.items()) if i not in unhealthy}, sort_keys=True)
        # Capacity reports the hardware; allocatable withholds unhealthy GPUs.
        cap = dict(node["status"]["allocatable"])
        cap[GPU] = str(len(host.gpus))
        cap[GPU_XCD] = str(XCDS_PER_GPU * len(host.gpus))
        cap[GPU_MEMORY] = str(sum(g.hbm_gib for g in host.gpus))
        node["status"]["capacity"] = cap
        fenced = self._fenced(healthy, xcd_faults)
        if fenced:
            alloc = node["status"]["allocatable"]
            alloc[GPU_XCD] = str(int(alloc[GPU_XCD]) - sum(x for x, _ in fenced.values()))
            alloc[GPU_MEMORY] = str(int(alloc[GPU_MEMORY]) - sum(m for _, m in fenced.values()))
        if self.kubelet_managed:
            for k in (GPU, GPU_XCD, GPU_MEMORY):
                node["status"]["allocatable"].pop(k, None)
                node["status"]["capacity"].pop(k, None)
        node["status"]["conditions"] = [self._ready_condition()]
        node["status"]["nodeInfo"] = {"architecture": "amd64", "operatingSystem": "linux",
                                      "kubeletVersion": "v1.23.3-xsched-agent"}
        return node

    @staticmethod
    def _ready_condition() -> dict:
        now = _now()
        return {"type": "Ready", "status": "True", "reason": "AgentReady", "message": "MI355X node agent is posting",
                "lastHeartbeatTime": now, "lastTransitionTime": now}

    def build_nrt(self, host: HostInfo, unhealthy: set[int] = frozenset(),
                  xcd_faults: dict[int, set[int]] | None = None) -> dict:
        sockets = max(1, len(host.numa_nodes))
        cpus = [len(host.numa_cpus.get(s, [])) or host.cpus // sockets for s in range(sockets)]
        mem_gib = host.memory_bytes // (1 << 30) // sockets
        gpus = [g.to_gpu_info() for g in host.gpus if g.index not in unhealthy]
        nrt = mi355x_nrt(self.name, gpus=gpus, cpu_per_socket=min(cpus), memory_per_socket_gib=mem_gib,
                         sockets=sockets)
        for z, c in zip(nrt["zones"], cpus):
            for r in z["resources"]:
                if r["name"] == "cpu":
                    r["capacity"] = r["allocatable"] = r["available"] = str(c)
        fenced = self._fenced([g for g in host.gpus if g.index not in unhealthy], xcd_faults)
        for g in host.gpus:
            if g.index not in fenced or not 0 <= max(g.numa, 0) < len(nrt["zones"]):
                continue
            lost = dict(zip((GPU_XCD, GPU_MEMORY), fenced[g.index]))
            for r in nrt["zones"][max(g.numa, 0)]["resources"]:
                if r["name"] in lost:  # capacity still reports the hardware
                    r["allocatable"] = r["available"] = str(int(r["allocatable"]) - lost[r["name"]])
        return nrt

    # --------------------------------------------------------------- publish
    def _upsert(self, kind: str, obj: dict, keep_spec: bool) -> None:
        name = obj["metadata"]["name"]
        for _ in range(5):
            cur = self.client.get(kind, "", name)
            if cur is None:
                try:
                    self.client.create(kind, obj)
                    return
                except Exception as e:  # noqa: BLE001
                    if not is_conflict(e):
                        raise
                    continue
            body = json.loads(json.dumps(obj))
            if keep_spec:
                # Node spec (cordon, admin taints) belongs to the cluster, not
                # the agent; keep it, only manage our own taint.
                spec = dict(cur.get("spec") or {})
                taints = [t for t in spec.get("taints") or [] if t.get("key") != UNHEALTHY_TAINT["key"]]
                taints += [t for t in (obj.get("spec") or {}).get("taints") or []]
                if taints:
                    spec["taints"] = taints
                else:
                    spec.pop("taints", None)
                body["spec"] = spec
                md = body["metadata"]
                md["labels"] = {**(cur["metadata"].get("labels") or {}), **(md.get("labels") or {})}
                md["annotations"] = {**(cur["metadata"].get("annotations") or {}), **(md.get("annotations") or {})}
            body["metadata"]["resourceVersion"] = cur["metadata"].get("resourceVersion")
            try:
                self.client.update(kind, body)
                return
            except Exception as e:  # noqa: BLE001
                if not is_conflict(e):
                    raise
        raise RuntimeError(f"could not update {kind}/{name}: persistent conflicts")

    def sync(self) -> HostInfo:
        host = self.host_fn()
        self.unhealthy, self.unhealthy_xcds, self.faults = self._probe_health(host)
        self.measure_bandwidth(host)
        for dp in self.device_plugins:
            dp.host = host
            dp.set_unhealthy(self.unhealthy)
            dp.set_unhealthy_xcds(self.unhealthy_xcds)
        self._upsert("nodes", self.build_node(host, self.unhealthy, self.unhealthy_xcds, self.faults), keep_spec=True)
        self._upsert("noderesourcetopologies", self.build_nrt(host, self.unhealthy, self.unhealthy_xcds),
                     keep_spec=False)
        self.host = host
        return host

    def post_heartbeat(self) -> None:
        self.client.patch("nodes", "", self.name, {"status": {"conditions": [self._ready_condition()]}})

    def sample_and_publish(self) -> dict | None:
        if self.telemetry is None:
            self.telemetry = NodeTelemetry(self.name, self._sampler or HostSampler(self._root))
        self.telemetry.sample()
        doc = self.telemetry.watcher_metrics("15m")
        if self.publish_metrics:
            publish(self.client, doc)
        return doc

    # ------------------------------------------------------------------ run
    def _loop(self, period: float, fn: Callable[[], object]) -> None:
        while not self._stop.wait(period):
            try:
                fn()
            except Exception:  # noqa: BLE001
                log.exception("node agent %s: periodic task failed", self.name)

    def start(self) -> "NodeAgent":
        self.sync()
        if self.publish_metrics:
            self.sample_and_publish()
        loops = [(self.heartbeat, self._heartbeat_and_resync)]
        if self.publish_metrics:
            loops.append((self.telemetry_period, self.sample_and_publish))
        for period, fn in loops:
            t = threading.Thread(target=self._loop, args=(period, fn), daemon=True, name="node-agent")
            t.start()
            self._threads.append(t)
        return self

    def _heartbeat_and_resync(self) -> None:
        host = self.host_fn()
        unhealthy, xcds, faults = self._probe_health(host)
        changed = (self.host is None or [g.to_gpu_info() for g in host.gpus] != [g.to_gpu_info() for g in self.host.gpus]
                   or unhealthy != self.unhealthy or xcds != self.unhealthy_xcds or faults != self.faults)
        if changed:
            self.sync()
        else:
            self.post_heartbeat()

    def stop(self) -> None:
        self._stop.set()
        for t in self._threads:
            t.join(timeout=5)


def hip_health_fn(sweep: bool = False, sweep_period_s: float = 600.0, sweep_args: dict | None = None,
                  matrix: bool = False, matrix_formats: list | None = None,
                  matrix_args: dict | None = None, hbm: bool = False, hbm_gib: float | None = None,
                  hbm_args: dict | None = None, regfile: bool = False,
                  regfile_args: dict | None = None, lane: bool = False, lane_paths: list | None = None,
                  lane_args: dict | None = None, valu: bool = False, valu_units: list | None = None,
                  valu_args: dict | None = None, mem: bool = False, mem_routes: list | None = None,
                  mem_args: dict | None = None, scalar: bool = False, scalar_parts: list | None = None,
                  scalar_args: dict | None = None, consensus: bool = False, consensus_parts: list | None = None,
                  consensus_args: dict | None = None, fetch: bool = False, fetch_parts: list | None = None,
                  fetch_args: dict | None = None) -> Callable[[int], "bool | GpuHealth"]:
    """Health callback backed by the HIP probes (HBM pattern + checksum and an
    MFMA tile check per GPU).

    Each kind of SWEEP_KINDS, SCALAR_SWEEP_KIND, CONSENSUS_SWEEP_KIND, FETCH_SWEEP_KIND and MEM_SWEEP_KIND, in the
    order they run,
    has a switch `<kind>` that also runs that per-CU sweep of HipProbe (`sweep`: the CU sweep), `<kind>_args` for its keywords
    and, where it sweeps named parts, `<kind>_<parts>` to select some (None for
    all). Its summary and, the CU sweep apart, its {xcd: fault} go into the
    verdict's detail under the kind's keys. A fault is the list of the failed
    formats, paths, units, scalar parts, consensus parts, fetch parts or routes; of `regfile`, {"files": [...], "cells": n,
    "flipMask": "0x...", "simds": n}. The VALU sweep's failed steps are in
    detail["valuSweep"]. The consensus sweep judges a CU by the vote of the
    GPU's CUs; a part the vote could not decide (detail["consensusSweep"]["undecided"])
    is logged at WARNING, fails nothing and touches no other sweep's verdict.
    The memory sweep holds an arena in HBM while it runs;
    where that cannot be had the device is logged as unswept, which neither
    fails it nor touches the other sweeps' verdicts.
    The callback runs on every heartbeat, so the sweeps' verdict is reused for
    `sweep_period_s`. On a device that shows all 8 XCDs the verdict is a
    GpuHealth naming the bad physical XCDs of any of these sweeps; a
    partition device numbers its XCDs logically, so there a failed sweep fails
    the device as a whole (a plain bool). CUs a sweep could not reach are
    logged, never counted as failed.

    `hbm`: also run the HBM sweep (HipProbe.hbm_sweep over `hbm_gib` GiB, None
    for all free HBM less its reserve; `hbm_args` are its other keywords) under
    the same period, with or without the other two. It holds the memory it
    tests for its duration, so a tenant's allocation can fail in that window:
    hence the GiB cap and the period. A fault makes the verdict, on every kind
    of device, a GpuHealth with ok False, the bad XCDs of the other sweeps,
    detail["hbmSweep"] (the summary) and detail["hbmFaults"] (what the agent
    publishes); the agent withholds such a GPU as a whole. A device on which no
    memory could be had is logged as unswept and a sweep that got less than it
    asked for as short; neither fails the device."""
    given = locals()  # the parameters by name, for SWEEP_KINDS
    from ..ops.hip_probe import HBM_UNSWEPT, MEM_UNSWEPT, ProbeError, probe

    p = probe()
    last: dict[int, tuple[float, object]] = {}  # dev -> (monotonic time, sweep verdict)
    # The enabled kinds, each with the keywords of its probe method.
    per_cu_sweeps = [(k, {**({k.selection: given[f"{k.enabled_by}_{k.selection}"]} if k.selection else {}),
                          **(given[f"{k.enabled_by}_args"] or {})})
                     for k in SWEEP_KINDS + (SCALAR_SWEEP_KIND, CONSENSUS_SWEEP_KIND, FETCH_SWEEP_KIND, MEM_SWEEP_KIND)
                     if given[k.enabled_by]]

    def sweep_verdict(dev: int):
        now = time.monotonic()
        if dev in last and now - last[dev][0] < sweep_period_s:
            return last[dev][1]
        bad: set[int] = set()
        detail: dict = {}
        for k, keywords in per_cu_sweeps:
            try:
                s = getattr(p, k.method)(dev, **keywords)["summary"]
            except ProbeError as e:
                if k is not MEM_SWEEP_KIND or e.rc != MEM_UNSWEPT:
                    raise
                log.warning("mem sweep GPU %d: unswept, no memory could be had (%s)", dev, e)
                continue
            fault_of = k.fault_of
            found = {int(x): fault_of(v) for x, v in s["xcds"].items() if fault_of(v)} if fault_of else s["bad_xcds"]
            log.log(logging.WARNING if s["bad_xcds"] else logging.INFO,
                    "%s sweep GPU %d: %d CUs on %d XCDs in %.2f ms (%d launch(es)), covered=%s uncovered=%s "
                    "%s=%s", k.label, dev, s["cus_seen"], len(s["xcds"]), s["ms"], s["rounds"], s["covered"],
                    {x: n for x, n in s["uncovered"].items() if n}, "bad_xcds" if fault_of is None else "faults", found)
            if s.get("failed_steps"):
                log.warning("%s sweep GPU %d: failed steps %s", k.label, dev, s["failed_steps"])
            if s.get("undecided"):
                log.warning("%s sweep GPU %d: no majority for %s: undecided, nothing failed for it", k.label, dev,
                            s["undecided"])
            bad |= set(s["bad_xcds"])
            detail[k.summary_key] = s
            if k.faults_key:
                detail[k.faults_key] = found
        hbm_faults: dict = {}
        if hbm:
            h = None
            try:
                h = p.hbm_sweep(dev, nbytes=int(hbm_gib * (1 << 30)) if hbm_gib else 0, **(hbm_args or {}))["summary"]
            except ProbeError as e:
                if e.rc != HBM_UNSWEPT:
                    raise
                log.warning("hbm sweep GPU %d: unswept, no memory could be had (%s)", dev, e)
            if h is not None:
                gib = h["bytes_tested"] / (1 << 30)
                log.log(logging.WARNING if h["bad_vectors"] or h["short"] else logging.INFO,
                        "hbm sweep GPU %d: %.2f GiB%s in %s ms (%s GB/s), from_dram=%s bad_vectors=%d bad_bits=%d "
                        "flip_mask=%s bad_chunks=%s", dev, gib, " (short: less than asked for)" if h["short"] else "",
                        h["ms"], h["GBps"], h["from_dram"], h["bad_vectors"], h["bad_bits"], h["flip_mask"],
                        h["bad_chunks"])
                if h["bad_vectors"]:
                    hbm_faults = {"badVectors": h["bad_vectors"], "badBits": h["bad_bits"],
                                  "flipMask": h["flip_mask"], "oneToZero": h["one_to_zero"],
                                  "zeroToOne": h["zero_to_one"], "testedGiB": round(gib, 3),
                                  "fromDram": h["from_dram"], "readerXcds": list(h["reader_xcds"])}
                detail["hbmSweep"] = h
                detail["hbmFaults"] = hbm_faults
        if hbm_faults:
            v = GpuHealth(False, frozenset(bad), detail)
        elif int(p.props(dev)["computeUnits"]) // 32 >= XCDS_PER_GPU:
            v = GpuHealth(not bad, frozenset(bad), detail)
        else:
            v = not bad
        last[dev] = (now, v)
        return v

    def check(dev: int):
        # HBM pattern/checksum and an exact-integer MFMA tile: a GPU whose matrix
        # cores mis-compute is withheld even if its memory checks out.
        ok = bool(p.health(dev)["healthy"]) and bool(p.mfma_check(dev)["healthy"])
        if not (per_cu_sweeps or hbm) or not ok:
            return ok
        return sweep_verdict(dev)

    return check


def hip_bandwidth_fn(nbytes: int = 1 << 30, iters: int = 10) -> Callable[[int], dict]:
    """Partition bandwidth table backed by the HIP XCD-pinned streaming probe
    (read and copy over a 1 GiB working set per CPX/QPX/DPX/SPX XCD set)."""
    from ..ops.hip_probe import probe

    p = probe()
    return lambda dev: p.partition_table(dev, nbytes, iters)


def run_forever(agent: NodeAgent) -> None:  # pragma: no cover - CLI
    agent.start()
    try:
        while True:
            time.sleep(3600)
    except KeyboardInterrupt:
        agent.stop()
