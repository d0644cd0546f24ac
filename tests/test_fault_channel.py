"""Every fault kind a health verdict can carry, at once: the node agent keeps
them, publishes each under its own key of the topology annotation, withholds
what they withhold, and re-publishes the node when any one of them changes."""
import json

import pytest

from flex_gpu_scheduler_amd.control import LocalClient
from flex_gpu_scheduler_amd.control.node_agent import GpuHealth, NodeAgent
from flex_gpu_scheduler_amd.gpu.discovery import fake_host
from flex_gpu_scheduler_amd.models import GPU, GPU_MEMORY, GPU_XCD, TOPOLOGY_ANNOTATION

REGISTER = {"files": ["agpr"], "cells": 64, "flipMask": "0x00000200", "simds": 1}
HBM = {"badVectors": 1, "badBits": 1, "flipMask": f"{0x10 << 32:032x}", "oneToZero": 0, "zeroToOne": 1,
       "testedGiB": 4.0, "fromDram": True, "readerXcds": [3]}

# kind -> (what the first verdict carries, the same fault grown, how it is published)
KINDS = {
    "matrixFaults": ({5: ["fp8", "mxfp4"], 2: []}, {5: ["fp8", "mxfp4", "i8"], 2: []},
                     lambda v: {"0": {"5": list(v[5])}}),
    "registerFaults": ({5: REGISTER, 2: {}}, {5: dict(REGISTER, cells=128), 2: {}},
                       lambda v: {"0": {"5": dict(v[5])}}),
    "laneFaults": ({5: ["ldstr", "ldsdma"], 2: []}, {5: ["ldstr"], 2: []}, lambda v: {"0": {"5": list(v[5])}}),
    "hbmFaults": (HBM, dict(HBM, badVectors=9, badBits=12), lambda v: {"1": dict(v)}),
}
PER_XCD = ("matrixFaults", "registerFaults", "laneFaults")

# The annotation of the first verdict, byte for byte.
TOPOLOGY = (
    '{"gpus": [{"bdf": "0000:10:00.0", "computePartition": "CPX", "cus": 256, "hbmGiB": 288, "index": 0, '
    '"memoryPartition": "NPS1", "numa": 0, "partitions": 8, "uniqueId": "", "xgmiLinkMBps": 76000, "xgmiLinks": 1}], '
    '"hbmFaults": {"1": {"badBits": 1, "badVectors": 1, "flipMask": "00000000000000000000001000000000", '
    '"fromDram": true, "oneToZero": 0, "readerXcds": [3], "testedGiB": 4.0, "zeroToOne": 1}}, '
    '"laneFaults": {"0": {"5": ["ldstr", "ldsdma"]}}, "matrixFaults": {"0": {"5": ["fp8", "mxfp4"]}}, '
    '"registerFaults": {"0": {"5": {"cells": 64, "files": ["agpr"], "flipMask": "0x00000200", "simds": 1}}}, '
    '"unhealthy": [1], "xcdFaults": {"0": [5]}, "xgmi": {"linkGBps": 153.0, "links": 7, "topology": "fullmesh"}}')


class Verdicts:
    """health_fn of a two-GPU host: GPU 0 has the per-XCD faults on XCD 5, GPU 1 the HBM fault."""

    def __init__(self):
        self.detail = {k: first for k, (first, _, _) in KINDS.items()}

    def __call__(self, dev):
        if dev == 0:
            return GpuHealth(False, {5}, {k: self.detail[k] for k in PER_XCD})
        return GpuHealth(False, (), {"hbmFaults": self.detail["hbmFaults"]}) if self.detail["hbmFaults"] else True


class CountingClient(LocalClient):
    def __init__(self, store):
        super().__init__(store)
        self.node_updates, self.node_patches = 0, 0

    def update(self, kind, obj):
        self.node_updates += kind == "nodes"
        return super().update(kind, obj)

    def patch(self, kind, ns, name, body):
        self.node_patches += kind == "nodes"
        return super().patch(kind, ns, name, body)


def synced(store):
    verdicts = Verdicts()
    agent = NodeAgent(CountingClient(store), "n", host_fn=lambda: fake_host(2, "CPX"), publish_metrics=False,
                      health_fn=verdicts)
    agent.sync()
    return agent, verdicts


def annotation(store) -> str:
    return store.get("nodes", "", "n")["metadata"]["annotations"][TOPOLOGY_ANNOTATION]


def test_all_kinds_at_once(store):
    agent, _ = synced(store)
    assert annotation(store) == TOPOLOGY
    assert agent.unhealthy == {1} and agent.unhealthy_xcds == {0: {5}}
    assert agent.faults["matrixFaults"] == {0: {5: ["fp8", "mxfp4"]}}
    assert agent.faults["registerFaults"] == {0: {5: REGISTER}}
    assert agent.faults["laneFaults"] == {0: {5: ["ldstr", "ldsdma"]}}
    assert agent.faults["hbmFaults"] == {1: HBM}
    # GPU 1 is withheld as a whole; of GPU 0 only the partition that owns XCD 5 is fenced
    host = fake_host(2, "CPX")
    node = store.get("nodes", "", "n")
    alloc, cap = node["status"]["allocatable"], node["status"]["capacity"]
    assert cap[GPU_XCD] == "16" and alloc[GPU_XCD] == "7"
    assert int(cap[GPU_MEMORY]) == 2 * host.gpus[0].hbm_gib
    assert int(alloc[GPU_MEMORY]) == host.gpus[0].hbm_gib - host.gpus[0].hbm_gib // 8
    assert cap[GPU] == "2" and alloc[GPU] == "1"


@pytest.mark.parametrize("kind", list(KINDS))
def test_heartbeat_follows_one_kind(store, kind):
    agent, verdicts = synced(store)
    client = agent.client
    _, grown, published = KINDS[kind]
    others = {k: json.loads(annotation(store))[k] for k in KINDS if k != kind}

    # nothing changed: the heartbeat alone
    updates = client.node_updates
    agent._heartbeat_and_resync()
    assert client.node_updates == updates and client.node_patches == 1
    assert annotation(store) == TOPOLOGY

    # only this kind's value changed: the node is published again
    verdicts.detail[kind] = grown
    agent._heartbeat_and_resync()
    assert client.node_updates == updates + 1 and client.node_patches == 1
    topo = json.loads(annotation(store))
    assert topo[kind] == published(grown)
    assert {k: topo[k] for k in others} == others and topo["xcdFaults"] == {"0": [5]}

    # and again nothing
    agent._heartbeat_and_resync()
    assert client.node_updates == updates + 1 and client.node_patches == 2

    # cleared: the key leaves the annotation, the others stay
    verdicts.detail[kind] = {}
    agent._heartbeat_and_resync()
    assert client.node_updates == updates + 2
    topo = json.loads(annotation(store))
    assert kind not in topo and {k: topo[k] for k in others} == others
    assert topo["unhealthy"] == ([] if kind == "hbmFaults" else [1])
