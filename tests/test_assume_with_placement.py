"""What a pod looks like once the cycle has assumed it with its GPU placement
(FlexGPU::prepare_assumed) must be what it looked like when Reserve annotated
it after the assume: these tests pin the observable side over a 4-node shard
(1 CPX node, 3 SPX nodes) running the flagship workload. They hold on the
tree before that change as well; that is their point.

After each of two waves is bound: every GPU pod carries the index annotation,
every pod on partitions also the partition annotation, no two pods of a node
hold the same whole GPU or exclusive partition, and the cache debugger finds
no accounting mismatch; after deletion the cache drains. With binds failing
(Unreserve, forget, retry after a fused assume) every pod still ends bound
and the cache is clean. A pod asking for a whole GPU and XCDs stays Pending
with FlexGPU's conflict message."""
import time

import pytest

from flex_gpu_scheduler_amd.models import GPU, make_pod
from flex_gpu_scheduler_amd.models.mi355x import GPU_MEMORY, GPU_XCD, INDEX_ANNOTATION, PARTITION_ANNOTATION
from flex_gpu_scheduler_amd.utils.benchrun import Shard
from flex_gpu_scheduler_amd.utils.workload import ClusterSpec, flagship_config

NS = "assume"


def wait_for(pred, timeout=20.0):
    t0 = time.time()
    while not pred():
        if time.time() - t0 > timeout:
            return False
        time.sleep(0.002)
    return True


def limits_of(pod):
    out = {}
    for c in pod["spec"]["containers"]:
        out.update((c.get("resources") or {}).get("limits") or {})
    return out


def create(shard, wave):
    for groups_js, pods_js in wave.chunks_json():
        if groups_js != "[]":
            shard.store.create_many("podgroups", groups_js)
        if pods_js != "[]":
            shard.store.create_many("pods", pods_js)


def wait_bound_and_quiet(shard, n_before, n):
    assert shard.sched.wait_bound(n_before + n, 30.0), (shard.sched.stats(), shard.sched.queue_counts())
    assert wait_for(lambda: shard.sched.stats()["inflight_bindings"] == 0)


def clean_cache(shard):
    """The cache debugger's report once the informer has caught up."""
    report = {}

    def clean():
        report.clear()
        report.update(shard.sched.check_cache())
        return report["clean"]

    wait_for(clean, 5.0)
    return report


def check_placements(pods):
    """Annotations of the bound pods: present, well-formed, and disjoint per node."""
    whole, exclusive, shared = {}, {}, {}  # node -> GPUs / (gpu, partition) pairs
    for p in pods:
        name, node = p["metadata"]["name"], p["spec"].get("nodeName")
        assert node, f"{name} is not bound"
        lim, ann = limits_of(p), p["metadata"].get("annotations") or {}
        if not any(k in lim for k in (GPU, GPU_XCD, GPU_MEMORY)):
            assert INDEX_ANNOTATION not in ann and PARTITION_ANNOTATION not in ann, (name, ann)
            continue
        assert ann.get(INDEX_ANNOTATION), (name, ann)
        gpus = [int(x) for x in ann[INDEX_ANNOTATION].split(",")]
        assert all(0 <= g < 8 for g in gpus) and len(set(gpus)) == len(gpus), (name, ann)
        if GPU in lim:
            assert PARTITION_ANNOTATION not in ann, (name, ann)
            assert len(gpus) == int(lim[GPU]), (name, ann)
            for g in gpus:
                assert g not in whole.setdefault(node, set()), f"{name}: GPU {g} of {node} given twice"
                whole[node].add(g)
            continue
        # A pod on partitions: XCDs (exclusive partitions of one GPU) or an HBM slice (one shared partition).
        assert ann.get(PARTITION_ANNOTATION), (name, ann)
        parts = [tuple(int(x) for x in pair.split(":")) for pair in ann[PARTITION_ANNOTATION].split(",")]
        assert len(gpus) == 1 and all(g == gpus[0] and 0 <= q < 8 for g, q in parts), (name, ann)
        if GPU_XCD in lim:
            assert len(parts) == int(lim[GPU_XCD]), (name, ann)  # CPX: one XCD per partition
            for gq in parts:
                assert gq not in exclusive.setdefault(node, set()), f"{name}: partition {gq} of {node} given twice"
                exclusive[node].add(gq)
        else:
            assert len(parts) == 1, (name, ann)
            shared.setdefault(node, set()).add(parts[0])
    for node in set(whole) | set(exclusive) | set(shared):
        w, e, s = whole.get(node, set()), exclusive.get(node, set()), shared.get(node, set())
        assert not (e & s), f"{node}: exclusive partitions also hold HBM slices: {sorted(e & s)}"
        assert not (w & {g for g, _ in e | s}), f"{node}: whole GPUs also partitioned out"
    return whole, exclusive, shared


@pytest.fixture
def shard():
    sh = Shard(ClusterSpec(nodes=4), namespace=NS, seed=3,
               config=flagship_config(permit_wait_s=5, denied_s=1),
               options={"podInitialBackoffSeconds": 0.01, "podMaxBackoffSeconds": 0.05})
    try:
        yield sh
    finally:
        sh.close()


def test_two_waves_bound_with_consistent_placements(shard):
    bound = 0
    for step in range(2):
        wave = shard.wave(step)
        kinds = {k for p in wave.pods for k in limits_of(p)}
        assert {GPU, GPU_XCD, GPU_MEMORY} <= kinds  # the wave has all three kinds of GPU pod
        create(shard, wave)
        wait_bound_and_quiet(shard, bound, len(wave.pods))
        bound += len(wave.pods)
        pods = shard.store.list("pods", NS)[0]
        assert len(pods) == len(wave.pods)
        whole, exclusive, shared = check_placements(pods)
        assert whole and exclusive and shared
        report = clean_cache(shard)
        assert report["clean"], report
        assert report["accounting"] == [], report
        shard.store.delete_all("pods", NS)
        shard.store.delete_all("podgroups", NS)
        assert shard.sched.wait_cache_empty(20.0)
    assert shard.sched.stats()["bound"] == bound


def test_failed_binds_are_retried_after_a_fused_assume(shard):
    """The first binds fail with a server error: fail_assumed runs Unreserve
    (which strips the placement from the assumed pod) and forgets the pod; the
    retries bind every pod, and nothing is left accounted twice."""
    wave = shard.wave(0)
    shard.store.add_fault("bind", "pods", fail_prob=1.0, remaining=7)
    create(shard, wave)
    assert shard.sched.wait_bound(len(wave.pods), 30.0), (shard.sched.stats(), shard.sched.queue_counts())
    assert wait_for(lambda: shard.sched.stats()["inflight_bindings"] == 0)
    shard.store.clear_faults()
    assert shard.sched.stats()["bind_failures"] >= 7
    pods = shard.store.list("pods", NS)[0]
    assert len(pods) == len(wave.pods)
    check_placements(pods)
    report = clean_cache(shard)
    assert report["clean"], report
    assert report["accounting"] == [], report
    shard.store.delete_all("pods", NS)
    shard.store.delete_all("podgroups", NS)
    assert shard.sched.wait_cache_empty(20.0)


def test_conflicting_demand_stays_pending(shard):
    shard.store.create("pods", make_pod("both", NS, requests={"cpu": "1"}, limits={GPU: "1", GPU_XCD: "2"}))

    def condition():
        p = shard.store.get("pods", NS, "both")
        for c in (p.get("status") or {}).get("conditions") or []:
            if c.get("type") == "PodScheduled":
                return c
        return None

    assert wait_for(lambda: condition() is not None, 10.0)
    c = condition()
    assert c["status"] == "False" and c["reason"] == "Unschedulable", c
    assert "pod conflict resources" in c["message"], c
    p = shard.store.get("pods", NS, "both")
    assert not p["spec"].get("nodeName")
    assert (p["status"].get("phase") or "Pending") == "Pending"
    assert INDEX_ANNOTATION not in (p["metadata"].get("annotations") or {})
    assert shard.sched.stats()["bound"] == 0
    assert shard.sched.check_cache()["clean"]
