"""Gang records, kept in the lister's per-gang entry (csrc/scheduler/gang.h).

The record of a gang is opened by the informer at the first member's enqueue,
updated by the scheduling thread at Permit and by the binders (a pool of
threads, one member each) at bind, and moved to the collected records by the
binder that binds the last member. These tests pin what the records said
before they moved into the entry: one record per gang with its size, node
set, hostable verdict and enqueue <= admit <= bound; none for a gang deleted
before admission; a record of its own for a successor of the same name."""
import time

from flex_gpu_scheduler_amd import load_config, new_scheduler
from flex_gpu_scheduler_amd.models import GPU, make_pod, make_pod_group, mi355x_node
from flex_gpu_scheduler_amd.models.mi355x import INDEX_ANNOTATION, mi355x_nrt
from flex_gpu_scheduler_amd.utils.workload import flagship_config


def wait_for(pred, timeout=10.0):
    t0 = time.time()
    while not pred():
        if time.time() - t0 > timeout:
            return False
        time.sleep(0.002)
    return True


def scheduler(store):
    cfg = flagship_config(permit_wait_s=10, denied_s=20, gang_colocation="Preferred")
    s = new_scheduler(store, load_config(cfg), podInitialBackoffSeconds=1, podMaxBackoffSeconds=10)
    s.start()
    return s


def add_node(store, name, busy=0):
    store.create("nodes", mi355x_node(name, mode="spx"))
    store.create("noderesourcetopologies", mi355x_nrt(name))
    for i in range(busy):
        store.create("pods", make_pod(f"busy-{name}-{i}", limits={GPU: "1"}, node_name=name,
                                      annotations={INDEX_ANNOTATION: str(i)}))


def submit(store, name, size, members=None):
    store.create("podgroups", make_pod_group(name, "default", size))
    names = [f"{name}-r{r}" for r in range(size if members is None else members)]
    for n in names:
        store.create("pods", make_pod(n, limits={GPU: "1"}, pod_group=name))
    return names


def bound(store, names):
    return all(store.get("pods", "default", n)["spec"].get("nodeName") for n in names)


def test_one_record_per_gang_bound_by_several_threads(store):
    """A gang of 8 that has to split 4 + 4 and five gangs of 4 that each fit a
    node, the five submitted together: the members of each gang are bound by
    different binder threads, and each gang yields exactly one record."""
    add_node(store, "split-0", busy=4)
    add_node(store, "split-1", busy=4)
    s = scheduler(store)
    try:
        assert s.stats()["bind_threads"] > 1
        big = submit(store, "big", 8)
        assert wait_for(lambda: bound(store, big))
        for i in range(5):
            add_node(store, f"mi-{i}")
        small = {f"g{i}": submit(store, f"g{i}", 4) for i in range(5)}
        assert wait_for(lambda: all(bound(store, m) for m in small.values()))
        assert wait_for(lambda: len(s.gang_records()) >= 6)
        recs = s.gang_records(True)
        assert sorted(r["pod_group"] for r in recs) == sorted(["default/big"] + [f"default/{g}" for g in small])
        by_name = {r["pod_group"]: r for r in recs}
        r = by_name["default/big"]
        assert (r["size"], r["nodes"], r["hostable"]) == (8, 2, 0)
        assert 0 < r["first_enqueue_us"] <= r["admit_us"] <= r["bound_us"]
        for g in small:
            r = by_name[f"default/{g}"]
            assert (r["size"], r["nodes"], r["hostable"]) == (4, 1, 1), r
            assert 0 < r["first_enqueue_us"] <= r["admit_us"] <= r["bound_us"]
        assert s.gang_records() == []  # collected: nothing is reported twice
    finally:
        s.stop()


def test_deleted_before_admission_leaves_none_and_successor_starts_its_own(store):
    add_node(store, "mi-0")
    s = scheduler(store)
    try:
        # Two of four members: the gang waits in PreFilter and is never admitted.
        first = submit(store, "g", 4, members=2)
        assert wait_for(lambda: s.stats()["attempts"] >= 2)
        for n in first:
            store.delete("pods", "default", n)
        store.delete("podgroups", "default", "g")
        # A marker gang after the deletion gives a point on the scheduler's clock.
        mark = submit(store, "mark", 1)
        assert wait_for(lambda: bound(store, mark))
        assert wait_for(lambda: len(s.gang_records()) == 1)
        (m,) = s.gang_records(True)
        assert m["pod_group"] == "default/mark" and m["size"] == 1
        # The successor of the same name: one record, on its own timeline.
        second = submit(store, "g", 2)
        assert wait_for(lambda: bound(store, second))
        assert wait_for(lambda: len(s.gang_records()) == 1)
        (r,) = s.gang_records(True)
        assert r["pod_group"] == "default/g" and r["size"] == 2 and r["nodes"] == 1
        assert m["bound_us"] <= r["first_enqueue_us"] <= r["admit_us"] <= r["bound_us"]
    finally:
        s.stop()
