"""vo_kfstore_update_connections[_dev] (KeyFrame::updateConnections on the device, keyframe.cpp:69-198) against the model
tests/connections_ref.py.  Every comparison is exact: the state is integers."""
import numpy as np
import pytest

import connections_inputs as ci
import test_gpu_local_map as lm
from connections_ref import Connections

pytestmark = pytest.mark.gpu

ctx = lm.ctx   # (its module fixture: the relocalisation inputs of the end-to-end test)


def _enabled_store(vo, kfs, max_features, max_keyframes=None):
    s = vo.KeyFrameStore(max_keyframes or len(kfs), max_features)
    s.enable_connections()
    for kf in kfs:
        s.insert(ci.device_arrays(kf))
    return s


def _states(store):
    return [store.connections(k) for k in range(len(store))]


def _assert_equal(store, model):
    size = len(store)
    for k in range(size):
        assert store.connections(k) == model.state(k, size), k


@pytest.mark.parametrize("case", ci.hand_cases(), ids=lambda c: c["name"])
def test_hand_made_case(vo, case):
    store = _enabled_store(vo, case["store"], ci.NK_HAND)
    assert len(store) == ci.K_HAND
    snap = []
    for step in case["script"]:
        if step[0] == "points":
            a = ci.device_arrays(dict(ids=step[2], flags=step[3]))
            store.update_points(step[1], a["flags"], a["points"], a["ids"], a["point_desc"], a["min_dist"], a["max_dist"])
        else:
            store.update_connections(step[1])
            snap.append(_states(store))
    assert snap == ci.run_model(case["store"], case["script"])[1]
    assert case["check"](snap)
    assert store.connections_status() == 0


def test_random_interleaved_script(vo):
    """40 key-frames x 96 features from a sliding id window (adjacent key-frames share 0-40 ids), duplicated ids, cleared
    flags; insert / insert_dev / update_points interleaved with update calls in host and device form, lists with repeats"""
    import torch
    rng = np.random.default_rng(11)
    kfs = ci.sliding_window_store(rng, 40, 96, 160, 50, 170)
    store = vo.KeyFrameStore(44, 96)
    store.enable_connections()
    model, held, keep = Connections(), [], []

    def insert(lo, hi, dev):
        for kf in kfs[lo:hi]:
            a = ci.device_arrays(kf)
            if dev:
                a = {key: torch.from_numpy(v).cuda() for key, v in a.items()}
                keep.append(a)
                store.insert_dev(a)
            else:
                store.insert(a)
            held.append(dict(ids=list(kf["ids"]), flags=list(kf["flags"])))

    def update(lst, dev):
        if dev:
            keep.append(torch.tensor(lst, dtype=torch.int32).cuda())
            store.update_connections(keep[-1])
        else:
            store.update_connections(lst)
        model.update_list(held, lst)
        _assert_equal(store, model)

    def points(k):
        kf = held[k]
        n = len(kf["ids"])
        other = held[(k + 2) % len(held)]["ids"]
        kf["ids"] = [int(other[i]) if rng.random() < 0.4 else kf["ids"][i] for i in range(n)]
        kf["flags"] = [int(f) & 2 if rng.random() < 0.2 else int(f) | 1 for f in kf["flags"]]
        a = ci.device_arrays(kf)
        store.update_points(k, a["flags"], a["points"], a["ids"], a["point_desc"], a["min_dist"], a["max_dist"])

    insert(0, 8, False)
    update(list(range(8)), False)
    insert(8, 20, True)
    update([19, 8, 9, 9, 3, 15, 8, 12, 19], True)
    update(list(range(20)), True)
    for k in (4, 9, 10):
        points(k)
    update([9, 4, 10, 11, 4, 8, 2], False)
    insert(20, 31, False)
    insert(31, 40, True)
    update([int(x) for x in rng.permutation(40)] + [5, 5, 30], True)
    points(33)
    update([33, 32, 34, 35, 33, 31], False)
    update(list(range(39, -1, -1)), False)
    W = np.array([store.connections(k)["weights"] for k in range(40)])
    lens = [len(store.connections(k)["ordered"]) for k in range(40)]
    assert (W != W.T).any() and (W >= 15).any() and ((W > 0) & (W < 15)).any() and max(lens) >= 2   # the script exercises all of it
    assert store.connections_status() == 0


def test_wide_store_one_call_lists_all(vo):
    """300 key-frames x 16 features: more key-frames than threads of a workgroup, 8192 index keys (four sort chunks)"""
    import torch
    rng = np.random.default_rng(12)
    kfs = ci.sliding_window_store(rng, 300, 16, 18, 0, 4, p_dup=0.08, p_clear=0.05)
    store = _enabled_store(vo, kfs, 16)
    lst = torch.arange(300, dtype=torch.int32).cuda()
    store.update_connections(lst)
    model = Connections()
    model.update_list(kfs, list(range(300)))
    _assert_equal(store, model)
    assert max(len(model.ordered[k]) for k in range(300)) >= 4 and any(len(model.children[k]) >= 2 for k in range(300))
    assert store.connections_status() == 0


def test_more_children_than_the_graph_row_holds(vo):
    """66 key-frames; 1 .. 65 each share one id with key-frame 0 alone, so every first connection chooses key-frame 0"""
    b = ci._Builder(66)
    b.store[0] = dict(ids=[], flags=[])
    for k in range(1, 66):
        ids = b.fresh(1)
        b.store[0]["ids"] += ids
        b.store[0]["flags"] += [1]
        b.store[k]["ids"] += ids
        b.store[k]["flags"] += [1]
    store = _enabled_store(vo, b.store, 80)
    lst = list(range(65, 0, -1))
    store.update_connections(lst)
    assert [store.connections(k)["parent"] for k in range(1, 66)] == [0] * 65
    assert store.connections(0)["children"] == list(range(1, 65))
    model = Connections()
    model.update_list(b.store, lst)
    _assert_equal(store, model)
    assert store.connections_status() == vo.KeyFrameStore.CONNECTIONS_CAPACITY
    assert store.connections_status() == 0


def test_a_number_outside_the_store(vo):
    import torch
    case = ci.hand_cases()[2]
    lst = [0, 99, 1, -3, 2]
    store = _enabled_store(vo, case["store"], ci.NK_HAND)
    with pytest.raises(vo.VoError, match="status -1"):
        store.update_connections(lst)
    fresh = Connections()
    fresh.grow(ci.K_HAND)
    _assert_equal(store, fresh)   # the host form changed nothing
    assert store.connections_status() == 0
    d = torch.tensor(lst, dtype=torch.int32).cuda()
    store.update_connections(d)
    model = Connections()
    model.update_list(case["store"], [0, 1, 2])
    _assert_equal(store, model)
    assert store.connections_status() == vo.KeyFrameStore.CONNECTIONS_INVALID
    assert store.connections_status() == 0


def test_one_writer_of_the_graph(vo):
    case = ci.hand_cases()[0]
    plain = vo.KeyFrameStore(4, ci.NK_HAND)
    plain.insert(ci.device_arrays(case["store"][0]))
    with pytest.raises(vo.VoError, match="status -1"):
        plain.enable_connections()
    with pytest.raises(vo.VoError, match="status -1"):
        plain.update_connections([0])
    plain.set_graph(0, [], [], -1)   # still the caller's
    store = _enabled_store(vo, case["store"], ci.NK_HAND)
    with pytest.raises(vo.VoError, match="status -1"):
        store.set_graph(0, [1], [], -1)
    with pytest.raises(vo.VoError, match="status -1"):
        store.set_graph_batch(0, [[1]], [[]], [-1])
    big = vo.KeyFrameStore(4097, 1)
    with pytest.raises(vo.VoError, match="status -4"):
        big.enable_connections()


def test_build_local_map_reads_the_device_graph(vo, ctx):
    """store A: the graph maintained on the device; store B: the model's graph uploaded with set_graph_batch.  Relocalise and
    build the local map on each: every local-map array is byte-identical (and equals tests/local_map_ref.py on the graph)"""
    rng = np.random.default_rng(13)
    max_local = 1500
    trk_a, keep_a, slots, status = lm._relocalized(vo, ctx, max_local)
    trk_b, keep_b, _, _ = lm._relocalized(vo, ctx, max_local)
    K = 24
    kfs = lm._synthetic(rng, K, 50, 64, lm._pool(slots, rng, 60), p_bad=0.1)
    held = lm._model(kfs)
    lst = list(range(K)) + [int(x) for x in rng.integers(0, K, 12)]
    model = Connections()
    model.update_list(held, lst)
    for k in range(K):
        nb, ch, parent = model.graph(k)
        kfs[k].update(neighbors=nb, children=ch, parent=parent)
    assert max(len(kf["neighbors"]) for kf in kfs) >= 3 and any(kf["children"] for kf in kfs)
    a = vo.KeyFrameStore(K, 64)
    a.enable_connections()
    for kf in kfs:
        a.insert(dict(ci.device_arrays(kf), points=kf["points"], point_desc=kf["point_desc"], min_dist=kf["min_dist"], max_dist=kf["max_dist"],
                      bad=kf["bad"]))
    for i, kf in enumerate(kfs):
        a.set_normals(i, kf["normals"])
    a.update_connections(lst)
    _assert_equal(a, model)
    b = lm._device_store(vo, kfs, 64)
    keys = lm.ARRAYS + ("LOCAL_KEYFRAMES", "LOCAL_N_KEYFRAMES", "LOCAL_N_POINTS", "LOCAL_REF_KF")
    got = []
    for trk, store in ((trk_a, a), (trk_b, b)):
        trk.build_local_map(store)
        trk.results()
        got.append({key: trk.get(getattr(trk, key)) for key in keys})
    for key in keys:
        assert got[0][key].tobytes() == got[1][key].tobytes(), key
    _, want = lm._compare(trk_a, kfs, slots, status & 4, max_local)
    assert sum(w["n_keyframes"] for w in want) > 0 and sum(w["n_points"] for w in want) > 0
    trk_a.close()
    trk_b.close()
