"""vo_kfstore_cull_keyframes / vo_kfstore_erase_keyframe (LocalMapping::cullingKeyFrames and KeyFrame::eraseKeyFrame on the
device, localMapping.cpp:434-494, keyframe.cpp:400-526) against the model tests/cull_ref.py.  Every comparison is exact: the
state is integers and bytes."""
import ctypes as C

import numpy as np
import pytest

import connections_inputs as ci
import cull_inputs as qi
import test_gpu_local_map as lm

pytestmark = pytest.mark.gpu

ctx = lm.ctx   # (its module fixture: the relocalisation inputs of the end-to-end test)


class DeviceRunner:
    """the steps of a script of tests/cull_inputs.py on a store, under the names cull_inputs.snapshot uses.  dev: every
    other key-frame goes in through insert_dev, and every key-frame's columns through set_keypoints_dev"""

    def __init__(self, vo, max_keyframes, max_features, dev=False, arrays=None):
        self.s = vo.KeyFrameStore(max_keyframes, max_features)
        self.s.enable_connections()
        self.s.enable_culling()
        self.dev, self.keep, self.n, self.arrays = dev, [], [], arrays

    def step(self, s):
        import torch
        st = self.s
        if s[0] == "insert":
            k = len(st)
            a = self.arrays(k, s) if self.arrays else ci.device_arrays(dict(ids=s[1], flags=s[2]))
            cols = (np.asarray(s[3], np.int32), np.asarray(s[4], np.float32), np.asarray(s[5], np.float32))
            if self.dev and k % 2:
                a = {key: torch.from_numpy(np.ascontiguousarray(v)).cuda() for key, v in a.items()}
                self.keep.append(a)
                st.insert_dev(a)
            else:
                st.insert(a)
            if self.dev:
                cols = tuple(torch.from_numpy(c).cuda() for c in cols)
                self.keep.append(cols)
            st.set_keypoints(k, *cols)
            self.n.append(len(s[1]))
        elif s[0] == "update":
            if self.dev:
                self.keep.append(torch.tensor(s[1], dtype=torch.int32).cuda())
                st.update_connections(self.keep[-1])
            else:
                st.update_connections(s[1])
        elif s[0] == "points":
            a = ci.device_arrays(dict(ids=s[2], flags=s[3]))
            st.update_points(s[1], a["flags"], a["points"], a["ids"], a["point_desc"], a["min_dist"], a["max_dist"])
        elif s[0] == "bad":
            st.set_bad(s[1])
        elif s[0] == "lock":
            st.set_erase_lock(s[1], s[2])
        elif s[0] == "cull":
            st.cull_keyframes(s[1], s[2])
        elif s[0] == "erase":
            st.erase_keyframe(s[1])
        else:
            raise ValueError(s[0])
        return s[0] in ("cull", "erase")

    def __len__(self):
        return len(self.s)

    def cull_result(self):
        return self.s.cull_result()

    def cull_state(self, k):
        return self.s.cull_state(k)

    def connections(self, k):
        return self.s.connections(k)

    def flags_of(self, k):
        return self.s.flags(k, self.n[k])


def _run_both(device, script):
    """the script on the device store and on the model, compared behind every cull and erase step -> (model, snapshots)"""
    model = qi.ModelRunner()
    snaps = []
    for s in script:
        model.step(s)
        if device.step(s):
            got, want = qi.snapshot(device, len(device)), qi.snapshot(model, len(model))
            for key in ("result", "state", "flags", "connections"):
                assert got[key] == want[key], (s[:2], key)
            snaps.append(got)
    return model.m, snaps


@pytest.mark.parametrize("case", qi.hand_cases(), ids=lambda c: c["name"])
def test_hand_made_case(vo, case):
    K = sum(1 for s in case["script"] if s[0] == "insert")
    dev = DeviceRunner(vo, K, qi.NK_HAND)
    _, snaps = _run_both(dev, case["script"])
    assert case["check"](snaps)
    assert dev.s.connections_status() == 0


@pytest.fixture(scope="module")
def sequence():
    return qi.random_script(qi.SEED)


@pytest.mark.parametrize("dev", [False, True], ids=["host_forms", "dev_forms"])
def test_random_interleaved_sequence(vo, sequence, dev):
    """12 key-frames of 48-64 features over a pool of 80 ids: insert / set_keypoints / update_connections / cull_keyframes
    interleaved, a lock, a set_bad and explicit erases; everything compared behind every cull and erase call.  The host and
    the device forms of insert, set_keypoints and update_connections give the same state: both equal the model's"""
    runner = DeviceRunner(vo, 12, 64, dev=dev)
    m, snaps = _run_both(runner, sequence)
    qi.assert_not_vacuous(m)
    # (the sequence lists erased key-frames for update_connections: skipped, and the sticky word says so)
    assert len(snaps) >= 10 and m.log["skipped_updates"] > 0
    assert runner.s.connections_status() == vo.KeyFrameStore.CONNECTIONS_INVALID and runner.s.connections_status() == 0


def _wide_script():
    """4 key-frames of 1030 features (more than the 1024 threads of k_cull_apply, more than the 256 of k_cull_count): 1000
    ids all four hold, 30 that 1 and 2 hold alone and 30 of their own for 0 and 3, features shuffled.  Key-frame 3 culls: 2 is
    redundant (about 970 of 1030) and goes, its 30 shared points die, and 1 is counted again inside k_cull_apply"""
    rng = np.random.default_rng(5)
    level = rng.integers(0, 7, 3000)
    script = []
    for k in range(4):
        ids = np.concatenate([np.arange(1000), {0: 2100, 1: 2000, 2: 2000, 3: 2200}[k] + np.arange(30)])
        ids = ids[rng.permutation(len(ids))]
        n = len(ids)
        depth = np.where(rng.random(n) < 0.05, -1.0, rng.uniform(0.5, qi.TH, n)).astype(np.float32)
        flags = np.where(rng.random(n) < 0.01, 2, 1)
        script.append(("insert", [int(x) for x in ids], [int(x) for x in flags], [int(x) for x in level[ids]], [float(x) for x in depth],
                       [-1.0] * n))
        script.append(("update", [k]))
    return script + [("cull", 3, qi.TH)]


def test_more_features_than_threads(vo):
    dev = DeviceRunner(vo, 4, 1100)
    m, snaps = _run_both(dev, _wide_script())
    r = {x[0]: x for x in snaps[0]["result"]}
    order = [x[0] for x in snaps[0]["result"]]
    assert {k: x[3] for k, x in r.items()} == {2: 1, 1: 0, 0: 3} and order.index(2) < order.index(1)
    assert r[2][1] > 900 and m.log["dead_points"] >= 25
    first = qi.run_model(_wide_script()[:-1])[0].count(1, qi.TH)    # key-frame 1 against the state the call started with
    assert first[0] - r[1][1] >= 25 and first[1] > r[1][2] == 0   # the recount saw the dead points and the missing observer


def test_a_store_without_culling(vo):
    """every new entry point is VO_ERR_INVALID without enable_culling, enable_culling needs an empty store with connections,
    and the existing calls give the same bytes on a store with culling enabled and one without"""
    L = vo.lib()
    script = [s for s in qi.random_script(qi.SEED) if s[0] in ("insert", "update")]
    plain = vo.KeyFrameStore(12, 64)
    with pytest.raises(vo.VoError, match="status -1"):
        plain.enable_culling()                      # no connections
    plain.enable_connections()
    with_culling = DeviceRunner(vo, 12, 64)
    for s in script:
        with_culling.step(s)
        if s[0] == "insert":
            plain.insert(ci.device_arrays(dict(ids=s[1], flags=s[2])))
        else:
            plain.update_connections(s[1])
    h, w, z = plain._h, C.c_int32(0), np.zeros(64, np.int32)
    zf = z.view(np.float32)
    assert L.vo_kfstore_enable_culling(h) == -1     # not empty
    assert L.vo_kfstore_set_keypoints(h, 0, vo._p(z), vo._p(zf), vo._p(zf)) == -1
    assert L.vo_kfstore_set_keypoints_dev(h, 0, vo._p(z), vo._p(zf), vo._p(zf)) == -1
    assert L.vo_kfstore_set_erase_lock(h, 1, 1) == -1
    assert L.vo_kfstore_cull_keyframes(h, 11, C.c_float(qi.TH)) == -1
    assert L.vo_kfstore_erase_keyframe(h, 1) == -1
    assert L.vo_kfstore_cull_result(h, C.byref(w), None, None, None, None) == -1
    assert L.vo_kfstore_cull_state(h, 1, None, None, None) == -1
    for k in range(12):
        assert plain.connections(k) == with_culling.s.connections(k), k
        assert plain.flags(k) == with_culling.s.flags(k), k
    assert plain.connections_status() == 0 and with_culling.s.connections_status() == 0
    # the numbers are validated on a store with culling
    s = with_culling.s
    for call in (lambda: s.set_keypoints(12, z, zf, zf), lambda: s.set_erase_lock(-1), lambda: s.cull_keyframes(12, qi.TH),
                 lambda: s.erase_keyframe(99), lambda: s.cull_state(12)):
        with pytest.raises(vo.VoError, match="status -1"):
            call()


def test_build_local_map_after_the_culls(vo, ctx, sequence):
    """store A: the random sequence on the device.  Store B: no connections, the MODEL's final state put in through insert,
    set_bad and set_graph_batch, the erased key-frames bad and their features unflagged.  Relocalise and build the local map
    on each: every local-map array is byte-identical"""
    rng = np.random.default_rng(21)
    max_local = 1500
    trk_a, _, slots, status = lm._relocalized(vo, ctx, max_local)
    trk_b, _, _, _ = lm._relocalized(vo, ctx, max_local)
    live = np.unique(slots[slots >= 0])
    idmap = np.concatenate([rng.permutation(live)[:80], 10 ** 6 + np.arange(80)])[:80]   # the sequence's ids in the frames' id space
    script = [(s[0], [int(idmap[p]) for p in s[1]]) + tuple(s[2:]) if s[0] == "insert" else s for s in sequence]
    side = {}

    def arrays(k, s):
        side[k] = dict(ci.device_arrays(dict(ids=s[1], flags=s[2]), rng), point_desc=rng.integers(0, 256, (len(s[1]), 32), dtype=np.uint8),
                       normals=rng.normal(0, 1, (len(s[1]), 3)))
        return {key: v for key, v in side[k].items() if key != "normals"}

    a = DeviceRunner(vo, 12, 64, arrays=arrays)
    m, _ = _run_both(a, script)
    qi.assert_not_vacuous(m)
    K = len(m.store)
    for k in range(K):
        a.s.set_normals(k, side[k]["normals"])
    b = vo.KeyFrameStore(K, 64)
    for k in range(K):
        flags = np.zeros(len(m.store[k]["ids"]), np.uint8) if m.erased[k] else np.asarray(m.store[k]["flags"], np.uint8)
        b.insert(dict({key: v for key, v in side[k].items() if key != "normals"}, flags=flags, bad=m.store[k]["bad"]))
        b.set_normals(k, side[k]["normals"])
    graphs = [m.conn.graph(k) for k in range(K)]
    b.set_graph_batch(0, [g[0] for g in graphs], [g[1] for g in graphs], [g[2] for g in graphs])
    keys = lm.ARRAYS + ("LOCAL_KEYFRAMES", "LOCAL_N_KEYFRAMES", "LOCAL_N_POINTS", "LOCAL_REF_KF")
    got = []
    for trk, store in ((trk_a, a.s), (trk_b, b)):
        trk.build_local_map(store)
        trk.results()
        got.append({key: trk.get(getattr(trk, key)) for key in keys})
    for key in keys:
        assert got[0][key].tobytes() == got[1][key].tobytes(), key
    assert got[0]["LOCAL_N_KEYFRAMES"].sum() > 0 and got[0]["LOCAL_N_POINTS"].sum() > 0
    assert not any(k in got[0]["LOCAL_KEYFRAMES"] for k in range(K) if m.erased[k]) and any(m.erased)
    trk_a.close()
    trk_b.close()
