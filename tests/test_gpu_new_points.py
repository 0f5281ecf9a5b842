"""vo_kfstore_create_map_points (LocalMapping::createNewMapPoints on the device, localMapping.cpp:132-361) against the model
tests/new_points_ref.py, through the binding.  Exact: the result record (statuses, match counts, created rows in order),
every flags byte and id, point_desc, the id counter, the connection state.  To the tolerance include/vo_hip.h states for
vo_triangulate (TAU): positions (relative), normals (absolute), min / max distance (relative).  The inputs contain no match
whose gates could fall either way within those tolerances (tests/test_new_points_ref.py)."""
import ctypes as C
import pathlib

import numpy as np
import pytest

import new_points_inputs as ni
import test_gpu_local_map as lm
from new_points_ref import TAU

pytestmark = pytest.mark.gpu

ctx = lm.ctx   # (its module fixture: the relocalisation inputs of the end-to-end test)


class DeviceRunner:
    """the steps of a script of tests/new_points_inputs.py on a store, under the names new_points_inputs.snapshot uses.  dev:
    every other key-frame goes in through insert_dev, and every key-frame's columns, pose and key-point positions through
    the device forms of their setters"""

    def __init__(self, vo, max_keyframes, max_features, dev=False, first_point_id=ni.FIRST_ID):
        self.s = vo.KeyFrameStore(max_keyframes, max_features)
        self.s.enable_connections()
        self.s.enable_culling()
        self.s.enable_mapping(ni.CAM6, ni.SF, first_point_id)
        self.dev, self.keep, self.n = dev, [], []

    def step(self, s):
        import torch
        st = self.s
        cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        if s[0] == "insert":
            k = len(st)
            a = ni.insert_arrays(s)
            cols = (np.asarray(s[3], np.int32), np.asarray(s[4], np.float32), np.asarray(s[5], np.float32))
            if self.dev and k % 2:
                a = {key: cuda(v) for key, v in a.items()}
                self.keep.append(a)
                st.insert_dev(a)
            else:
                st.insert(a)
            if self.dev:
                cols = tuple(cuda(c) for c in cols)
                self.keep.append(cols)
            st.set_keypoints(k, *cols)
            self.n.append(len(s[1]))
        elif s[0] == "update":
            if self.dev:
                self.keep.append(torch.tensor(s[1], dtype=torch.int32).cuda())
                st.update_connections(self.keep[-1])
            else:
                st.update_connections(s[1])
        elif s[0] == "bad":
            st.set_bad(s[1])
        elif s[0] == "erase":
            st.erase_keyframe(s[1])
        elif s[0] == "pose":
            T = np.asarray(s[2], np.float64)
            if self.dev:
                self.keep.append(cuda(T))
                T = self.keep[-1]
            st.set_pose(s[1], T)
        elif s[0] == "xy":
            xy = np.asarray(s[2], np.float32)
            if self.dev:
                self.keep.append(cuda(xy))
                xy = self.keep[-1]
            st.set_keypoint_xy(s[1], xy)
        elif s[0] == "create":
            st.create_map_points(s[1], s[2])
        else:
            raise ValueError(s[0])
        return s[0] == "create"

    def __len__(self):
        return len(self.s)

    def new_points_result(self):
        return self.s.new_points_result()

    def next_point_id(self):
        return self.s.next_point_id()

    def connections(self, k):
        return self.s.connections(k)

    def points_of(self, k):
        return self.s.points(k, self.n[k])


def _assert_same(got, want, where):
    assert got["result"] == want["result"], where
    assert got["next_id"] == want["next_id"], where
    assert got["connections"] == want["connections"], where
    for k, (g, w) in enumerate(zip(got["points"], want["points"])):
        for key in ("flags", "ids", "point_desc"):
            assert np.array_equal(g[key], w[key]), (where, k, key)
        new = w["ids"] >= 0   # (the map side of a feature without a point is filler on both sides: compared where a point is)
        scale = np.maximum(np.linalg.norm(w["points"][new], axis=1, keepdims=True), 1e-30)
        assert (np.abs(g["points"][new] - w["points"][new]) <= TAU * scale).all(), (where, k, "points")
        assert (np.abs(g["normals"][new] - w["normals"][new]) <= TAU).all(), (where, k, "normals")
        for key in ("min_dist", "max_dist"):
            assert (np.abs(g[key][new] - w[key][new]) <= TAU * np.abs(w[key][new])).all(), (where, k, key)


def _run_both(device, script, first_point_id=ni.FIRST_ID):
    """the script on the device store and on the model, compared behind every create step -> (model, the device's snapshots)"""
    model = ni.ModelRunner(first_point_id)
    snaps = []
    for i, s in enumerate(script):
        model.step(s)
        if device.step(s):
            got, want = ni.snapshot(device, len(device)), ni.snapshot(model, len(model))
            _assert_same(got, want, (i, s[:2]))
            snaps.append(got)
    return model.m, snaps


@pytest.mark.parametrize("case", ni.hand_cases(), ids=lambda c: c["name"])
def test_hand_made_case(vo, case):
    """cases a .. h of the issue (e without |x3| < 1e-8: see test_degenerate_triangulation_is_flagged)"""
    K = sum(1 for s in case["script"] if s[0] == "insert")
    dev = DeviceRunner(vo, K, ni.NK_HAND)
    _, snaps = _run_both(dev, case["script"])
    assert case["check"](snaps)
    assert dev.s.connections_status() == case.get("sticky", 0)


def test_case_a_differs_from_independent_searches(vo):
    """the ten searches of vo_match_triangulation_batch are independent: against the flags the call starts with, neighbour 1
    gives (c0, b0) and leaves c1 alone.  The store-side call gives b0 to c1, because c0 got its point from neighbour 0"""
    case = [c for c in ni.hand_cases() if c["name"].startswith("a_")][0]
    m, _ = ni.run_model(case["script"][:-1])
    from new_points_ref import geometry
    views = [m._view(k) for k in range(3)]
    fa = lambda v: vo.FrameArrays(v["x"], v["y"], v["octave"], v["angle"], v["u_right"], v["desc"])
    has = [np.array([f & 1 for f in m.store[k]["flags"]], np.uint8) for k in range(3)]
    pairs = []
    for k in (0, 1):
        G = geometry(m.store[2]["pose"], m.store[k]["pose"], m.cam)
        pairs.append((fa(views[k]), has[k], vo.BowNodes(views[k]["nodes"]), np.array(G["F"]).reshape(3, 3), float(G["ex"]), float(G["ey"])))
    sf = np.array(ni.SF, np.float32)
    counts, match = vo.Matcher(0.6).searchForTriangulation_batch(fa(views[2]), has[2], vo.BowNodes(views[2]["nodes"]), pairs, sf, True)
    a = case["a"]
    dev = DeviceRunner(vo, 3, ni.NK_HAND)
    _, snaps = _run_both(dev, case["script"])
    created = [(k, i1, i2) for k, i1, i2, _ in snaps[0]["result"]["created"]]
    assert (int(match[1][a["c0"]]), int(match[1][a["c1"]]), created[1]) == (a["b0"], -1, (1, a["c1"], a["b0"]))


@pytest.fixture(scope="module")
def scene():
    return ni.random_scene(ni.SEED)


@pytest.mark.parametrize("dev", [False, True], ids=["host_forms", "dev_forms"])
def test_seeded_random_scene(vo, scene, dev):
    """12 key-frames of 256 features, stereo and mono mixed; create for the last three key-frames in turn with an update
    between them; everything compared behind every create call, and the weights of the updates count the new points"""
    runner = DeviceRunner(vo, 12, 256, dev=dev)
    m, snaps = _run_both(runner, scene)
    ni.assert_not_vacuous(m)
    assert len(snaps) == 3 and sum(len(s["result"]["created"]) for s in snaps) >= 150
    assert runner.s.connections_status() == 0
    # behind the last update: the index rebuild has seen the commit
    assert [runner.s.connections(k) for k in range(12)] == [m.connections(k) for k in range(12)]
    first = ni.run_model([s for s in scene if s[0] != "create"])[0]
    assert m.connections(11)["weights"] != first.connections(11)["weights"]


def test_misuse(vo):
    L = vo.lib()
    cam, sf = np.array(ni.CAM6, np.float32), np.array(ni.SF, np.float32)
    z = np.zeros(64, np.float64)
    plain = vo.KeyFrameStore(4, 64)
    plain.enable_connections()
    assert L.vo_kfstore_enable_mapping(plain._h, vo._p(cam), 8, vo._p(sf), 0) == -1        # no culling
    plain.enable_culling()
    h, w = plain._h, C.c_int32(0)
    for rc in (L.vo_kfstore_set_pose(h, 0, vo._p(z)), L.vo_kfstore_set_pose_dev(h, 0, vo._p(z)), L.vo_kfstore_set_keypoint_xy(h, 0, vo._p(z)),
               L.vo_kfstore_set_keypoint_xy_dev(h, 0, vo._p(z)), L.vo_kfstore_next_point_id(h, C.byref(w)),
               L.vo_kfstore_create_map_points(h, 0, 10), L.vo_kfstore_new_points_result(h, C.byref(w), None, None, None, None, None, 0)):
        assert rc == -1                                                                       # no enable_mapping
    assert L.vo_kfstore_enable_mapping(h, vo._p(cam), 17, vo._p(sf), 0) == -1 and L.vo_kfstore_enable_mapping(h, vo._p(cam), 8, vo._p(sf), -1) == -1
    # numbers out of range, on a store with one key-frame without neighbours
    case = ni.hand_cases()[0]
    dev = DeviceRunner(vo, 3, ni.NK_HAND)
    dev.step(case["script"][0])
    assert L.vo_kfstore_enable_mapping(dev.s._h, vo._p(cam), 8, vo._p(sf), 0) == -1         # not empty
    for call in (lambda: dev.s.create_map_points(1, 10), lambda: dev.s.create_map_points(-1, 10), lambda: dev.s.create_map_points(0, 0),
                 lambda: dev.s.create_map_points(0, 11), lambda: dev.s.set_pose(1, z[:12]), lambda: dev.s.set_keypoint_xy(3, z[:2])):
        with pytest.raises(vo.VoError, match="status -1"):
            call()
    import torch
    for call in (lambda: dev.s.set_pose(0, torch.zeros(12, dtype=torch.float32).cuda()), lambda: dev.s.set_pose(0, torch.zeros(9, dtype=torch.float64).cuda()),
                 lambda: dev.s.set_keypoint_xy(0, torch.zeros((ni.NK_HAND, 2), dtype=torch.float64).cuda())):
        with pytest.raises(vo.VoError, match="tensor"):   # a device tensor of another element type or length is refused by the binding
            call()
    dev.s.set_pose(0, case["script"][1][2])
    dev.s.create_map_points(0, 10)                                                            # no neighbours: an empty record
    assert dev.s.new_points_result() == dict(neighbors=[], created=[]) and dev.s.connections_status() == 0
    assert dev.s.next_point_id() == ni.FIRST_ID


def test_erased_current_creates_nothing(vo):
    """case g's store with the current key-frame erased: the sticky bit, an empty record, not a byte written"""
    case = [c for c in ni.hand_cases() if c["name"].startswith("g_")][0]
    dev = DeviceRunner(vo, 3, ni.NK_HAND)
    script = [s for s in case["script"] if s[0] != "create"]
    for s in script:
        dev.step(s)
    dev.s.erase_keyframe(2)
    before = [dev.points_of(k) for k in range(3)]
    dev.s.create_map_points(2, 10)
    after = [dev.points_of(k) for k in range(3)]
    assert dev.s.new_points_result() == dict(neighbors=[], created=[]) and dev.s.next_point_id() == ni.FIRST_ID
    assert all(b[key].tobytes() == a[key].tobytes() for b, a in zip(before, after) for key in b)
    assert dev.s.connections_status() == vo.KeyFrameStore.CONNECTIONS_INVALID


def test_vo_triangulate_is_bit_identical_after_the_header_move(vo):
    """vo_triangulate on tests/test_gpu_loop.py's inputs against the bytes recorded before its arithmetic moved into
    csrc/triangulate.h (tests/golden/new_points_triangulate.npz)"""
    g = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "new_points_triangulate.npz")
    xn1, xn2, T1, T2s = ni.triangulation_inputs()
    pts, ok = vo.triangulate(xn1, xn2, T1, T2s)
    one, ok1 = vo.triangulate(xn1[:4], xn2[:4], T1, T2s[0])
    assert pts.tobytes() == g["points"].tobytes() and ok.tobytes() == g["ok"].tobytes()
    assert one.tobytes() == g["one"].tobytes() and ok1.tobytes() == g["ok1"].tobytes()


def test_degenerate_triangulation_is_flagged(vo):
    """|x3| < 1e-8 (:245-246).  With identical rays cosParallaxRay is 1, which no cosParallaxDepth exceeds by more than the
    four ulps a decisive match needs, so no decisive input reaches the check through create_map_points; the shared
    arithmetic is exercised directly: identical poses up to an offset along the common ray leave a null vector without a
    finite point"""
    T1 = np.eye(3, 4, dtype=np.float32)
    T2 = T1.copy()
    T2[2, 3] = -0.5
    pts, ok = vo.triangulate(np.zeros((1, 2), np.float32), np.zeros((1, 2), np.float32), T1, T2)
    assert (int(ok[0]), pts[0].tolist()) == (0, [0.0, 0.0, 0.0])


def test_build_local_map_lists_the_new_points(vo, ctx):
    """store A: the random scene on the device, its old ids mapped into the id space of relocalised frames.  Store B: a plain
    store holding what A holds afterwards (read back), its graph set from A's connections.  The local map built from either
    is byte-identical, and it lists points the create calls made"""
    c = ctx
    rng = np.random.default_rng(21)
    max_local, first = 4000, 2_000_000
    trk_a, _, slots, _ = lm._relocalized(vo, c, max_local)
    trk_b, _, _, _ = lm._relocalized(vo, c, max_local)
    live = rng.permutation(np.unique(slots[slots >= 0]))
    script = [(s[0], [int(live[p % len(live)]) if p >= 0 else -1 for p in s[1]]) + tuple(s[2:]) if s[0] == "insert" else s
              for s in ni.random_scene(ni.SEED)]
    a = DeviceRunner(vo, 12, 256, first_point_id=first)
    m, snaps = _run_both(a, script, first)
    assert sum(len(s["result"]["created"]) for s in snaps) >= 150
    b = vo.KeyFrameStore(12, 256)
    held = [a.points_of(k) for k in range(12)]
    for k, s in enumerate(s for s in script if s[0] == "insert"):
        arr = ni.insert_arrays(s)
        b.insert(dict(arr, flags=held[k]["flags"], ids=held[k]["ids"], points=held[k]["points"], point_desc=held[k]["point_desc"],
                      min_dist=held[k]["min_dist"], max_dist=held[k]["max_dist"]))
        b.set_normals(k, held[k]["normals"])
    graphs = [m.conn.graph(k) for k in range(12)]
    b.set_graph_batch(0, [g[0] for g in graphs], [g[1] for g in graphs], [g[2] for g in graphs])
    keys = lm.ARRAYS + ("LOCAL_KEYFRAMES", "LOCAL_N_KEYFRAMES", "LOCAL_N_POINTS", "LOCAL_REF_KF")
    got = []
    for trk, store in ((trk_a, a.s), (trk_b, b)):
        trk.build_local_map(store)
        trk.results()
        got.append({key: trk.get(getattr(trk, key)) for key in keys})
    for key in keys:
        assert got[0][key].tobytes() == got[1][key].tobytes(), key
    assert got[0]["LOCAL_N_KEYFRAMES"].sum() > 0 and (got[0]["LOCAL_POINT_IDS"] >= first).sum() >= 50
    trk_a.close()
    trk_b.close()
