"""Key-frame creation on the device against the model tests/keyframe_create_ref.py, through the binding:
vo_kfstore_create_keyframe (host, device and frames forms), keyframe_result and keyframe_need_stats.  Compared byte for byte: every flags
byte, id, point row, point_desc, normal, min / max distance, ref_kf, the pose, the id counter, the record, the created lists
and the sticky word -- after every NaN has been made THE positive quiet NaN on both sides (IEEE leaves a generated NaN's sign
open; the device and the host's numpy choose differently).  The feature side -- angle, desc, octave / depth / u_right,
xy and the FeatureVector CSR, read through vo_kfstore_get_features -- is compared byte for byte too, for every key-frame of every
form and shape; the model's node ids come from a numpy restatement of the vocabulary descent (keyframe_create_inputs.node_of)."""
import pathlib

import numpy as np
import pytest

import keyframe_create_inputs as ki
import point_upkeep_inputs as ui
from keyframe_create_ref import RECORD, KeyframeCreateModel, canonical

from test_gpu_local_ba_store import _exp, _log
from test_gpu_point_upkeep import UDev

pytestmark = pytest.mark.gpu
f32 = np.float32
VD = ki.vocabulary()
FEATURE_SIDE = ("angle", "desc", "octave", "depth", "u_right", "xy")
COLUMNS = ("Tcw12", "x", "y", "octave", "angle", "depth", "u_right", "desc", "slot_ids")


@pytest.fixture(scope="module")
def voc(vo):
    vd = VD
    return vo.Vocabulary(vd["L"], vd["child_start"], vd["children"], vd["node_desc"], vd["node_weight"], vd["word_id"])


class KDev(UDev):
    """test_gpu_point_upkeep.UDev on a store with every layer up to the upkeep and, with `layer`, key-frame creation"""

    def __init__(self, vo, K, NK, dev=False, layer=True, stream=None, first_point_id=ki.FIRST_ID):
        s = vo.KeyFrameStore(K, NK, stream=stream)
        s.enable_connections(), s.enable_culling(), s.enable_mapping(ki.CAM6, ki.SF, first_point_id)
        s.enable_local_ba(*ki.CAPS), s.enable_point_upkeep(ki.MAX_RECENT)
        if layer:
            s.enable_keyframe_create()
        self.s, self.dev, self.local_ba, self.keep, self.n = s, dev, True, [], []

    def create(self, voc, f, th, initial=False):
        if self.dev:
            import torch
            f = {k: torch.from_numpy(np.ascontiguousarray(f[k])).cuda() for k in COLUMNS if k in f}
            self.keep.append(f)
        k = self.s.create_keyframe(voc, f, float(th), initial)
        self.n.append(len(f["depth"]))
        return k


def _model(vo, script=()):
    r = ui.ModelRunner.__new__(ui.ModelRunner)
    r.m = KeyframeCreateModel(ki.CAM6, ki.SF, ki.FIRST_ID, ki.CAPS, _exp(vo), _log(vo), ki.MAX_RECENT)
    create = r.m.create_keyframe      # the model's FeatureVector: the node of every descriptor by the numpy descent
    r.m.create_keyframe = lambda f, th, initial=False, nodes=None: create(f, th, initial, ki.node_of(VD, f["desc"]) if nodes is None else nodes)
    for s in script:
        r.step(s)
    return r


def _pair(vo, K=8, NK=ki.NK, dev=False, script=None):
    """the holder store on the device and in the model"""
    script = ki.holder_store() if script is None else script
    d, mr = KDev(vo, K, NK, dev), _model(vo)
    for s in script:
        d.step(s), mr.step(s)
    return d, mr


def _same_keyframe(d, m, k, where):
    got, want = d.state(k), m.state(k)
    for key in ("flags", "ids", "points", "ref", "normals", "min_dist", "max_dist", "pose", "bad", "point_desc"):
        assert canonical(np.asarray(got[key])).tobytes() == canonical(np.asarray(want[key])).tobytes(), (where, k, key)
    feat = d.s.features(k, d.n[k])
    for key in FEATURE_SIDE:
        assert canonical(feat[key]).tobytes() == canonical(np.asarray(want[key])).tobytes(), (where, k, key)
    assert feat["feature_vector"] == want["feature_vector"], (where, k, "feature_vector")


def _same_call(d, m, k, where, others=()):
    rec = d.s.keyframe_result()
    assert rec == m.keyframe_result() and set(RECORD) <= set(rec), (where, rec, m.keyframe_result())
    assert d.s.next_point_id() == m.next_id and len(d.s) == len(m.store), where
    for j in (k,) + tuple(others):
        _same_keyframe(d, m, j, where)
    assert d.s.connections_status() == m.sticky, where
    m.sticky = 0


TABLES = ki.tables()


@pytest.mark.parametrize("dev", [False, True], ids=["host_form", "dev_form"])
@pytest.mark.parametrize("name", list(TABLES))
def test_tables(vo, voc, name, dev):
    f, want = TABLES[name]
    d, mr = _pair(vo, dev=dev)
    k = d.create(voc, f, ki.TH)
    assert k == mr.m.create_keyframe(f, ki.TH) == 6
    _same_call(d, mr.m, k, name, others=range(6))          # (the earlier key-frames keep their bytes)
    assert d.s.keyframe_result()["n_created"] == want


@pytest.mark.parametrize("dev", [False, True], ids=["host_form", "dev_form"])
def test_initial_key_frame(vo, voc, dev):
    f, want = ki.initial_table()
    d, mr = KDev(vo, 2, ki.NK, dev), _model(vo)
    if dev:
        f = {k: v for k, v in f.items() if k != "slot_ids"}    # ignored, and may be missing
    k = d.create(voc, f, ki.TH, initial=True)
    assert k == mr.m.create_keyframe(f, ki.TH, True) == 0
    _same_call(d, mr.m, k, "initial")
    rec = d.s.keyframe_result()
    assert rec["n_created"] == want and [i for i, _ in rec["created"]] == sorted(i for i, _ in rec["created"])


@pytest.mark.parametrize("n", [0, 1, 255, 256])
def test_feature_counts(vo, voc, n):
    f = ki.random_frame(20 + n, n, ki.HELD + [ki.ERASED_ONLY, ki.NOBODY])
    d, mr = _pair(vo)
    k = d.create(voc, f, ki.TH)
    assert k == mr.m.create_keyframe(f, ki.TH)
    _same_call(d, mr.m, k, n)
    d.s.process_new_keyframe(k), mr.m.process_new_keyframe(k)      # the key-frame is one the next step takes
    _same_keyframe(d, mr.m, k, (n, "processed"))
    assert d.s.upkeep_result() == mr.m.upkeep_result()


@pytest.mark.parametrize("n,NK", [(1500, 2048), (9000, 9100)], ids=["sort_in_lds_two_scan_passes", "sort_in_device_memory"])
def test_large_frames(vo, voc, n, NK):
    """1500 features: the sort is past one power of two and the scan past one workgroup pass; 9000: the keys no longer fit the
    LDS array and are sorted in the layer's block"""
    f = ki.random_frame(n, n, ki.HELD + [ki.NOBODY], p_null=0.6, p_mono=0.1)
    d, mr = _pair(vo, K=7, NK=NK, dev=True)
    k = d.create(voc, f, f32(4.0))
    assert k == mr.m.create_keyframe(f, f32(4.0))
    _same_call(d, mr.m, k, n, others=range(6))
    rec = d.s.keyframe_result()
    assert rec["n_pairs"] > 1024 and rec["ended_early"] == 1 and rec["n_created"] > 101


def _uploaded(vo, f, slot=1, cap=ki.NK):
    """the frame in `slot` of a two-slot vo_frames handle (vo_frames_upload)"""
    fr = vo.Frames(2, cap)
    fa = vo.FrameArrays(f["x"], f["y"], f["octave"], f["angle"], f["u_right"], f["desc"])
    fr.upload(slot, fa, depth=f["depth"])
    return fr, fa


@pytest.mark.parametrize("own_stream", [False, True], ids=["same_stream", "store_on_its_own_stream"])
@pytest.mark.parametrize("name", ["near_101_then_far", "holder_rules", "special_depths"])
def test_frames_form(vo, voc, name, own_stream):
    import torch
    f, want = TABLES[name]
    st = torch.cuda.Stream() if own_stream else None
    d, mr = KDev(vo, 8, ki.NK, stream=st.cuda_stream if st else None), _model(vo)
    for s in ki.holder_store():
        d.step(s), mr.step(s)
    fr, fa = _uploaded(vo, f)
    T, slots = torch.from_numpy(f["Tcw12"]).cuda(), torch.from_numpy(f["slot_ids"]).cuda()
    torch.cuda.synchronize()
    k = d.s.create_keyframe_from_frames(voc, fr, 1, len(f["depth"]), T, slots, float(ki.TH))
    d.n.append(len(f["depth"]))
    assert k == mr.m.create_keyframe(f, ki.TH)
    _same_call(d, mr.m, k, name)
    assert d.s.keyframe_result()["n_created"] == want
    d.s.process_new_keyframe(k), mr.m.process_new_keyframe(k)
    _same_keyframe(d, mr.m, k, (name, "processed"))
    assert [d.s.connections(j) for j in range(k + 1)] == [mr.m.connections(j) for j in range(k + 1)]


def test_frames_form_waits_for_the_frames_producer(vo, voc):
    """the slot is written by vo_frames_build_dev on another stream, behind a tenth of a second of device time that is still
    running when the call returns: only the event makes the store's stream see the frame (without it the call would meet the
    slot's old count and answer status 1).  The model gets the columns the frames hold afterwards"""
    import torch
    n, NK = 200, ki.NK
    rng = np.random.default_rng(9)
    kp = np.zeros((1, NK), vo.KP_DTYPE)
    kp["x"][0, :n], kp["y"][0, :n] = rng.integers(20, 620, n), rng.integers(20, 460, n)
    kp["angle"][0, :n], kp["octave"][0, :n] = rng.uniform(0, 360, n), rng.integers(0, 8, n)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    kps, desc = cuda(kp.view(np.uint8).reshape(1, NK, -1)), cuda(rng.integers(0, 256, (1, NK, 32), dtype=np.uint8))
    counts, depth = cuda(np.array([n], np.int32)), cuda(rng.uniform(0.5, 9.0, (1, 480, 640)).astype(f32))
    slot_ids = np.where(rng.random(n) < 0.5, -1, np.array(ki.HELD)[rng.integers(0, len(ki.HELD), n)]).astype(np.int32)
    Tcw = np.array(ki.frame(rng, [1.0], [-1])["Tcw12"])
    T, slots = cuda(Tcw), cuda(slot_ids)
    fr = vo.Frames(2, NK, intrinsics=[500.0, 500.0, 320.0, 240.0, 40.0])
    S, P = torch.cuda.Stream(), torch.cuda.Stream()
    d, mr = KDev(vo, 8, NK, stream=S.cuda_stream), _model(vo)
    for s in ki.holder_store():
        d.step(s), mr.step(s)
    torch.cuda.synchronize()
    with torch.cuda.stream(P):
        torch.cuda._sleep(200_000_000)
    fr.build_dev(kps, desc, counts, depth=depth, slot0=1, stream=P.cuda_stream)
    k = d.s.create_keyframe_from_frames(voc, fr, 1, n, T, slots, float(ki.TH))
    busy = not P.query()
    torch.cuda.synchronize()
    assert busy
    got = fr.download(1)
    assert got["n"] == n and (got["depth"] > 0).sum() > 100
    f = dict(Tcw12=Tcw, x=got["x"], y=got["y"], octave=got["octave"], angle=got["angle"], depth=got["depth"], u_right=got["uright"],
             desc=got["desc"], slot_ids=slot_ids)
    d.n.append(n)
    assert k == mr.m.create_keyframe(f, ki.TH)
    _same_call(d, mr.m, k, "producer")
    rec = d.s.keyframe_result()
    assert rec["status"] == 0 and rec["n_created"] > 20 and rec["n_tracked"] > 50


def test_frames_form_initial(vo, voc):
    import torch
    f, want = ki.initial_table()
    d, mr = KDev(vo, 2, ki.NK), _model(vo)
    fr, fa = _uploaded(vo, f, slot=0)
    k = d.s.create_keyframe_from_frames(voc, fr, 0, len(f["depth"]), torch.from_numpy(f["Tcw12"]).cuda(), None, float(ki.TH), initial=True)
    d.n.append(len(f["depth"]))
    assert k == mr.m.create_keyframe(f, ki.TH, True) == 0
    _same_call(d, mr.m, k, "initial from frames")
    assert d.s.keyframe_result()["n_created"] == want


def test_frames_form_with_a_wrong_count(vo, voc):
    """n is not the slot's count: the key-frame gets no features, the status and the sticky bit say so, no id is handed out"""
    import torch
    f, _ = TABLES["all_below"]
    d, mr = _pair(vo)
    fr, fa = _uploaded(vo, f)
    n = len(f["depth"]) - 1
    T, slots = torch.from_numpy(f["Tcw12"]).cuda(), torch.from_numpy(f["slot_ids"][:n].copy()).cuda()
    k = d.s.create_keyframe_from_frames(voc, fr, 1, n, T, slots, float(ki.TH))
    rec = d.s.keyframe_result()
    assert (rec["keyframe"], rec["n"], rec["status"], rec["n_created"], rec["n_pairs"], rec["n_tracked"]) == (k, n, 1, 0, 0, 0)
    assert rec["created"] == [] and d.s.next_point_id() == ki.FIRST_ID and len(d.s) == 7
    pts, feat = d.s.points(k, n), d.s.features(k, n)       # the rows the getters span are null slots without a feature
    assert not pts["flags"].any() and (pts["ids"] == -1).all() and (d.s.point_refs(k, n) == -1).all()
    assert not any(pts[key].any() for key in ("points", "point_desc", "min_dist", "max_dist", "normals"))
    assert not any(feat[key].any() for key in ("angle", "desc", "octave", "xy")) and feat["feature_vector"] == []
    assert (feat["depth"] == -1).all() and (feat["u_right"] == -1).all()
    assert d.s.connections_status() == vo.KeyFrameStore.CONNECTIONS_INVALID
    for j in range(6):
        _same_keyframe(d, mr.m, j, "wrong count")          # the earlier key-frames keep their bytes
    d.s.process_new_keyframe(k)                             # a key-frame without features: nothing tracked, nothing listed
    up = d.s.upkeep_result()
    assert (up["n_tracked"], up["n_new"]) == (0, 0) and d.s.connections(k)["n_connected"] == 0
    with pytest.raises(vo.VoError, match="status -1"):
        d.s.create_keyframe_from_frames(voc, fr, 2, n, T, slots, float(ki.TH))       # a slot the handle does not have


def test_same_store_as_insert_dev_and_the_setters(vo, voc):
    """the key-frame put in through the route a caller has without the layer, from arrays the model computed"""
    import torch
    f, _ = TABLES["holder_rules"]
    a, mr = _pair(vo, dev=True)
    b = KDev(vo, 8, ki.NK, dev=True)
    for s in ki.holder_store():
        b.step(s)
    k = a.create(voc, f, ki.TH)
    mr.m.create_keyframe(f, ki.TH)
    st = mr.m.state(k)
    cuda = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()
    arrays = dict(angle=cuda(f["angle"], f32), desc=cuda(f["desc"], np.uint8), nodes=cuda(voc.transform(f["desc"], 3)[2], np.int32),
                  flags=cuda(st["flags"], np.uint8), points=cuda(st["points"], np.float64), ids=cuda(st["ids"], np.int32),
                  point_desc=cuda(st["point_desc"], np.uint8), min_dist=cuda(st["min_dist"], f32), max_dist=cuda(st["max_dist"], f32))
    cols = (cuda(f["octave"], np.int32), cuda(f["depth"], f32), cuda(f["u_right"], f32))
    xy, T, refs = cuda(np.stack([f["x"], f["y"]], 1), f32), cuda(f["Tcw12"], np.float64), cuda(st["ref"], np.int32)
    assert b.s.insert_dev(arrays) == k
    b.s.set_keypoints(k, *cols), b.s.set_keypoint_xy(k, xy), b.s.set_pose(k, T), b.s.set_point_refs(k, refs)
    b.s.set_normals(k, st["normals"])                      # (the existing route's sixth call: normals have a setter of their own)
    b.n.append(len(f["depth"]))

    def same(where):
        for j in range(k + 1):
            ga, gb = a.state(j), b.state(j)
            for key in ga:
                assert np.asarray(ga[key]).tobytes() == np.asarray(gb[key]).tobytes(), (where, j, key)
        assert [a.s.connections(j) for j in range(k + 1)] == [b.s.connections(j) for j in range(k + 1)], where
    same("created")
    a.s.process_new_keyframe(k), b.s.process_new_keyframe(k)       # reads desc, the columns, the poses and the index
    same("processed")
    assert a.s.upkeep_result() == b.s.upkeep_result() and a.s.recent_points() == b.s.recent_points()


def test_refresh_changes_no_byte(vo, voc):
    f, _ = TABLES["near_101_then_far"]
    d, mr = _pair(vo)
    k = d.create(voc, f, ki.TH)
    before = d.state(k)
    ids = [p for _, p in d.s.keyframe_result()["created"]]
    assert len(ids) == 102
    d.s.refresh_points(ids)
    after = d.state(k)
    for key in before:
        assert np.asarray(before[key]).tobytes() == np.asarray(after[key]).tobytes(), key
    assert d.s.connections_status() == 0


@pytest.mark.parametrize("dev", [False, True], ids=["host_form", "dev_form"])
def test_need_stats(vo, dev):
    import torch
    d, mr = _pair(vo, dev=dev)
    f, _ = TABLES["holder_rules"]
    for ref_kf, min_obs in ((0, 2), (0, 3), (3, 5), (5, 99), (2, 2), (4, 2), (9, 2), (-1, 2)):
        if dev:
            out = torch.full((4,), -7, dtype=torch.int32, device="cuda")
            d.s.keyframe_need_stats(ref_kf, min_obs, torch.from_numpy(f["depth"]).cuda(), torch.from_numpy(f["slot_ids"]).cuda(), float(ki.TH), out)
            got = tuple(int(x) for x in out.cpu())
            assert got[3] == 0
            got = got[:3]
        else:
            got = d.s.keyframe_need_stats(ref_kf, min_obs, f["depth"], f["slot_ids"], float(ki.TH))
        assert got == mr.m.need_stats(ref_kf, min_obs, f["depth"], f["slot_ids"], ki.TH), (ref_kf, min_obs)
        assert d.s.connections_status() == mr.m.sticky == (1 if ref_kf in (2, 9, -1) else 0)
        mr.m.sticky = 0
    assert mr.m.need_stats(0, 2, f["depth"], f["slot_ids"], ki.TH)[1:] == (7, 12)


def test_device_form_does_not_synchronise(vo, voc):
    """the call is made while the producer of its inputs is still enqueued on the store's stream: it returns with the stream
    busy, and the result is the model's"""
    import torch
    f, _ = TABLES["fewer_than_101_near"]
    st = torch.cuda.Stream()
    d, mr = KDev(vo, 8, ki.NK, dev=False, stream=st.cuda_stream), _model(vo)
    for s in ki.holder_store():
        d.step(s), mr.step(s)
    host = {k: torch.from_numpy(np.ascontiguousarray(f[k])).pin_memory() for k in COLUMNS}
    with torch.cuda.stream(st):
        torch.cuda._sleep(200_000_000)                     # a tenth of a second of device time in front of the inputs
        t = {k: v.to("cuda", non_blocking=True) for k, v in host.items()}
        k = d.s.create_keyframe(voc, t, float(ki.TH))
        busy = not st.query()
    d.n.append(len(f["depth"]))
    assert busy
    st.synchronize()
    assert k == mr.m.create_keyframe(f, ki.TH)
    _same_call(d, mr.m, k, "stream")


def test_errors_change_nothing(vo, voc):
    f, _ = TABLES["all_below"]
    d, mr = _pair(vo, K=7)
    k = d.create(voc, f, ki.TH)
    mr.m.create_keyframe(f, ki.TH)
    with pytest.raises(vo.VoError, match="status -4"):             # the store is full
        d.s.create_keyframe(voc, f, float(ki.TH))
    big = ki.random_frame(1, ki.NK + 1, ki.HELD)
    e = KDev(vo, 2, ki.NK)
    with pytest.raises(vo.VoError, match="status -4"):             # n > max_features
        e.s.create_keyframe(voc, big, float(ki.TH))
    bad = dict(f, octave=np.where(np.arange(len(f["octave"])) == 5, 8, f["octave"]).astype(np.int32))
    with pytest.raises(vo.VoError, match="status -1"):             # an octave outside the store's eight levels (host form)
        e.s.create_keyframe(voc, bad, float(ki.TH))
    assert len(e.s) == 0 and e.s.next_point_id() == ki.FIRST_ID
    _same_call(d, mr.m, k, "after the refusals")
    plain = KDev(vo, 2, ki.NK, layer=False)
    with pytest.raises(vo.VoError, match="enable_keyframe_create"):
        plain.s.create_keyframe(voc, f, float(ki.TH))
    with pytest.raises(vo.VoError, match="status -1"):
        plain.s.keyframe_need_stats(0, 2, f["depth"], f["slot_ids"], float(ki.TH))
    late = KDev(vo, 2, ki.NK, layer=False)
    late.step(ki.holder_store()[0])
    with pytest.raises(vo.VoError, match="status -1"):             # valid on an empty store only
        late.s.enable_keyframe_create()
    wide = vo.KeyFrameStore(2, 16385)                               # the FeatureVector kernel sorts 16384: no such store gets as far
    wide.enable_connections(), wide.enable_culling()
    with pytest.raises(vo.VoError, match="status -4"):
        wide.enable_mapping(ki.CAM6, ki.SF, 0)
    with pytest.raises(vo.VoError, match="status -1"):
        wide.enable_keyframe_create()
    bare = vo.KeyFrameStore(2, ki.NK)
    with pytest.raises(vo.VoError, match="status -1"):             # needs the local-BA layer
        bare.enable_keyframe_create()


GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "point_upkeep_without_keyframe_create.npz"


def upkeep_snapshot(vo):
    """two of test_gpu_point_upkeep's scenes (the processNewKeyFrame case and the cull script) on stores WITHOUT the layer ->
    every byte the getters return, as a flat dict of arrays"""
    out = {}
    for name, script, K in (("process", ui.process_cases()["tracked_and_created_with"], 6), ("cull", ui.cull_script() + [("cullmp", 6)], 7)):
        d = UDev(vo, K, ui.NK_HAND, ui.CAPS)
        for s in script:
            d.step(s)
        for k in range(K):
            for key, v in d.state(k).items():
                out[f"{name}_kf{k}_{key}"] = np.asarray(v)
            c = d.s.connections(k)
            for key in ("weights", "ordered", "ordered_weights", "children"):
                out[f"{name}_kf{k}_{key}"] = np.array(c[key], np.int32)
            out[f"{name}_kf{k}_graph"] = np.array([c["n_connected"], c["parent"]], np.int32)
        rec = d.s.upkeep_result()
        out[f"{name}_recent"] = np.array(d.s.recent_points(), np.int32).reshape(-1, 4)
        out[f"{name}_record"] = np.array([rec[key] for key in vo.KeyFrameStore.UPKEEP_RECORD] + rec["erased"], np.int32)
        out[f"{name}_sticky"] = np.array([d.s.connections_status()], np.int32)
    return out


def test_a_store_without_the_layer_is_the_parent_commits(vo):
    """the fixture holds upkeep_snapshot() as the library of the commit before this layer gave it"""
    want = np.load(GOLDEN)
    got = upkeep_snapshot(vo)
    assert sorted(got) == sorted(want.files) and len(got) > 100
    for key in got:
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), key


def test_the_generation_word_advances(vo, voc):
    """a local-BA window taken before the call is no longer the store's: its apply is refused"""
    f, _ = TABLES["holder_rules"]
    d, mr = _pair(vo)
    d.s.local_ba_window(5)
    d.create(voc, f, ki.TH)
    with pytest.raises(vo.VoError, match="changed since"):
        d.s.local_ba_apply(np.zeros((1, 6)), np.zeros((1, 3)), np.zeros(1, np.uint8))


@pytest.mark.parametrize("dev", [False, True], ids=["host_form", "dev_form"])
def test_chain(vo, voc, dev):
    """create (initial) -> process, four times need_stats -> create -> process, then create_map_points and the local-BA window"""
    m, log = ki.model_chain(exp=_exp(vo), log=_log(vo))
    d = KDev(vo, ki.K_CHAIN, ki.N_CHAIN, dev)
    r = _model(vo)
    for k, f in enumerate(log["frames"]):
        if k:
            got = d.s.keyframe_need_stats(k - 1, 2 if k <= 2 else 3, f["depth"], f["slot_ids"], float(ki.CHAIN_TH))
            assert got == log["stats"][k - 1] == r.m.need_stats(k - 1, 2 if k <= 2 else 3, f["depth"], f["slot_ids"], ki.CHAIN_TH), k
        assert d.create(voc, f, ki.CHAIN_TH, initial=k == 0) == r.m.create_keyframe(f, ki.CHAIN_TH, k == 0, log["nodes"][k]) == k
        assert d.s.keyframe_result() == log["records"][k], k
        d.s.process_new_keyframe(k), r.m.process_new_keyframe(k)
        for j in range(k + 1):
            _same_keyframe(d, r.m, j, ("chain", k))
        assert [d.s.connections(j) for j in range(k + 1)] == [r.m.connections(j) for j in range(k + 1)], k
        assert d.s.recent_points() == r.m.recent_points() and d.s.upkeep_result() == r.m.upkeep_result(), k
    last = ki.K_CHAIN - 1
    d.s.create_map_points(last, 10), r.m.create(last, 10)
    assert d.s.new_points_result() == dict(neighbors=r.m.np_result["neighbors"], created=r.m.np_result["created"])
    assert len(r.m.np_result["created"]) > 5
    assert d.s.recent_points() == r.m.recent_points()
    d.s.local_ba_window(last), r.m.window(last)
    w = d.s.local_ba_window_result()
    assert w["record"] == {key: r.m.record[key] for key in w["record"]} == {key: log["window"][key] for key in w["record"]}
    for key in ("cam_keyframe", "fixed", "point_id", "e_cam", "e_pt", "e_feature", "e_obs", "e_inv_sigma"):
        assert np.asarray(w[key]).tobytes() == np.asarray(r.m.win[key]).tobytes(), key
    # the points create_keyframe made are the model's bytes; those create_map_points triangulated agree within vo_triangulate's
    # stated tolerance (tests/new_points_ref.py: TAU)
    from new_points_ref import TAU
    tri = np.isin(w["point_id"], [row[3] for row in r.m.np_result["created"]])
    assert tri.sum() == len(r.m.np_result["created"])
    assert w["points"][~tri].tobytes() == r.m.win["points"][~tri].tobytes()
    assert np.all(np.linalg.norm(w["points"][tri] - r.m.win["points"][tri], axis=1) <= 2 * TAU * np.linalg.norm(r.m.win["points"][tri], axis=1))
    assert [d.s.connections(j) for j in range(ki.K_CHAIN)] == [r.m.connections(j) for j in range(ki.K_CHAIN)]
    assert d.s.connections_status() == r.m.sticky == 0
