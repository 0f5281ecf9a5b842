"""Handles give back what they took ("Who owns device memory"): the free device memory after
repeated create / use / close cycles of every handle that owns arrays, the lazily laid-out store-route set of the tracker,
and the two "nothing has run yet" errors of a fresh tracker.

The sizes are chosen so that one handle takes at least 16 MiB: a leak of one array set per cycle then shows as about ten
footprints, far above anything the allocator's granularity or another process on the device could hide."""
import numpy as np
import pytest

import reloc_db_inputs
import reloc_inputs

pytestmark = pytest.mark.gpu

MiB = 1 << 20
CYCLES = 10
B = 2            # frames of the fixture: a bad candidate then a success; too few BoW matches then a success
CAP = 16384      # feature slots per frame (the most a frame store takes)
NK = 5000        # features per candidate: 3 x 5000 ids still sort in LDS, the route the other tests run


@pytest.fixture(scope="module")
def fx(orc):
    return reloc_inputs.build(orc, n_frames=B)


def _free():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _cycles(cycle):
    """cycle() creates a handle, uses it, returns (free memory while it lives, close).  -> (footprint, drop after CYCLES more)"""
    cycle()[1]()  # warm-up: per-thread scratch, code objects, the allocator's own pools
    base = _free()
    held, close = cycle()
    close()
    for _ in range(CYCLES):
        cycle()[1]()
    return base - held, base - _free()


def _check(footprint, drop, what):
    print(f"{what}: footprint {footprint / MiB:.1f} MiB, free memory down {drop / MiB:.1f} MiB after {CYCLES} cycles")
    assert footprint >= 16 * MiB, what
    assert drop < footprint / 2, what


def _tracker(vo, fx):
    return vo.Tracker(B, fx["cam5"], None, reloc_inputs.W, reloc_inputs.H, max_last=32768, max_local=32768, max_features=CAP,
                      inv_depth_scale=float(fx["inv"]), max_reloc_candidates=reloc_inputs.MAX_CAND, max_reloc_features=NK)


class _StoreRoute:
    """what a store route needs besides the tracker, made once: it must not count as any tracker's footprint"""

    def __init__(self, vo, fx):
        import torch
        vd = fx["vocab"]
        self.voc = vo.Vocabulary(vd["L"], vd["child_start"], vd["children"], vd["node_desc"], vd["node_weight"], vd["word_id"])
        self.kfs, self.lists = reloc_db_inputs.keyframes(fx)
        self.store = vo.KeyFrameStore(len(self.kfs), fx["nk"])
        for k in self.kfs:
            self.store.insert(k)
        cand = np.full((B, reloc_inputs.MAX_CAND), -1, np.int32)
        for f, ls in enumerate(self.lists):
            cand[f, :len(ls)] = ls
        self.n_cand = torch.tensor([len(ls) for ls in self.lists], dtype=torch.int32).cuda()
        self.cand = torch.from_numpy(cand).cuda()
        self.imgs, self.raw = fx["imgs"], fx["raw"].view(np.uint16)

    def run(self, trk):
        trk.relocalize_store(self.store, self.voc, self.n_cand, self.cand, self.imgs, self.raw)
        return trk.results()

    def run_host(self, trk):
        dense = [reloc_db_inputs.dense_ids([self.kfs[g] for g in ls])[0] for ls in self.lists]
        trk.set_reloc_candidates(self.voc, dense)
        trk.relocalize(self.imgs, self.raw)
        return trk.results()

    def close(self):
        self.store.close(), self.voc.close()


@pytest.fixture(scope="module")
def route(vo, fx):
    r = _StoreRoute(vo, fx)
    yield r
    r.close()


def test_tracker_cycles(vo, fx, route):
    def cycle():
        trk = _tracker(vo, fx)
        out = route.run(trk)  # the lazy sets exist from here
        assert (out["status"] & trk.RELOC_FAILED == 0).all()
        return _free(), trk.close

    _check(*_cycles(cycle), "Tracker")


def test_keyframe_store_cycles(vo, fx):
    kf = reloc_db_inputs.keyframes(fx)[0][1]

    def cycle():
        st = vo.KeyFrameStore(64, 4096)
        assert st.insert(kf) == 0 and len(st) == 1
        return _free(), st.close

    _check(*_cycles(cycle), "KeyFrameStore")


def test_keyframe_database_cycles(vo):
    words, values = np.arange(8, dtype=np.int32), np.full(8, 0.125)

    def cycle():
        db = vo.KeyFrameDatabase(4096, 2048, 512, 4)
        assert db.insert(words, values) == 0
        assert [list(c) for c in db.query_reloc([(words, values)])] == [[0]]
        return _free(), db.close

    _check(*_cycles(cycle), "KeyFrameDatabase")


def test_frames_cycles(vo, fx):
    k, d, ux, uy, ur, _ = fx["frames"][0]
    fa = vo.FrameArrays(ux, uy, k["octave"], k["angle"], ur, d)

    def cycle():
        fr = vo.Frames(16, CAP)
        fr.upload(3, fa)
        assert fr.download(3)["n"] == len(ux)
        return _free(), fr.close

    _check(*_cycles(cycle), "Frames")


def test_store_route_arrays_are_lazy(vo, fx, route):
    """a tracker that only ever relocalises from host candidates does not hold the store routes' arrays"""
    warm = _tracker(vo, fx)
    route.run_host(warm), route.run(warm)
    warm.close()
    base = _free()
    trk = _tracker(vo, fx)
    route.run_host(trk)
    before = base - _free()
    route.run(trk)
    after = base - _free()
    trk.close()
    print(f"tracker footprint {before / MiB:.1f} MiB before the first store route, {after / MiB:.1f} MiB after")
    assert after > before


def test_fresh_tracker_errors(vo, fx):
    trk = _tracker(vo, fx)
    with pytest.raises(vo.VoError, match=r"vo_tracker_results failed with status -1: vo_tracker_results: no batch has been tracked"):
        trk.results()
    with pytest.raises(vo.VoError, match=r"status -1: vo_tracker_track_local_map: no first stage has run \(vo_tracker_track_first / "
                                         r"_ref_keyframe_first\)"):
        trk.track_local_map()
    trk.close()
