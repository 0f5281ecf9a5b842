"""Seeded fixture of the relocalisation route (test infrastructure): synthetic frames, and per frame an ordered list of
candidate key-frames made the way test_track_ref_keyframe_route makes its key-frame -- the frame's own features,
shuffled, with descriptor noise, given map points (the features back-projected with their depth) and ids.  The true
pose is the identity.  A map point keeps its id in every candidate of a frame (id = the frame feature it came from), so
that `found` and the slots a rejected candidate leaves behind mean something; the candidate built to leak uses an id
range of its own.  The knobs per candidate -- which features it holds, which of them have a descriptor the BoW search
can match, how their map points are disturbed -- are set so that the batch walks every branch of
visualOdometry.cpp:313-395 (tests/test_reloc_ref.py asserts that from the model's branch trace)."""
import numpy as np

from vo_slam_test_amd import synth

W, H = 640, 480
START = 80          # first synthetic frame index
N_FRAMES = 6
MAX_CAND = 3
LEAK_FRAME, LEAK_CAND = 2, 0


def oracle_frames(orc, imgs, raw, inv, cam5):
    p = orc.orb_params()
    out = []
    for f in range(len(imgs)):
        k, d, _ = orc.extract(p, imgs[f])
        n = len(k)
        x, y = np.ascontiguousarray(k["x"]), np.ascontiguousarray(k["y"])
        ux, uy = np.zeros(n, np.float32), np.zeros(n, np.float32)
        orc.lib().orc_undistort_points(n, x, y, cam5[:4].copy(), None, ux, uy)
        dimg = np.zeros((H, W), np.float32)
        orc.lib().orc_depth_to_float(np.ascontiguousarray(raw[f]).reshape(-1), H * W, inv, dimg.reshape(-1))
        ur, dep = np.zeros(n, np.float32), np.zeros(n, np.float32)
        orc.lib().orc_find_depth(n, x, y, ux, dimg, W, H, W, float(cam5[4]), ur, dep)
        out.append((k, d, ux, uy, ur, dep))
    return out


def bow_transform(orc, vd, desc, levelsup=3):
    """per-feature node ids (Frame::computeBow) on the oracle"""
    n = len(desc)
    word, weight, node = np.zeros(n, np.int32), np.zeros(n, np.float64), np.zeros(n, np.int32)
    orc.lib().orc_bow_transform(int(vd["L"]), np.ascontiguousarray(vd["child_start"], np.int32), np.ascontiguousarray(vd["children"], np.int32),
                                np.ascontiguousarray(vd["node_desc"], np.uint8), np.ascontiguousarray(vd["node_weight"], np.float64),
                                np.ascontiguousarray(vd["word_id"], np.int32), n, np.ascontiguousarray(desc, np.uint8), levelsup, word, weight,
                                node)
    return node


def _backproject(ux, uy, z, cam5):
    fx, fy, cx, cy = (float(c) for c in cam5[:4])
    return np.stack([(ux.astype(np.float64) - cx) * z / fx, (uy.astype(np.float64) - cy) * z / fy, z], axis=1)


def make_candidate(rng, fr, cam5, node_of, keep, matchable, px_noise=0.0, garbage=None, offset=None, id_base=0, desc_noise=0.01,
                   bad=False, tight=None):
    """keep: frame features the key-frame holds; matchable [len(keep)] bool: the feature's descriptor is the frame's (with
    noise), else random; px_noise: pixel disturbance of the back-projection; garbage [len(keep)] bool: a map point
    somewhere else; offset: se3 applied to the map points of the MATCHABLE features (a consistent wrong pose); tight
    [len(keep)] bool: the map point's distance range ends 4 % beyond its true distance (the gate of matcher.cpp:198 lets
    it through from the true camera centre only)."""
    k, d, ux, uy, ur, dep = fr
    keep = np.asarray(keep)
    perm = rng.permutation(len(keep))
    idx = keep[perm]
    matchable = np.asarray(matchable, bool)[perm]
    n = len(idx)
    z = np.where(dep[idx] > 0, dep[idx], 2.5).astype(np.float64)
    du = rng.normal(0, 1.0, (n, 2))
    du = px_noise * du / np.maximum(np.linalg.norm(du, axis=1, keepdims=True), 1e-9) if px_noise > 0 else np.zeros((n, 2))
    P = _backproject(ux[idx] + du[:, 0].astype(np.float32), uy[idx] + du[:, 1].astype(np.float32), z, cam5)
    if garbage is not None:
        g = np.asarray(garbage, bool)[perm]
        P[g] = np.stack([rng.uniform(-2, 2, g.sum()), rng.uniform(-1.5, 1.5, g.sum()), rng.uniform(1, 6, g.sum())], 1)
    if offset is not None:  # points consistent with Tcw = exp(offset): p' = T^-1 p
        R, t = synth.se3_exp(np.asarray(offset, np.float64))
        P[matchable] = (P[matchable] - t) @ R
    desc = d[idx].copy()
    flip = rng.random(desc.shape) < desc_noise
    desc[flip] ^= rng.integers(1, 256, int(flip.sum()), dtype=np.uint8)
    desc[~matchable] = rng.integers(0, 256, (int((~matchable).sum()), 32), dtype=np.uint8)
    pdesc = d[idx].copy()
    flip = rng.random(pdesc.shape) < desc_noise
    pdesc[flip] ^= rng.integers(1, 256, int(flip.sum()), dtype=np.uint8)
    dist = np.linalg.norm(P, axis=1)
    maxd = (dist * 1.2 ** k["octave"][idx].astype(np.float64)).astype(np.float32)
    if tight is not None:
        tg = np.asarray(tight, bool)[perm]
        maxd[tg] = (dist[tg] * 1.04 / 1.2).astype(np.float32)  # getMaxDistanceThreshold() = 1.2 maxDistance_
    flags = np.ones(n, np.uint8)
    flags[rng.random(n) < 0.03] = 0
    return dict(angle=k["angle"][idx].astype(np.float32), desc=desc, nodes=node_of(desc), flags=flags, points=P,
                ids=(id_base + idx).astype(np.int32), point_desc=pdesc, min_dist=(maxd / np.float32(1.2 ** 7)).astype(np.float32),
                max_dist=maxd, bad=bad, frame_index=idx)


def build(orc, seed=0, n_frames=N_FRAMES):
    """-> dict(imgs, raw, inv, cam5, sf, vocab (synth dict), frames (oracle frames), fnodes, candidates [B][<= MAX_CAND], nk)"""
    imgs = synth.make_frames(n_frames, start=START)
    raw = np.stack([synth.make_depth(START + i) for i in range(n_frames)])
    inv = np.float32(1.0) / np.float32(synth.DEPTH_SCALE)
    cam5 = synth.CAM.astype(np.float32)
    sf = np.array(list(orc.orb_params().scale)[:8], np.float32)
    vd = synth.make_vocabulary(3, k=8, L=4)
    frames = oracle_frames(orc, imgs, raw, inv, cam5)
    node_of = lambda desc: bow_transform(orc, vd, desc)
    fnodes = [node_of(fr[1]) for fr in frames]
    rng = np.random.default_rng(0x5E10C + seed)
    nk = max(len(fr[0]) for fr in frames)
    cands = []
    for f, fr in enumerate(frames):
        n = len(fr[0])
        every, ones = np.arange(n), np.ones(n, bool)
        few = lambda m: np.isin(every, rng.choice(n, m, replace=False))  # only m features have a descriptor BoW can match
        mk = lambda keep, matchable, **kw: make_candidate(rng, fr, cam5, node_of, keep, matchable, **kw)
        unrelated = lambda: mk(every, np.zeros(n, bool))            # < 15 BoW matches
        low = every[fr[0]["octave"] == 0]
        loose = lambda: mk(low[rng.choice(len(low), 40, replace=False)], np.ones(40, bool), px_noise=7.0, desc_noise=0.0)  # PnP >= 10, solve < 10
        if f % 6 == 0:    # a bad candidate, then success straight after the first solve; the third is never reached
            cl = [mk(every, ones, bad=True), mk(every, ones), mk(every, ones)]
        elif f % 6 == 1:  # too few BoW matches, then success through the first top-up only
            cl = [unrelated(), mk(every, few(35))]
        elif f % 6 == 2:  # 0 < PnP inliers < 10 with ids of its own that leak into the winner's solve
            own = rng.choice(n, 20, replace=False)
            g = np.zeros(20, bool)
            g[9:] = True
            rest = np.setdiff1d(every, own)
            cl = [mk(own, np.ones(20, bool), garbage=g, id_base=nk, desc_noise=0.0), mk(rest, np.ones(len(rest), bool))]
        elif f % 6 == 3:
            # Success through both top-ups.  The BoW matches are 19 features: 12 carry map points consistent with a camera
            # 0.2 m behind the true one, 7 carry points elsewhere (PnP outliers), so PnP and the first solve settle there.  From that centre the first top-up sees
            # only 49 features within 120 px of the principal point (they move < 10 px); the level-0/1 points have a distance
            # range that ends 4 % beyond their true distance and fail the gate.  The second solve, now with more true
            # points than displaced ones, comes back to the true pose with 30..50 inliers; from there the second top-up
            # admits the level-0/1 points.
            k_ = fr[0]
            r2 = (fr[2] - cam5[2]) ** 2 + (fr[3] - cam5[3]) ** 2
            centre = rng.choice(every[r2 < 120.0 ** 2], 49, replace=False)
            lowlev = np.setdiff1d(every[k_["octave"] <= 1], centre)
            others = np.setdiff1d(every, np.concatenate([centre, lowlev]))
            biased = others[rng.choice(len(others), 19, replace=False)]
            keep = np.concatenate([biased, centre, lowlev])
            cl = [mk(keep, np.isin(keep, biased), garbage=np.isin(keep, biased[12:]), offset=[0, 0, 0.2, 0, 0, 0],
                     tight=np.isin(keep, lowlev), desc_noise=0.0)]
        elif f % 6 == 4:  # every candidate fails
            cl = [unrelated(), loose()]
        else:             # no candidates
            cl = []
        cands.append(cl)
    return dict(imgs=imgs, raw=raw, inv=inv, cam5=cam5, sf=sf, vocab=vd, frames=frames, fnodes=fnodes, candidates=cands, nk=nk)
