"""Plain-Python restatement of the key-frame database contract: Map::insertKeyFrame's inverted
index, Map::detectRelocalizationCandidates, Map::detectLoopCandidates with detectLoop's minScore loop, and the BoW vector
of DBoW3::Vocabulary::transform.  Per-key-frame members are carried across queries exactly as the reference's are
(relocateFrameId_, relocateWordCnt_, relocateScore_, loopKFId_, loopWordCnt_, loopScore_); float steps are np.float32,
double steps Python floats (IEEE binary64), in the reference's order.  Frame / key-frame ids passed to the queries must be
positive and distinct (id 0 collides with the members' initial value and is not reproduced)."""
import bisect

import numpy as np

F32 = np.float32


def bow_vector(words, weights):
    """(word, weight) per feature -> (ascending distinct words int32, L1-normalised values float64): an ordered map kept as
    two sorted lists, addWeight in feature order, normalize(L1) in word order"""
    ks, vs = [], []
    for w, x in zip(words, weights):
        x = float(x)
        if not x > 0:
            continue
        w = int(w)
        i = bisect.bisect_left(ks, w)
        if i < len(ks) and ks[i] == w:
            vs[i] = vs[i] + x
        else:
            ks.insert(i, w)
            vs.insert(i, x)
    norm = 0.0
    for x in vs:
        norm = norm + abs(x)
    if norm > 0.0:
        vs = [x / norm for x in vs]
    return np.array(ks, np.int32), np.array(vs, np.float64)


def score(w1, v1, w2, v2):
    """Map::score: the merge over two ascending vectors, FP64"""
    i = j = 0
    n1, n2 = len(w1), len(w2)
    s = 0.0
    while i < n1 and j < n2:
        a, b = w1[i], w2[j]
        if a == b:
            vi, wi = v1[i], v2[j]
            s = s + ((abs(vi - wi) - abs(vi)) - abs(wi))
            i += 1
            j += 1
        elif a < b:
            i += 1
        else:
            j += 1
    return -s / 2.0


class KeyFrame:
    def __init__(self, index, words, values):
        self.index = index
        self.words = [int(w) for w in words]
        self.values = [float(v) for v in values]
        self.neighbors = []          # getBestCovisibleKFs(10), in its order
        self.reloc_frame_id = 0
        self.reloc_word_cnt = 0
        self.reloc_score = F32(0.0)
        self.loop_kf_id = 0
        self.loop_word_cnt = 0
        self.loop_score = F32(0.0)


class Database:
    def __init__(self):
        self.kfs = []
        self.inverted = {}
        self.trace = {}              # what the last query did, for the coverage assertions of the fixture

    def insert(self, words, values):
        kf = KeyFrame(len(self.kfs), words, values)
        self.kfs.append(kf)
        for w in kf.words:
            self.inverted.setdefault(w, []).append(kf)
        return kf.index

    def set_neighbors(self, index, ids):
        assert len(ids) <= 10
        self.kfs[index].neighbors = [self.kfs[i] for i in ids]

    # ------------------------------------------------------------------ Map::detectRelocalizationCandidates
    def detect_reloc(self, frame_id, words, values):
        assert frame_id > 0
        tr = self.trace = dict(kind="reloc", early=None)
        qw, qv = [int(w) for w in words], [float(v) for v in values]
        sharing = []
        for w in qw:
            for kf in self.inverted.get(w, ()):
                if kf.reloc_frame_id != frame_id:
                    kf.reloc_word_cnt = 0
                    kf.reloc_frame_id = frame_id
                    sharing.append(kf)
                kf.reloc_word_cnt += 1
        tr["sharing"] = [kf.index for kf in sharing]
        if not sharing:
            tr["early"] = "sharing"
            return []
        max_common = 0
        for kf in sharing:
            if kf.reloc_word_cnt > max_common:
                max_common = kf.reloc_word_cnt
        min_common = int(0.8 * max_common)
        tr["max_common"], tr["min_common"] = max_common, min_common
        scored = []
        for kf in sharing:
            if kf.reloc_word_cnt > min_common:
                sc = F32(score(qw, qv, kf.words, kf.values))
                kf.reloc_score = sc
                scored.append((sc, kf))
        tr["scored"] = [kf.index for _, kf in scored]
        if not scored:
            tr["early"] = "scored"
            return []
        groups = []
        best_group = F32(0.0)
        scored_set = set(tr["scored"])
        tr["stale_nonzero"] = tr["stale_zero"] = 0
        for sc, kf in scored:
            best, group, best_kf = sc, sc, kf
            for n in kf.neighbors:
                if n.reloc_frame_id != frame_id:
                    continue
                if n.index not in scored_set:
                    tr["stale_nonzero" if n.reloc_score != 0 else "stale_zero"] += 1
                group = F32(group + n.reloc_score)
                if n.reloc_score > best:
                    best_kf, best = n, n.reloc_score
            groups.append((group, best_kf))
            if group > best_group:
                best_group = group
        return self._keep(groups, best_group, tr)

    @staticmethod
    def _keep(groups, best_group, tr):
        keep = F32(0.75) * best_group
        tr["groups"] = [(float(g), kf.index) for g, kf in groups]
        tr["keep"] = float(keep)
        added, out = set(), []
        tr["duplicates"] = 0
        for g, kf in groups:
            if g > keep:
                if kf.index not in added:
                    added.add(kf.index)
                    out.append(kf.index)
                else:
                    tr["duplicates"] += 1
        return out

    # ------------------------------------------------------------------ LoopClosing::detectLoop :71-83
    def min_score(self, words, values, connected):
        qw, qv = [int(w) for w in words], [float(v) for v in values]
        m = F32(1.0)
        for c in connected:
            kf = self.kfs[c]
            sc = F32(score(qw, qv, kf.words, kf.values))
            if sc < m:
                m = sc
        return m

    # ------------------------------------------------------------------ Map::detectLoopCandidates
    def detect_loop(self, kf_id, words, values, excluded, min_score):
        assert kf_id > 0
        tr = self.trace = dict(kind="loop", early=None)
        min_score = F32(min_score)
        qw, qv = [int(w) for w in words], [float(v) for v in values]
        connect = set(int(e) for e in excluded)
        sharing = []
        seen_excluded = {}
        for w in qw:
            for kf in self.inverted.get(w, ()):
                if kf.loop_kf_id != kf_id:
                    kf.loop_word_cnt = 0
                    if kf.index not in connect:
                        kf.loop_kf_id = kf_id
                        sharing.append(kf)
                    else:
                        seen_excluded[kf.index] = seen_excluded.get(kf.index, 0) + 1
                kf.loop_word_cnt += 1
        tr["sharing"] = [kf.index for kf in sharing]
        tr["excluded_shared"] = seen_excluded      # shared words of the excluded key-frames (never compared by the query)
        if not sharing:
            tr["early"] = "sharing"
            return []
        max_common = 0
        for kf in sharing:
            if kf.loop_word_cnt > max_common:
                max_common = kf.loop_word_cnt
        min_common = int(F32(0.8) * F32(max_common))
        tr["max_common"], tr["min_common"] = max_common, min_common
        scored = []
        tr["scored_all"] = []
        for kf in sharing:
            if kf.loop_word_cnt > min_common:
                sc = F32(score(qw, qv, kf.words, kf.values))
                kf.loop_score = sc
                tr["scored_all"].append(kf.index)
                if sc >= min_score:
                    scored.append((sc, kf))
        tr["scored"] = [kf.index for _, kf in scored]
        if not scored:
            tr["early"] = "scored"
            return []
        groups = []
        best_group = min_score
        for sc, kf in scored:
            best, group, best_kf = sc, sc, kf
            for n in kf.neighbors:
                if n.loop_kf_id == kf_id and n.loop_word_cnt > min_common:
                    group = F32(group + n.loop_score)
                    if n.loop_score > best:
                        best_kf, best = n, n.loop_score
            groups.append((group, best_kf))
            if group > best_group:
                best_group = group
        return self._keep(groups, best_group, tr)

    # ------------------------------------------------------------------ the batched entry points' pure-function form
    def reloc_scores(self):
        return np.array([kf.reloc_score for kf in self.kfs], np.float32)

    def query_reloc(self, words, values, stale=None):
        """one query of vo_kfdb_query_reloc: the members are set from `stale` first -> (candidates, score_out row)"""
        self._next_id = getattr(self, "_next_id", 1 << 20) + 1
        for i, kf in enumerate(self.kfs):
            kf.reloc_score = F32(0.0) if stale is None else F32(stale[i])
        cands = self.detect_reloc(self._next_id, words, values)
        return cands, self.reloc_scores()

    def query_loop(self, words, values, excluded, min_score=None, connected=None):
        """one query of vo_kfdb_query_loop -> (candidates, score_out row: loopScore_ where written by this query, else -1)"""
        self._next_id = getattr(self, "_next_id", 1 << 20) + 1
        if min_score is None:
            min_score = self.min_score(words, values, connected)
        cands = self.detect_loop(self._next_id, words, values, excluded, min_score)
        row = np.full(len(self.kfs), -1.0, np.float32)
        for i in self.trace.get("scored_all", ()):
            row[i] = self.kfs[i].loop_score
        return cands, row
