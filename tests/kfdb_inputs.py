"""Seeded inputs for the key-frame database tests: key-frames along a closed trajectory of "places" (every place has its
own word pool, neighbouring places overlap, the end of the trajectory revisits its start), repeated words per frame,
idf-like weights with a few stop words, covisibility lists of at most 10."""
import numpy as np

import kfdb_ref

N_WORDS = 100_000
SIZES = (0, 1, 37, 500, 4096)
PER_PLACE = 4        # consecutive key-frames per place
POOL = 260           # words of a place
N_FEAT = 180         # features per frame


class Scene:
    def __init__(self, n_kf, seed=0):
        rng = np.random.default_rng(1000 + seed)
        self.rng = rng
        self.n_kf = n_kf
        # the last fifth of the trajectory walks over the first places again
        self.n_places = max(1, int(np.ceil(n_kf / PER_PLACE * 0.8)))
        self.idf = rng.uniform(0.5, 8.0, N_WORDS)
        self.idf[rng.random(N_WORDS) < 0.02] = 0.0                       # stop words
        self.pools = [rng.choice(N_WORDS - 1000, POOL, replace=False) for _ in range(self.n_places)]  # the top 1000 ids stay unused
        self.place = [(i // PER_PLACE) % self.n_places for i in range(n_kf)]
        self.features = [self.frame_features(self.place[i]) for i in range(n_kf)]
        self.vectors = [kfdb_ref.bow_vector(w, x) for w, x in self.features]
        self.neighbors = [self.covisible(i, n_kf) for i in range(n_kf)]

    def frame_features(self, place, own=0.7, n=N_FEAT):
        """per-feature (word, weight): `own` of the features from the place's pool, the rest from the two neighbouring places;
        draws favour the front of a pool, so words repeat within a frame"""
        rng, P = self.rng, self.n_places
        src = rng.random(n)
        side = np.where(src < own, 0, np.where(src < own + (1 - own) / 2, -1, 1))
        pick = np.minimum((rng.random(n) ** 2 * POOL).astype(int), POOL - 1)
        words = np.array([self.pools[(place + s) % P][k] for s, k in zip(side, pick)], np.int32)
        return words, self.idf[words].copy()

    def covisible(self, i, size):
        """at most 10 of the key-frames around i (and around its earlier visit of the place), in a shuffled weight order,
        restricted to insertion numbers < size"""
        rng = self.rng
        around = [j for j in range(i - 7, i + 8) if j != i and 0 <= j < size]
        first_visit = [j for j in range(size) if j < i - 8 and self.place[j] == self.place[i]][:3]
        ids = np.array(around + first_visit, np.int64)
        rng.shuffle(ids)
        return [int(j) for j in ids[:10]]

    def lost_frame(self, place, own=0.7):
        w, x = self.frame_features(place % self.n_places, own)
        return kfdb_ref.bow_vector(w, x)

    def reloc_queries(self, n, seed=0):
        """lost frames walking along the trajectory (so that consecutive queries see neighbouring places); every 17th one
        carries only unused words, every 29th is empty"""
        rng = np.random.default_rng(2000 + seed)
        out, place = [], int(rng.integers(0, self.n_places))
        for i in range(n):
            if i % 29 == 28:
                out.append((np.zeros(0, np.int32), np.zeros(0, np.float64)))
            elif i % 17 == 16:
                w = np.sort(rng.choice(np.arange(N_WORDS - 1000, N_WORDS), 40, replace=False)).astype(np.int32)
                out.append((w, np.full(40, 1.0 / 40)))
            else:
                out.append(self.lost_frame(place, own=float(rng.choice([0.5, 0.7, 0.9]))))
            if rng.random() < 0.6:
                place = (place + int(rng.integers(0, 2))) % self.n_places
            elif rng.random() < 0.2:
                place = int(rng.integers(0, self.n_places))
        return out

    def loop_queries(self, n, seed=0):
        """new key-frames asking for loop candidates: inserted key-frames themselves (the later ones revisit the start) ->
        list of dict(vector, excluded = connected key-frames and itself, connected = ordered covisibility list)"""
        rng = np.random.default_rng(3000 + seed)
        out = []
        if self.n_kf == 0:
            return out
        for i in range(n):
            k = self.n_kf - 1 - (i * 3) % self.n_kf if i % 2 == 0 else int(rng.integers(0, self.n_kf))
            conn = list(self.neighbors[k])
            excl = sorted(set(conn + [j for j in range(k - 3, k + 4) if 0 <= j < self.n_kf] + [k]))
            out.append(dict(kf=k, vector=self.vectors[k], excluded=excl, connected=conn))
        return out


def build_ref(scene, n=None):
    db = kfdb_ref.Database()
    n = scene.n_kf if n is None else n
    for i in range(n):
        db.insert(*scene.vectors[i])
    for i in range(n):
        db.set_neighbors(i, [j for j in scene.neighbors[i] if j < n])
    return db
