"""Model of vo_kfstore_update_connections (test infrastructure): KeyFrame::updateConnections, addConnection and
updateBestCovisibles (src/keyframe.cpp:69-198) restated over the list-of-dicts store of tests/local_map_ref.py, in plain
Python.  Only `ids` and `flags` of a key-frame are read; key-frame j HOLDS id p when one of its features has ids == p and
bit 0 set (local_map_ref.holders), and the `bad` flag plays no part.

State per key-frame k (class Connections):
  W[k]              connectedKFWts_: {key-frame number: weight}
  ordered[k]        orderedConnectKFs_, weights[k] orderedWTs_
  first_connect[k]  firstConnect_
  parent[k]         key-frame number or -1
  children[k]       set of key-frame numbers (read in ascending number)

Pointer-keyed containers are walked in ascending key-frame number; sort((weight, KeyFrame*)) ascending followed by
push_front gives weight descending with ties in DESCENDING key-frame number."""

THRESHOLD = 15
MAX_NEIGHBORS = 10
MAX_CHILDREN = 64


def holder_index(store):
    """id -> ascending list of the key-frames that hold it (local_map_ref.holders for every id at once)"""
    index = {}
    for k in range(len(store)):
        kf = store[k]
        for i in range(len(kf["ids"])):
            if kf["flags"][i] & 1:
                hs = index.setdefault(kf["ids"][i], [])
                if not hs or hs[-1] != k:
                    hs.append(k)
    return index


def counts(store, k, index=None):
    """C of update(k): {j: features of k with bit 0 set whose id j holds}, j != k (:80-93)"""
    if index is None:
        index = holder_index(store)
    C = {}
    kf = store[k]
    for i in range(len(kf["ids"])):
        if not (kf["flags"][i] & 1):
            continue
        for j in index.get(kf["ids"][i], []):
            if j == k:
                continue
            C[j] = C.get(j, 0) + 1
    return C


def _sorted(pairs):
    """[(weight, key-frame)] -> (key-frames, weights): sort ascending, then push_front (:127-134)"""
    kfs, wts = [], []
    for w, j in sorted(pairs):
        kfs.insert(0, j)
        wts.insert(0, w)
    return kfs, wts


class Connections:
    def __init__(self):
        self.W, self.ordered, self.weights, self.first_connect, self.parent, self.children = [], [], [], [], [], []

    def grow(self, n):
        while len(self.W) < n:
            self.W.append({})
            self.ordered.append([])
            self.weights.append([])
            self.first_connect.append(True)
            self.parent.append(-1)
            self.children.append(set())

    def add_connection(self, j, k, w):
        """addConnection on key-frame j (:157-171) + updateBestCovisibles (:176-198)"""
        if k in self.W[j] and self.W[j][k] == w:
            return
        self.W[j][k] = w
        self.ordered[j], self.weights[j] = _sorted([(wt, x) for x, wt in self.W[j].items()])

    def update(self, store, k, index=None):
        self.grow(len(store))
        C = counts(store, k, index)
        if not C:
            return
        nmax, kfmax = 0, -1
        pairs = []
        for j in sorted(C):
            if C[j] > nmax:
                nmax, kfmax = C[j], j
            if C[j] >= THRESHOLD:
                pairs.append((C[j], j))
                self.add_connection(j, k, C[j])
        if not pairs:
            pairs.append((nmax, kfmax))
            self.add_connection(kfmax, k, nmax)
        self.W[k] = dict(C)
        self.ordered[k], self.weights[k] = _sorted(pairs)
        if self.first_connect[k] and k != 0:
            self.parent[k] = self.ordered[k][0]
            self.children[self.parent[k]].add(k)
            self.first_connect[k] = False

    def update_list(self, store, keyframes):
        """update(k) in list order; the index is built once: the store does not change inside a call"""
        index = holder_index(store)
        for k in keyframes:
            self.update(store, k, index)

    def state(self, k, size):
        """what vo_kfstore_get_connections returns for key-frame k of a store of `size` key-frames"""
        row = [self.W[k].get(j, 0) for j in range(size)]
        ch = sorted(self.children[k])[:MAX_CHILDREN]
        return dict(n_connected=len(self.W[k]), weights=row, ordered=list(self.ordered[k]), ordered_weights=list(self.weights[k]),
                    parent=self.parent[k], children=ch)

    def graph(self, k):
        """the graph row vo_kfstore_set_graph takes: getBestCovisibleKFs(10), children ascending (the lowest 64), parent"""
        return self.ordered[k][:MAX_NEIGHBORS], sorted(self.children[k])[:MAX_CHILDREN], self.parent[k]
