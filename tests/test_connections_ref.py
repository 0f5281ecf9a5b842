"""The updateConnections model (tests/connections_ref.py) against an independent numpy formulation for a single update on
fresh state, the hand-made cases of tests/connections_inputs.py on the model, and the C-ABI of the new entry points (no GPU
needed: the calls below fail before they reach the device)."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import connections_inputs as ci
from connections_ref import THRESHOLD, Connections, counts, holder_index
from local_map_ref import holders

ROOT = pathlib.Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["vo_kfstore_enable_connections", "vo_kfstore_update_connections", "vo_kfstore_update_connections_dev",
               "vo_kfstore_connections_status", "vo_kfstore_get_connections"]


def _count_matrix(store):
    """C = F M^T with the diagonal zeroed: F[k][p] the flagged features of k that carry p, M[j][p] in {0, 1}"""
    ids = sorted({p for kf in store for p, f in zip(kf["ids"], kf["flags"]) if f & 1})
    col = {p: c for c, p in enumerate(ids)}
    F = np.zeros((len(store), len(ids)), np.int64)
    for k, kf in enumerate(store):
        for p, f in zip(kf["ids"], kf["flags"]):
            if f & 1:
                F[k, col[p]] += 1
    Cm = F @ (F > 0).astype(np.int64).T
    np.fill_diagonal(Cm, 0)
    return Cm


@pytest.fixture(scope="module")
def random_store():
    return ci.sliding_window_store(np.random.default_rng(7), 30, 60, 100, 10, 60)


def test_holder_index_is_local_map_refs_holders(random_store):
    index = holder_index(random_store)
    some = sorted(index)[::17] + [-5]
    assert all(index.get(p, []) == holders(random_store, p) for p in some)


def test_counts_equal_the_matrix_product(random_store):
    Cm = _count_matrix(random_store)
    assert (Cm != Cm.T).any() and (Cm >= THRESHOLD).any() and ((Cm > 0) & (Cm < THRESHOLD)).any()   # the store exercises all of it
    for k in range(len(random_store)):
        assert [counts(random_store, k).get(j, 0) for j in range(len(random_store))] == list(Cm[k])


def test_single_update_on_fresh_state_equals_the_numpy_form(random_store):
    Cm = _count_matrix(random_store)
    K = len(random_store)
    for k in range(K):
        c = Connections()
        c.update(random_store, k)
        row = Cm[k]
        if not row.any():
            assert c.W[k] == {} and c.ordered[k] == []
            continue
        T = np.nonzero(row >= THRESHOLD)[0]
        if len(T) == 0:
            T = np.array([int(np.argmax(row))])          # argmax: the first of the largest
        order = sorted(T, key=lambda j: (-row[j], -j))   # weight descending, number descending
        assert c.ordered[k] == [int(j) for j in order] and c.weights[k] == [int(row[j]) for j in order]
        assert c.W[k] == {j: int(row[j]) for j in range(K) if row[j] > 0}
        for j in range(K):
            if j != k:   # on fresh state a neighbour knows k alone
                assert c.W[j] == ({k: int(row[j])} if j in T else {}) and c.ordered[j] == ([k] if j in T else [])
        assert c.parent[k] == (int(order[0]) if k != 0 else -1) and c.first_connect[k] == (k == 0)
        assert all(c.children[j] == ({k} if k != 0 and j == order[0] else set()) for j in range(K))


@pytest.mark.parametrize("case", ci.hand_cases(), ids=lambda c: c["name"])
def test_hand_made_case_on_the_model(case):
    _, snap = ci.run_model(case["store"], case["script"])
    assert case["check"](snap)


def test_header_declares_and_binding_lists_the_new_symbols(vo):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "vo_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(vo_[a-z0-9_]+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(vo.SYMBOLS)
    assert all(hasattr(vo.lib(), s) for s in NEW_SYMBOLS)
    assert re.search(r"#define\s+VO_KFSTORE_CONNECTIONS_MAX_KEYFRAMES\s+4096\b", text)
    assert (vo.KeyFrameStore.CONNECTIONS_INVALID, vo.KeyFrameStore.CONNECTIONS_CAPACITY) == (1, 2)


def test_null_handles_are_rejected(vo):
    L = vo.lib()
    w = C.c_int32(0)
    assert L.vo_kfstore_enable_connections(None) == -1
    assert L.vo_kfstore_update_connections(None, 0, None) == -1
    assert L.vo_kfstore_update_connections_dev(None, 0, None) == -1
    assert L.vo_kfstore_connections_status(None, C.byref(w)) == -1
    assert L.vo_kfstore_get_connections(None, 0, None, None, None, None, None, None, None, None) == -1
