"""CPU test of the drop-in boundary for vo_kfstore_enable_pose_graph .. vo_kfstore_pose_graph: the symbols
are declared in include/vo_hip.h with the argument counts the binding calls them with, listed in the binding and exported by
the library, and the new constants match the binding and the model."""
import pathlib
import re
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent

ARGS = {
    "vo_kfstore_enable_pose_graph": 4, "vo_kfstore_add_loop_edge": 3, "vo_kfstore_get_loop_edges": 4,
    "vo_kfstore_pose_graph_window": 12, "vo_kfstore_pose_graph_window_dev": 13, "vo_kfstore_pose_graph_window_result": 11,
    "vo_kfstore_pose_graph_apply": 3, "vo_kfstore_pose_graph": 14,
}


def _declarations():
    text = (ROOT / "include" / "vo_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\bint\s+(vo_kfstore_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def test_new_symbols_are_declared_with_their_argument_counts():
    decl = _declarations()
    assert {name: decl.get(name) for name in ARGS} == ARGS


def test_new_symbols_are_listed_and_exported(vo):
    assert set(ARGS) <= set(vo.SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", str(vo.SO)], capture_output=True, text=True).stdout
    assert set(ARGS) <= set(re.findall(r" T (vo_[a-z0-9_]+)", out))


def test_constants_match_the_binding_and_the_model(vo):
    import pose_graph_store_ref as pr
    text = (ROOT / "include" / "vo_hip.h").read_text()
    want = {name: int(val) for name, val in re.findall(r"#define VO_KFSTORE_(MAX_LOOP_EDGES|POSE_GRAPH_CAPACITY) (\d+)", text)}
    S = vo.KeyFrameStore
    assert want == dict(MAX_LOOP_EDGES=S.MAX_LOOP_EDGES, POSE_GRAPH_CAPACITY=S.CONNECTIONS_POSE_GRAPH_CAPACITY)
    assert want == dict(MAX_LOOP_EDGES=pr.MAX_LOOP_EDGES, POSE_GRAPH_CAPACITY=pr.STICKY_PG_CAPACITY)
    assert S.POSE_GRAPH_MAX_NODES == pr.MAX_NODES == 4096 // 6 + 1 and S.PG_RECORD == pr.PG_RECORD
    others = {int(v) for v in re.findall(r"#define VO_KFSTORE_(?:CONNECTIONS_INVALID|CONNECTIONS_CAPACITY|LOCAL_BA_CAPACITY|UPKEEP_CAPACITY|"
                                         r"FUSE_CAPACITY|LOOP_RAND_SHORT|LOOP_CAPACITY) (\d+)", text)}
    assert want["POSE_GRAPH_CAPACITY"] not in others and len(others) == 7   # a bit of its own in the sticky word


def test_the_sources_are_in_the_build_list():
    from vo_slam_test_amd import build
    assert ("pose_graph_store.hip", ["-ffp-contract=off"]) in build.SOURCES
    assert (build.CSRC / "pose_graph_store.hip").exists() and (build.CSRC / "sim3_compose.h").exists()
