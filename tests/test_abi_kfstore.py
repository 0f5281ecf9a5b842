"""CPU test of the drop-in boundary of the key-frame store's layers (DESIGN.md sections 4j, 4l-4o): a layer's symbols are
declared in include/vo_hip.h with the argument counts the binding calls them with, listed in the binding and exported by the
library; its constants match the binding (and the model, where there is one); its source is in the build list.  And for the
store as a whole: every int vo_kfstore_*() the header declares is listed and exported."""
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "vo_hip.h"


def _new_points_constants(vo, text):
    want = {name: int(val) for name, val in re.findall(r"#define VO_KFSTORE_(NP_[A-Z_]+) (\d+)", text)}
    assert want == {name: getattr(vo.KeyFrameStore, name) for name in ("NP_SEARCHED", "NP_SKIPPED_BAD", "NP_SKIPPED_BASELINE",
                                                                      "NP_SKIPPED_NO_POSE", "NP_NOT_REACHED")}


def _point_upkeep_constants(vo, text):
    want = {name: int(val) for name, val in re.findall(r"#define VO_KFSTORE_(UPKEEP_[A-Z_]+|DESC_MAX_HOLDERS) (\d+)", text)}
    S = vo.KeyFrameStore
    assert want == dict(UPKEEP_CAPACITY=S.CONNECTIONS_UPKEEP_CAPACITY, DESC_MAX_HOLDERS=S.DESC_MAX_HOLDERS, UPKEEP_PROCESS=S.UPKEEP_PROCESS,
                        UPKEEP_CULL=S.UPKEEP_CULL, UPKEEP_CREATED=S.UPKEEP_CREATED)
    assert want["UPKEEP_CAPACITY"] == 8 and len(S.UPKEEP_RECORD) <= 16


def _fuse_constants(vo, text):
    import fuse_ref
    want = {name: int(val) for name, val in re.findall(r"#define VO_KFSTORE_(FUSE_[A-Z_]+) (\d+)", text)}
    S = vo.KeyFrameStore
    assert want == dict(FUSE_CAPACITY=S.CONNECTIONS_FUSE_CAPACITY, FUSE_MAX_CARRIERS=S.FUSE_MAX_CARRIERS, FUSE_MAX_STEPS=S.FUSE_MAX_STEPS)
    assert want["FUSE_CAPACITY"] == 16 == fuse_ref.STICKY_FUSE and want["FUSE_MAX_CARRIERS"] == fuse_ref.CARRIERS_MAX
    assert want["FUSE_MAX_STEPS"] == fuse_ref.MAX_TARGETS + 1 and S.FUSE_COLUMNS == fuse_ref.STEP


def _loop_sim3_constants(vo, text):
    import loop_sim3_ref as ref
    want = {name: int(val) for name, val in re.findall(r"#define VO_KFSTORE_(LOOP_[A-Z_]+) (\d+)", text)}
    S = vo.KeyFrameStore
    assert want == dict(LOOP_MAX_CANDIDATES=S.LOOP_MAX_CANDIDATES, LOOP_RAND_SHORT=S.CONNECTIONS_LOOP_RAND_SHORT,
                        LOOP_CAPACITY=S.CONNECTIONS_LOOP_CAPACITY, LOOP_UNDECIDED=S.LOOP_UNDECIDED, LOOP_NO_MATCH=S.LOOP_NO_MATCH,
                        LOOP_REJECTED=S.LOOP_REJECTED, LOOP_ACCEPTED=S.LOOP_ACCEPTED)
    assert (want["LOOP_MAX_CANDIDATES"], want["LOOP_RAND_SHORT"], want["LOOP_CAPACITY"]) == (16, 32, 64) == \
        (ref.MAX_CANDIDATES, ref.STICKY_RAND_SHORT, ref.STICKY_CAPACITY)
    assert (ref.UNDECIDED, ref.NO_MATCH, ref.REJECTED, ref.ACCEPTED) == (0, 1, 2, 3)
    assert S.LOOP_RECORD == ref.RECORD and S.LOOP_PER_CANDIDATE == ref.PER_CANDIDATE
    # the sticky bits below are taken: 1, 2 (connections), 4 (local BA), 8 (upkeep), 16 (fuse)
    assert {S.CONNECTIONS_INVALID, S.CONNECTIONS_CAPACITY, S.CONNECTIONS_LOCAL_BA_CAPACITY, S.CONNECTIONS_FUSE_CAPACITY} == {1, 2, 4, 16}


def _pose_graph_store_constants(vo, text):
    import pose_graph_store_ref as pr
    want = {name: int(val) for name, val in re.findall(r"#define VO_KFSTORE_(MAX_LOOP_EDGES|POSE_GRAPH_CAPACITY) (\d+)", text)}
    S = vo.KeyFrameStore
    assert want == dict(MAX_LOOP_EDGES=S.MAX_LOOP_EDGES, POSE_GRAPH_CAPACITY=S.CONNECTIONS_POSE_GRAPH_CAPACITY)
    assert want == dict(MAX_LOOP_EDGES=pr.MAX_LOOP_EDGES, POSE_GRAPH_CAPACITY=pr.STICKY_PG_CAPACITY)
    assert S.POSE_GRAPH_MAX_NODES == pr.MAX_NODES == 4096 // 6 + 1 and S.PG_RECORD == pr.PG_RECORD
    others = {int(v) for v in re.findall(r"#define VO_KFSTORE_(?:CONNECTIONS_INVALID|CONNECTIONS_CAPACITY|LOCAL_BA_CAPACITY|UPKEEP_CAPACITY|"
                                         r"FUSE_CAPACITY|LOOP_RAND_SHORT|LOOP_CAPACITY) (\d+)", text)}
    assert want["POSE_GRAPH_CAPACITY"] not in others and len(others) == 7   # a bit of its own in the sticky word


# layer -> (symbol: argument count, the constants' check, the files its build-list check names: the source first)
LAYERS = {
    "new_points": ({
        "vo_kfstore_enable_mapping": 5, "vo_kfstore_set_pose": 3, "vo_kfstore_set_pose_dev": 3, "vo_kfstore_set_keypoint_xy": 3,
        "vo_kfstore_set_keypoint_xy_dev": 3, "vo_kfstore_next_point_id": 2, "vo_kfstore_create_map_points": 3,
        "vo_kfstore_new_points_result": 8, "vo_kfstore_get_points": 9,
    }, _new_points_constants, ()),
    "point_upkeep": ({
        "vo_kfstore_enable_point_upkeep": 2, "vo_kfstore_compute_descriptors": 3, "vo_kfstore_compute_descriptors_dev": 3,
        "vo_kfstore_process_new_keyframe": 2, "vo_kfstore_add_point_stats": 5, "vo_kfstore_add_point_stats_dev": 5,
        "vo_kfstore_cull_map_points": 2, "vo_kfstore_recent_points": 6, "vo_kfstore_upkeep_result": 3,
    }, _point_upkeep_constants, ("point_upkeep.hip",)),
    "fuse": ({
        "vo_kfstore_enable_fuse": 3, "vo_kfstore_fuse_map_points": 5, "vo_kfstore_fuse_map_points_dev": 5,
        "vo_kfstore_search_in_neighbors": 2, "vo_kfstore_fuse_result": 4,
    }, _fuse_constants, ("fuse.hip",)),
    "loop_sim3": ({
        "vo_kfstore_enable_loop": 4, "vo_kfstore_compute_sim3": 9, "vo_kfstore_compute_sim3_dev": 9, "vo_kfstore_compute_sim3_continue": 2,
        "vo_kfstore_loop_result": 8, "vo_kfstore_loop_solver_inputs": 10, "vo_kfstore_loop_ransac_max_iters": 1,
    }, _loop_sim3_constants, ("loop_sim3.hip",)),
    "pose_graph_store": ({
        "vo_kfstore_enable_pose_graph": 4, "vo_kfstore_add_loop_edge": 3, "vo_kfstore_get_loop_edges": 4,
        "vo_kfstore_pose_graph_window": 12, "vo_kfstore_pose_graph_window_dev": 13, "vo_kfstore_pose_graph_window_result": 11,
        "vo_kfstore_pose_graph_apply": 3, "vo_kfstore_pose_graph": 14,
    }, _pose_graph_store_constants, ("pose_graph_store.hip", "sim3_compose.h")),
}
layers = pytest.mark.parametrize("layer", list(LAYERS))


def _declarations():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\bint\s+(vo_kfstore_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}


def _exported(vo):
    out = subprocess.run(["nm", "-D", "--defined-only", str(vo.SO)], capture_output=True, text=True).stdout
    return set(re.findall(r" T (vo_[a-z0-9_]+)", out))


@layers
def test_new_symbols_are_declared_with_their_argument_counts(layer):
    args, decl = LAYERS[layer][0], _declarations()
    assert {name: decl.get(name) for name in args} == args


@layers
def test_new_symbols_are_listed_and_exported(vo, layer):
    args = LAYERS[layer][0]
    assert set(args) <= set(vo.SYMBOLS)
    assert set(args) <= _exported(vo)


@layers
def test_constants_match_the_binding(vo, layer):
    LAYERS[layer][1](vo, HEADER.read_text())


@pytest.mark.parametrize("layer", [name for name, entry in LAYERS.items() if entry[2]])
def test_the_source_is_in_the_build_list(layer):
    from vo_slam_test_amd import build
    files = LAYERS[layer][2]
    assert (files[0], ["-ffp-contract=off"]) in build.SOURCES
    assert all((build.CSRC / name).exists() for name in files)


def test_every_declared_store_function_is_listed_and_exported(vo):
    declared = set(_declarations())
    assert len(declared) > sum(len(entry[0]) for entry in LAYERS.values())  # (the tables above cover the later layers only)
    assert declared <= set(vo.SYMBOLS)
    assert declared <= _exported(vo)
