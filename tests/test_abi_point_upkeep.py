"""CPU test of the drop-in boundary for vo_kfstore_enable_point_upkeep .. vo_kfstore_upkeep_result: the
symbols are declared in include/vo_hip.h with the argument counts the binding calls them with, listed in the binding and
exported by the library, and the new constants match the binding."""
import pathlib
import re
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent

ARGS = {
    "vo_kfstore_enable_point_upkeep": 2, "vo_kfstore_compute_descriptors": 3, "vo_kfstore_compute_descriptors_dev": 3,
    "vo_kfstore_process_new_keyframe": 2, "vo_kfstore_add_point_stats": 5, "vo_kfstore_add_point_stats_dev": 5,
    "vo_kfstore_cull_map_points": 2, "vo_kfstore_recent_points": 6, "vo_kfstore_upkeep_result": 3,
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


def test_constants_match_the_binding(vo):
    text = (ROOT / "include" / "vo_hip.h").read_text()
    want = {name: int(val) for name, val in re.findall(r"#define VO_KFSTORE_(UPKEEP_[A-Z_]+|DESC_MAX_HOLDERS) (\d+)", text)}
    S = vo.KeyFrameStore
    assert want == dict(UPKEEP_CAPACITY=S.CONNECTIONS_UPKEEP_CAPACITY, DESC_MAX_HOLDERS=S.DESC_MAX_HOLDERS, UPKEEP_PROCESS=S.UPKEEP_PROCESS,
                        UPKEEP_CULL=S.UPKEEP_CULL, UPKEEP_CREATED=S.UPKEEP_CREATED)
    assert want["UPKEEP_CAPACITY"] == 8 and len(S.UPKEEP_RECORD) <= 16


def test_the_source_is_in_the_build_list():
    from vo_slam_test_amd import build
    assert ("point_upkeep.hip", ["-ffp-contract=off"]) in build.SOURCES and (build.CSRC / "point_upkeep.hip").exists()
