"""CPU test of the drop-in boundary for vo_kfstore_enable_mapping .. vo_kfstore_get_points: the symbols
are declared in include/vo_hip.h with the argument counts the binding calls them with, listed in the binding and exported by
the library."""
import pathlib
import re
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent

ARGS = {
    "vo_kfstore_enable_mapping": 5, "vo_kfstore_set_pose": 3, "vo_kfstore_set_pose_dev": 3, "vo_kfstore_set_keypoint_xy": 3,
    "vo_kfstore_set_keypoint_xy_dev": 3, "vo_kfstore_next_point_id": 2, "vo_kfstore_create_map_points": 3,
    "vo_kfstore_new_points_result": 8, "vo_kfstore_get_points": 9,
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


def test_status_constants_match_the_binding(vo):
    text = (ROOT / "include" / "vo_hip.h").read_text()
    want = {name: int(val) for name, val in re.findall(r"#define VO_KFSTORE_(NP_[A-Z_]+) (\d+)", text)}
    assert want == {name: getattr(vo.KeyFrameStore, name) for name in ("NP_SEARCHED", "NP_SKIPPED_BAD", "NP_SKIPPED_BASELINE",
                                                                      "NP_SKIPPED_NO_POSE", "NP_NOT_REACHED")}
