"""CPU test of the drop-in boundary of the hand-over, in the manner of tests/test_abi_kfstore.py: its
symbols are declared in include/vo_hip.h with the argument counts the binding calls them with, listed in the binding and
exported by the library; its selectors keep the old numbers and match the binding; its source is in the build list."""
import ctypes as C
import re

import test_abi_kfstore as abi

SYMBOLS = {"vo_tracker_set_last_frame_ids": 3, "vo_tracker_set_last_pose": 3, "vo_tracker_end_frame": 2, "vo_tracker_begin_frame": 3,
           "vo_tracker_handover_arrays": 4}
SELECTORS = ("SLOT_IDS", "SLOT_DESC", "FRAME_POSE", "VELOCITY", "MOTION_STATE", "TEMP_COUNT", "LAST_POINTS", "LAST_FLAGS", "LAST_OCTAVE",
             "LAST_ANGLE", "LAST_DESC", "LAST_IDS", "LAST_N", "TCW_START")


def test_symbols_are_declared_with_their_argument_counts():
    text = re.sub(r"/\*.*?\*/", "", abi.HEADER.read_text(), flags=re.S)
    decl = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\bint\s+(vo_tracker_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}
    assert {name: decl.get(name) for name in SYMBOLS} == SYMBOLS


def test_symbols_are_listed_and_exported(vo):
    assert set(SYMBOLS) <= set(vo.SYMBOLS) and set(SYMBOLS) <= abi._exported(vo)


def test_selectors_follow_pose_start_and_match_the_binding(vo):
    enum = {k: int(v) for k, v in re.findall(r"VO_TRACKER_(\w+) = (\d+)", abi.HEADER.read_text())}
    assert enum["ASSIGNED_LAST"] == 0 and enum["POSE_START"] == 35           # existing values keep their numbers
    assert [enum[n] for n in SELECTORS] == list(range(36, 36 + len(SELECTORS)))
    assert all(getattr(vo.Tracker, n) == enum[n] for n in enum if hasattr(vo.Tracker, n)) and all(hasattr(vo.Tracker, n) for n in SELECTORS)
    assert C.sizeof(vo.HandoverParams) == 8 and [f[0] for f in vo.HandoverParams._fields_] == ["th_depth", "min_tracked"]


def test_the_sources_are_in_the_build_list():
    from vo_slam_test_amd import build
    assert ("handover.hip", ["-ffp-contract=off"]) in build.SOURCES
    assert all((build.CSRC / name).exists() for name in ("handover.hip", "handover_geom.h", "tracker_state.h"))
