"""CPU test of the drop-in boundary of the hand-over behind the store's relocalisation and reference-key-frame routes (DESIGN.md
section 4w), in the manner of tests/test_abi_motion_store.py: its two symbols are declared in include/vo_hip.h with the argument
counts the binding calls them with, listed in the binding and exported by the library; the selectors before it keep their
numbers and the one it adds continues them; its source is in the build list with its flag."""
import re

import test_abi_kfstore as abi

SYMBOLS = {"vo_tracker_end_frame_store": 3, "vo_tracker_point_stats_store": 2}


def test_symbols_are_declared_with_their_argument_counts():
    text = re.sub(r"/\*.*?\*/", "", abi.HEADER.read_text(), flags=re.S)
    decl = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\bint\s+(vo_tracker_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)}
    assert {name: decl.get(name) for name in SYMBOLS} == SYMBOLS
    assert decl["vo_tracker_end_frame"] == 2 and decl["vo_tracker_point_stats"] == 1      # the calls they stand beside keep their signatures


def test_symbols_are_listed_and_exported(vo):
    assert set(SYMBOLS) <= set(vo.SYMBOLS) and set(SYMBOLS) <= abi._exported(vo)
    assert all(hasattr(vo.Tracker, m) for m in ("end_frame_store", "point_stats_store"))


def test_existing_selectors_keep_their_numbers(vo):
    enum = {k: int(v) for k, v in re.findall(r"VO_TRACKER_(\w+) = (\d+)", abi.HEADER.read_text())}
    assert enum["ASSIGNED_LAST"] == 0 and enum["FEATURE_OUTLIER"] == 14 and enum["RELOC_POINT_IDS"] == 16 and enum["SLOT_IDS"] == 36
    assert enum["TCW_START"] == 49 and enum["FIRST_SLOT_IDS"] == 50 and enum["REF_KF"] == 55
    assert enum["FEATURE_OBSERVED"] == 56 and vo.Tracker.FEATURE_OBSERVED == 56           # the one new selector continues from 56
    assert all(getattr(vo.Tracker, n) == enum[n] for n in enum if hasattr(vo.Tracker, n))
    assert set(range(57)) <= set(enum.values())                                            # no number of the enumeration is left out


def test_the_source_is_in_the_build_list():
    from vo_slam_test_amd import build
    assert ("handover_store.hip", ["-ffp-contract=off"]) in build.SOURCES
    assert all((build.CSRC / name).exists() for name in ("handover_store.hip", "handover_end.h", "point_stats_rows.h", "obs_walk.h"))
