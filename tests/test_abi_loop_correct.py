"""CPU test of the drop-in boundary of the loop-correction layer, in the manner of tests/test_abi_kfstore.py:
its symbols are declared in include/vo_hip.h with the argument counts the binding calls them with, listed in the binding and
exported by the library; its record and its sticky bit match the binding and the model; its sources are in the build list."""
import re

import test_abi_kfstore as abi

SYMBOLS = {
    "vo_kfstore_enable_loop_correct": 4, "vo_kfstore_propagate_loop": 3, "vo_kfstore_propagate_loop_dev": 3, "vo_kfstore_propagate_loop_sim3": 1,
    "vo_kfstore_loop_connections": 1, "vo_kfstore_loop_correct_result": 10, "vo_kfstore_loop_correct_arrays": 8,
}


def test_symbols_are_declared_with_their_argument_counts():
    decl = abi._declarations()
    assert {name: decl.get(name) for name in SYMBOLS} == SYMBOLS


def test_symbols_are_listed_and_exported(vo):
    assert set(SYMBOLS) <= set(vo.SYMBOLS)
    assert set(SYMBOLS) <= abi._exported(vo)


def test_record_and_sticky_bit_match_the_binding_and_the_model(vo):
    import loop_correct_ref as ref
    S = vo.KeyFrameStore
    assert S.LC_RECORD == ref.LC_RECORD and ref.ACCEPTED == S.LOOP_ACCEPTED
    want = int(re.search(r"#define VO_KFSTORE_CORRECT_LOOP_CAPACITY (\d+)", abi.HEADER.read_text()).group(1))
    assert want == 256 == S.CONNECTIONS_CORRECT_LOOP_CAPACITY == ref.STICKY_LC_CAPACITY
    # the sticky bits below are taken: 1, 2, 4, 8, 16, 32, 64, 128
    assert (ref.OK, ref.EMPTY, ref.OVERFLOW) == (S.BA_WINDOW_OK, S.BA_WINDOW_EMPTY, S.BA_WINDOW_OVERFLOW)


def test_the_sources_are_in_the_build_list():
    from vo_slam_test_amd import build
    assert ("loop_correct.hip", ["-ffp-contract=off"]) in build.SOURCES
    assert all((build.CSRC / name).exists() for name in ("loop_correct.hip", "sim3_compose.h", "refresh_point.h", "obs_walk.h", "new_points_geom.h"))
