"""CPU test of the drop-in boundary of the loop-detection layer, in the manner of tests/test_abi_kfstore.py:
its symbols are declared in include/vo_hip.h with the argument counts the binding calls them with, listed in the binding and
exported by the library; its records and constants match the binding and the model; its source is in the build list."""
import test_abi_kfstore as abi

SYMBOLS = {
    "vo_kfstore_enable_detect_loop": 3, "vo_kfstore_detect_loop": 4, "vo_kfstore_detect_loop_result": 4, "vo_kfstore_detect_loop_groups": 4,
    "vo_kfstore_compute_sim3_detected": 6, "vo_kfstore_compute_sim3_detected_dev": 6, "vo_kfstore_release_loop_locks": 1,
    "vo_kfstore_loop_locks_result": 4, "vo_kfstore_set_last_loop_keyframe": 2, "vo_kfstore_get_last_loop_keyframe": 2,
    "vo_kfstore_loop_closing_step": 12,
}


def test_symbols_are_declared_with_their_argument_counts():
    decl = abi._declarations()
    assert {name: decl.get(name) for name in SYMBOLS} == SYMBOLS


def test_symbols_are_listed_and_exported(vo):
    names = set(SYMBOLS) | {"vo_kfdb_get_neighbors"}
    assert names <= set(vo.SYMBOLS)
    assert names <= abi._exported(vo)
    assert "int vo_kfdb_get_neighbors(vo_kfdb *db, int keyframe, int32_t *n, int32_t *ids" in abi.HEADER.read_text()


def test_records_and_constants_match_the_binding_and_the_model(vo):
    import re

    import detect_loop_ref as ref
    S = vo.KeyFrameStore
    assert S.DL_RECORD == ref.DL_RECORD and len(S.DL_RECORD) <= 16 and len(S.LCS_RECORD) <= 16
    assert (S.DETECT_NONE, S.DETECT_GATED, S.DETECT_NO_CANDIDATES, S.DETECT_NOT_CONSISTENT, S.DETECT_DETECTED, S.DETECT_OVERFLOW) == \
        (ref.NONE, ref.GATED, ref.NO_CANDIDATES, ref.NOT_CONSISTENT, ref.DETECTED, ref.OVERFLOW)
    assert (ref.UNDECIDED, ref.NO_MATCH, ref.REJECTED, ref.ACCEPTED) == (0, 1, 2, S.LOOP_ACCEPTED)
    assert (ref.STICKY_INVALID, ref.STICKY_DETECT_CAPACITY) == (S.CONNECTIONS_INVALID, S.CONNECTIONS_DETECT_CAPACITY)
    header = abi.HEADER.read_text()
    defines = dict(re.findall(r"#define (VO_KFSTORE_DETECT_\w+) (\d+)", header))
    assert int(defines["VO_KFSTORE_DETECT_CAPACITY"]) == S.CONNECTIONS_DETECT_CAPACITY
    assert int(defines["VO_KFSTORE_DETECT_MAX_GROUPS"]) == S.DETECT_MAX_GROUPS
    assert [int(defines["VO_KFSTORE_DETECT_" + n]) for n in ("NONE", "GATED", "NO_CANDIDATES", "NOT_CONSISTENT", "DETECTED", "OVERFLOW")] == list(range(6))


def test_the_sources_are_in_the_build_list():
    from vo_slam_test_amd import build
    assert ("detect_loop.hip", ["-ffp-contract=off"]) in build.SOURCES
    assert all((build.CSRC / name).exists() for name in ("detect_loop.hip", "kfstore.h"))
