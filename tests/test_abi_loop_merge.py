"""CPU test of the drop-in boundary of the loop-merge layer, in the manner of tests/test_abi_kfstore.py: its
symbols are declared in include/vo_hip.h with the argument counts the binding calls them with, listed in the binding and exported
by the library; its records match the binding and the model; its source is in the build list."""
import test_abi_kfstore as abi

SYMBOLS = {
    "vo_kfstore_enable_loop_merge": 1, "vo_kfstore_merge_loop_matches": 4, "vo_kfstore_merge_loop_matches_dev": 4,
    "vo_kfstore_merge_loop_matches_loop": 1, "vo_kfstore_loop_merge_result": 3, "vo_kfstore_correct_loop": 5,
}


def test_symbols_are_declared_with_their_argument_counts():
    decl = abi._declarations()
    assert {name: decl.get(name) for name in SYMBOLS} == SYMBOLS


def test_symbols_are_listed_and_exported(vo):
    assert set(SYMBOLS) <= set(vo.SYMBOLS)
    assert set(SYMBOLS) <= abi._exported(vo)


def test_records_match_the_binding_and_the_model(vo):
    import loop_merge_ref as ref
    S = vo.KeyFrameStore
    assert S.LM_RECORD == ref.LM_RECORD and ref.ACCEPTED == S.LOOP_ACCEPTED and len(S.CL_RECORD) <= 16
    assert (S.LM_NONE, S.LM_ADD, S.LM_NOOP, S.LM_REPLACE, S.LM_DEAD, S.LM_UNDONE) == (ref.NONE, ref.ADD, ref.NOOP, ref.REPLACE, ref.DEAD, ref.UNDONE)
    assert (ref.STICKY_INVALID, ref.STICKY_UPKEEP, ref.STICKY_FUSE) == (S.CONNECTIONS_INVALID, S.CONNECTIONS_UPKEEP_CAPACITY, S.CONNECTIONS_FUSE_CAPACITY)
    assert ref.CARRIERS_MAX == S.FUSE_MAX_CARRIERS


def test_the_sources_are_in_the_build_list():
    from vo_slam_test_amd import build
    assert ("loop_merge.hip", ["-ffp-contract=off"]) in build.SOURCES
    assert all((build.CSRC / name).exists() for name in ("loop_merge.hip", "fuse_ops.h", "obs_walk.h", "block_sort.h"))
