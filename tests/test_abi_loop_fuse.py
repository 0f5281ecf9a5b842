"""CPU test of the drop-in boundary of the loop-fusion layer, in the manner of tests/test_abi_kfstore.py:
its symbols are declared in include/vo_hip.h with the argument counts the binding calls them with, listed in the binding and
exported by the library; its columns match the binding and the model; its sources are in the build list."""
import test_abi_kfstore as abi

SYMBOLS = {
    "vo_kfstore_enable_loop_fuse": 3, "vo_kfstore_search_and_fuse": 7, "vo_kfstore_search_and_fuse_dev": 7,
    "vo_kfstore_search_and_fuse_loop": 5, "vo_kfstore_loop_fuse_result": 3,
}


def test_symbols_are_declared_with_their_argument_counts():
    decl = abi._declarations()
    assert {name: decl.get(name) for name in SYMBOLS} == SYMBOLS


def test_symbols_are_listed_and_exported(vo):
    assert set(SYMBOLS) <= set(vo.SYMBOLS)
    assert set(SYMBOLS) <= abi._exported(vo)


def test_columns_match_the_binding_and_the_model(vo):
    import loop_fuse_ref
    assert vo.KeyFrameStore.LOOP_FUSE_COLUMNS == loop_fuse_ref.PASS and len(loop_fuse_ref.PASS) == 6
    assert loop_fuse_ref.ACCEPTED == vo.KeyFrameStore.LOOP_ACCEPTED


def test_the_sources_are_in_the_build_list():
    from vo_slam_test_amd import build
    assert ("loop_fuse.hip", ["-ffp-contract=off"]) in build.SOURCES
    assert all((build.CSRC / name).exists() for name in ("loop_fuse.hip", "fuse_ops.h", "sim3_compose.h", "kf_area.h"))
