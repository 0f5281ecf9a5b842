"""CPU test of the drop-in boundary for vo_kfstore_enable_fuse .. vo_kfstore_fuse_result: the symbols are
declared in include/vo_hip.h with the argument counts the binding calls them with, listed in the binding and exported by the
library, and the new constants match the binding."""
import pathlib
import re
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent

ARGS = {
    "vo_kfstore_enable_fuse": 3, "vo_kfstore_fuse_map_points": 5, "vo_kfstore_fuse_map_points_dev": 5,
    "vo_kfstore_search_in_neighbors": 2, "vo_kfstore_fuse_result": 4,
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
    import fuse_ref
    text = (ROOT / "include" / "vo_hip.h").read_text()
    want = {name: int(val) for name, val in re.findall(r"#define VO_KFSTORE_(FUSE_[A-Z_]+) (\d+)", text)}
    S = vo.KeyFrameStore
    assert want == dict(FUSE_CAPACITY=S.CONNECTIONS_FUSE_CAPACITY, FUSE_MAX_CARRIERS=S.FUSE_MAX_CARRIERS, FUSE_MAX_STEPS=S.FUSE_MAX_STEPS)
    assert want["FUSE_CAPACITY"] == 16 == fuse_ref.STICKY_FUSE and want["FUSE_MAX_CARRIERS"] == fuse_ref.CARRIERS_MAX
    assert want["FUSE_MAX_STEPS"] == fuse_ref.MAX_TARGETS + 1 and S.FUSE_COLUMNS == fuse_ref.STEP


def test_the_source_is_in_the_build_list():
    from vo_slam_test_amd import build
    assert ("fuse.hip", ["-ffp-contract=off"]) in build.SOURCES and (build.CSRC / "fuse.hip").exists()
