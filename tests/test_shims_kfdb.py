"""Boundary compile check of include/myslam_shim/keyframe_db_hip.inl: parsed by g++ -fsyntax-only in a translation unit of
its own (tests/shim_stubs_kfdb/), against the stubs of tests/shim_stubs/ and one overriding header for the members of
KeyFrame / Map that those stubs do not declare."""
import pathlib
import shutil
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent
STUBS = ROOT / "tests" / "shim_stubs"
OWN = ROOT / "tests" / "shim_stubs_kfdb"


def test_keyframe_db_shim_parses():
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    r = subprocess.run([gxx, "-std=gnu++14", "-fsyntax-only", "-Wall", "-Werror", f"-I{OWN}", f"-I{STUBS}", f"-I{STUBS / 'thirdparty'}",
                        f"-I{ROOT / 'include'}", str(OWN / "tu_keyframe_db.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

