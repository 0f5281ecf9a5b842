"""The drop-in claim checked against the reference's OWN declarations.  build() compiles them from the reference checkout
(oracle/reference.mk, into the git-ignored oracle/_ref/; skipped where no build found the checkout):
  * the reference's real include/myslam/*.h (frame.h, keyframe.h, mappoint.h, map.h, matcher.h, optimizer_ceres.h,
    sim3Solver.h, ...) as a precompiled header, which every shim of include/myslam_shim/*.inl is parsed against here, and
  * the reference's callers src/visualOdometry.cpp, src/localMapping.cpp and src/loopClosing.cpp, unchanged, compiled
    against myslam_shim/ORBextractor.h in place of the reference's ORBextractor.h (tests/shim_stubs/override/),
with declaration-only stand-ins for the THIRD-PARTY headers only (Eigen, OpenCV, Sophus, DBoW3, Ceres, Pangolin:
tests/shim_stubs/thirdparty/).  Nothing of the reference is copied into the repository."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
STUBS = ROOT / "tests" / "shim_stubs"
REF_BUILD = ROOT / "oracle" / "_ref"
DECLS = REF_BUILD / "myslam_decls.h"   # written by oracle/reference.mk whenever it found the reference checkout

pytestmark = pytest.mark.skipif(not DECLS.exists(), reason="build() found no reference checkout: oracle/_ref/ holds nothing to check against")


def _log(name):
    f = REF_BUILD / f"{name}.log"
    return f.read_text()[-3000:] if f.exists() else f"no {f.name}"


def _gxx(args, **kw):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    pch = REF_BUILD / "myslam_decls.h.gch"
    assert pch.exists(), "the reference's headers did not compile with the third-party stubs:\n" + _log("myslam_decls")
    # gnu++14 like the reference's own build; the declarations come from the precompiled header only
    return subprocess.run([gxx, "-std=gnu++14", "-fsyntax-only", "-Winvalid-pch", f"-I{STUBS / 'override'}", f"-I{STUBS / 'thirdparty'}",
                           f"-I{ROOT / 'include'}", "-include", str(DECLS), *args], capture_output=True, text=True, **kw)


def test_reference_headers_parse_with_third_party_stubs_only():
    r = _gxx(["-x", "c++", "-"], input="int main() { return 0; }\n")
    assert r.returncode == 0 and "invalid" not in r.stderr, r.stderr[-3000:]


@pytest.mark.parametrize("shim", ["frame", "mappoint", "matcher", "optimizer", "sim3solver", "localmapping", "map"])
def test_shim_parses_against_the_reference_headers(shim):
    """the member definitions of the shim must match the reference's own class declarations (names, signatures,
    constness, the members they read and write)"""
    r = _gxx(["-x", "c++", "-"], input=f'#include "myslam_shim/{shim}_hip.inl"\n')
    assert r.returncode == 0 and "invalid" not in r.stderr, r.stderr[-3000:]


def test_shim_extractor_header_replaces_the_reference_one():
    """every member the reference's own header declares (and its callers use) is declared by the shim header"""
    src = '#include "myslam/ORBextractor.h"\n' \
          "void f(ORB_SLAM2::ORBextractor &e, cv::Mat im, std::vector<cv::KeyPoint> &k, cv::Mat &d) {\n" \
          "  e(im, cv::Mat(), k, d); (void)e.GetLevels(); (void)e.GetScaleFactor(); (void)e.GetScaleFactors();\n" \
          "  (void)e.GetInverseScaleFactors(); (void)e.mvImagePyramid.size(); }\n"
    r = _gxx(["-x", "c++", "-"], input=src)
    assert r.returncode == 0 and "invalid" not in r.stderr, r.stderr[-3000:]


@pytest.mark.parametrize("caller", ["visualOdometry.cpp", "localMapping.cpp", "loopClosing.cpp"])
def test_reference_callers_parse_unchanged(caller):
    """`visualOdometry.cpp and localMapping.cpp drop it in unchanged` (north_star): the callers of the hot path, as they
    lie in the reference, compiled against the shim extractor header and the reference's own class declarations"""
    name = caller[:-len(".cpp")]
    obj = REF_BUILD / f"{name}.o"
    assert obj.exists(), f"{caller} did not compile against the shims:\n" + _log(name)
