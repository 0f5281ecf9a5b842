# Compiles, from the reference checkout, what tests/test_shims_vs_reference.py checks the C++ shims against, into _ref/
# (git-ignored; nothing of the reference is copied into the repository):
#   _ref/myslam_decls.h.gch  the reference's class declarations (include/myslam/*.h), with include/myslam_shim/ORBextractor.h
#                            in place of its own ORBextractor.h (tests/shim_stubs/override/) and declaration-only stand-ins
#                            for the third-party headers (tests/shim_stubs/thirdparty/), as a precompiled header
#   _ref/<caller>.o          the reference's callers src/{visualOdometry,localMapping,loopClosing}.cpp, unchanged, compiled
#                            against the same headers
# Whatever does not compile leaves the compiler's output in _ref/<name>.log for the test to show.  Without the reference
# checkout nothing is built.
#   make -C oracle -f reference.mk [REFERENCE=<reference checkout>]
REFERENCE ?= /root/reference
CXX ?= g++
STUBS = ../tests/shim_stubs
INC = -I$(STUBS)/override -I$(REFERENCE)/include -I$(STUBS)/thirdparty -I../include
# gnu++14 like the reference's own build
CXXFLAGS_REF = -std=gnu++14
HEADERS = common_include.h camera.h frame.h keyframe.h mappoint.h map.h matcher.h optimizer_ceres.h sim3Solver.h \
          localMapping.h loopClosing.h visualOdometry.h
CALLERS = visualOdometry localMapping loopClosing
DEPS = reference.mk $(wildcard ../include/*.h ../include/myslam_shim/* $(STUBS)/override/myslam/* $(STUBS)/thirdparty/*/* \
                                $(STUBS)/thirdparty/*/*/* $(REFERENCE)/include/myslam/*.h)

ifeq ($(wildcard $(REFERENCE)/include/myslam/matcher.h),)
all:
	@echo "reference.mk: no reference checkout at $(REFERENCE), nothing to build"
else
all: _ref/myslam_decls.h.gch $(CALLERS:%=_ref/%.o)
endif

_ref/myslam_decls.h.gch: $(DEPS)
	mkdir -p _ref
	printf '#include "myslam/%s"\n' $(HEADERS) > _ref/myslam_decls.h
	$(CXX) $(CXXFLAGS_REF) $(INC) -x c++-header _ref/myslam_decls.h -o $@ > _ref/myslam_decls.log 2>&1 || { rm -f $@; exit 1; }

_ref/%.o: $(REFERENCE)/src/%.cpp $(DEPS)
	mkdir -p _ref
	$(CXX) $(CXXFLAGS_REF) $(INC) -c $< -o $@ > _ref/$*.log 2>&1 || { rm -f $@; exit 1; }

clean:
	rm -rf _ref

.PHONY: all clean
