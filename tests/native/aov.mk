# Test-only host build of the guide-plane pass (pt_aov.hpp) for tests/test_aov_host.py: libpath.so's flags
# (Makefile), no GPU code is run.  make -f aov.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC = ../../rs-pathtracing_amd/csrc
HFLAGS = -O2 -std=c++17 -fPIC -shared -ffp-contract=off -x hip --offload-arch=gfx950 --offload-host-only
DEPS = $(wildcard $(CSRC)/*.hpp) $(CSRC)/pt_scene.cpp $(CSRC)/pt_accel.cpp

all: _build/libaov.so

_build/libaov.so: aov_harness.cpp $(DEPS)
	@mkdir -p _build
	$(HIPCC) $(HFLAGS) -o $@ aov_harness.cpp $(CSRC)/pt_scene.cpp $(CSRC)/pt_accel.cpp

.PHONY: all
