# Test-only host build of adaptive sampling's per-tile error and stop rule (pt_adaptive.hpp) for
# tests/test_adaptive_host.py: libvariance.so's flags (variance.mk), no GPU code is run.
# make -f adaptive.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC = ../../rs-pathtracing_amd/csrc
HFLAGS = -O2 -std=c++17 -fPIC -shared -ffp-contract=off -x hip --offload-arch=gfx950 --offload-host-only

all: _build/libadaptive.so

_build/libadaptive.so: adaptive_harness.cpp $(CSRC)/pt_adaptive.hpp $(CSRC)/pt_device.hpp $(CSRC)/pt_types.hpp $(CSRC)/pt_dims.hpp
	@mkdir -p _build
	$(HIPCC) $(HFLAGS) -o $@ adaptive_harness.cpp

.PHONY: all
