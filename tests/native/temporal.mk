# Test-only host build of the temporal accumulation (pt_temporal.hpp) for tests/test_temporal_host.py: libdenoise.so's
# flags (denoise.mk), no GPU code is run.  make -f temporal.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC = ../../rs-pathtracing_amd/csrc
HFLAGS = -O2 -std=c++17 -fPIC -shared -ffp-contract=off -x hip --offload-arch=gfx950 --offload-host-only

all: _build/libtemporal.so

_build/libtemporal.so: temporal_harness.cpp $(CSRC)/pt_temporal.hpp $(CSRC)/pt_denoise.hpp
	@mkdir -p _build
	$(HIPCC) $(HFLAGS) -o $@ temporal_harness.cpp

.PHONY: all
