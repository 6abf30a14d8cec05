# Test-only host build of the listed launch's host pieces (pt_adaptive.hpp: tile_list_ok, adaptive_list) for
# tests/test_tile_list_host.py: libadaptive.so's flags (adaptive.mk), no GPU code is run.
# make -f tile_list.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC = ../../rs-pathtracing_amd/csrc
HFLAGS = -O2 -std=c++17 -fPIC -shared -ffp-contract=off -x hip --offload-arch=gfx950 --offload-host-only

all: _build/libtilelist.so

_build/libtilelist.so: tile_list_harness.cpp $(CSRC)/pt_adaptive.hpp $(CSRC)/pt_device.hpp $(CSRC)/pt_types.hpp $(CSRC)/pt_dims.hpp
	@mkdir -p _build
	$(HIPCC) $(HFLAGS) -o $@ tile_list_harness.cpp

.PHONY: all
