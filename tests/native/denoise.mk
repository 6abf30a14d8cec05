# Test-only host build of the guided denoiser (pt_denoise.hpp) for tests/test_denoise_host.py: libaov.so's flags
# (aov.mk), no GPU code is run.  make -f denoise.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC = ../../rs-pathtracing_amd/csrc
HFLAGS = -O2 -std=c++17 -fPIC -shared -ffp-contract=off -x hip --offload-arch=gfx950 --offload-host-only

all: _build/libdenoise.so

_build/libdenoise.so: denoise_harness.cpp $(CSRC)/pt_denoise.hpp
	@mkdir -p _build
	$(HIPCC) $(HFLAGS) -o $@ denoise_harness.cpp

.PHONY: all
