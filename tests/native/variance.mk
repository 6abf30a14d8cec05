# Test-only host build of the variance accumulation (pt_variance.hpp) and the denoiser's variance term
# (pt_denoise.hpp) for tests/test_variance_host.py: libdenoise.so's flags (denoise.mk), no GPU code is run.
# make -f variance.mk
HIPCC ?= /opt/rocm/bin/hipcc
CSRC = ../../rs-pathtracing_amd/csrc
HFLAGS = -O2 -std=c++17 -fPIC -shared -ffp-contract=off -x hip --offload-arch=gfx950 --offload-host-only

all: _build/libvariance.so

_build/libvariance.so: variance_harness.cpp $(CSRC)/pt_variance.hpp $(CSRC)/pt_denoise.hpp
	@mkdir -p _build
	$(HIPCC) $(HFLAGS) -o $@ variance_harness.cpp

.PHONY: all
