# TEST INFRASTRUCTURE: csrc/sign_core.h built for the host (tests/test_sign_cpu.py) and as a gfx950 probe with the
# flags of the product's kernel objects (tests/test_gpu_sign.py).
#   make -f sign.mk
CXX ?= g++
HIPCC ?= /opt/rocm/bin/hipcc
CSRC = ../../stellar-core_amd/csrc
all: libsigncore.so libsignprobe.so
libsigncore.so: sign_core.cpp $(CSRC)/*.h
	$(CXX) -O2 -std=c++17 -fPIC -shared -Wno-unknown-pragmas -I$(CSRC) -o $@ sign_core.cpp -lpthread
libsignprobe.so: sign_probe.hip $(CSRC)/*.h
	$(HIPCC) -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I$(CSRC) -shared -o $@ sign_probe.hip -Wl,-rpath,/opt/rocm/lib
clean:
	rm -f libsigncore.so libsignprobe.so
.PHONY: all clean
