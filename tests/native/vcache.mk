# TEST INFRASTRUCTURE: host (g++) build of the verdict cache's policy (csrc/vcache.h): the model of
# tests/test_vcache_cpu.py and tests/test_gpu_vcache.py (tests/vcache_model.py builds it on demand).
#   make -f vcache.mk
CXX ?= g++
CSRC = ../../stellar-core_amd/csrc
all: libvcachecore.so
libvcachecore.so: vcache_core.cpp $(CSRC)/vcache.h $(CSRC)/sv_common.h
	$(CXX) -O2 -std=c++17 -fPIC -shared -Wall -Wextra -Wno-unknown-pragmas -o $@ vcache_core.cpp
clean:
	rm -f libvcachecore.so
.PHONY: all clean
