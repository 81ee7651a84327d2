# TEST INFRASTRUCTURE: host (g++) build of the sharing of verdicts between slots (csrc/vshare.h over
# csrc/vjournal.h): the model of tests/test_vshare_model_cpu.py and tests/test_gpu_vcache_share.py
# (tests/vshare_model.py builds it on demand).
#   make -f vshare.mk
CXX ?= g++
CSRC = ../../stellar-core_amd/csrc
all: libvsharecore.so
libvsharecore.so: vshare_core.cpp $(CSRC)/vshare.h $(CSRC)/vjournal.h
	$(CXX) -O2 -std=c++17 -fPIC -shared -Wall -Wextra -Wno-unknown-pragmas -o $@ vshare_core.cpp -lpthread
clean:
	rm -f libvsharecore.so
.PHONY: all clean
