# TEST INFRASTRUCTURE: host (g++) build of the verdict cache's feed (csrc/vjournal.h and the insert pass of
# csrc/vcache.h): the model of tests/test_vcache_feed_cpu.py and tests/test_gpu_vcache_feed.py
# (tests/vcache_feed_model.py builds it on demand).
#   make -f vcache_feed.mk
CXX ?= g++
CSRC = ../../stellar-core_amd/csrc
all: libvcachefeedcore.so
libvcachefeedcore.so: vcache_feed_core.cpp $(CSRC)/vcache.h $(CSRC)/vjournal.h $(CSRC)/sv_common.h
	$(CXX) -O2 -std=c++17 -fPIC -shared -Wall -Wextra -Wno-unknown-pragmas -o $@ vcache_feed_core.cpp -lpthread
clean:
	rm -f libvcachefeedcore.so
.PHONY: all clean
