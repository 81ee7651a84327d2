// Host environment of the engine: environment knobs, the CPUs and NUMA nodes
// this process may use, the steady clock of the traces, and the copy a pack
// task makes.  No HIP: included by host_image.h and engine_state.h
// (sv_api.cpp), and by the CPU tests (tests/native/host_core.cpp).
#pragma once

#include <emmintrin.h>
#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

// The engine's modules are the internals of the one translation unit that
// includes them (sv_api.cpp; the CPU tests' host_core.cpp for the two host
// headers): the unnamed namespace keeps them out of the library's exports
// and lets the compiler treat every function as local to that unit.
namespace sv {
namespace {

inline size_t env_size(const char* name, size_t dflt) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  char* end = nullptr;
  const unsigned long long x = strtoull(v, &end, 0);
  return (end && *end == 0) ? (size_t)x : dflt;
}

// CPUs this process may use at once: its affinity mask, limited by a cgroup
// v2 CPU quota (the GPU box grants 16 of a 256-CPU host by quota).
inline size_t usable_cpus() {
  cpu_set_t set;
  size_t aff = std::max(1u, std::thread::hardware_concurrency());
  if (sched_getaffinity(0, sizeof(set), &set) == 0) aff = (size_t)std::max(1, CPU_COUNT(&set));
  if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
    char q[32] = {0};
    unsigned long long per = 0;
    if (fscanf(f, "%31s %llu", q, &per) == 2 && std::strcmp(q, "max") != 0 && per > 0) {
      const size_t quota = (size_t)(strtoull(q, nullptr, 10) / per);
      if (quota >= 1) aff = std::min(aff, quota);
    }
    fclose(f);
  }
  return aff;
}

// NUMA node of the PCI device at `bus` ("0000:c1:00.0", any case; -1:
// unknown), and a node's CPUs this process may run on (empty: no placement).
inline int pci_numa_node(std::string bus) {
  for (char& c : bus) c = (char)tolower(c);
  int node = -1;
  if (FILE* f = fopen(("/sys/bus/pci/devices/" + bus + "/numa_node").c_str(), "r")) {
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
  }
  return node;
}
inline std::vector<int> node_cpus(int node) {
  std::vector<int> out;
  if (node < 0) return out;
  cpu_set_t mine;
  if (sched_getaffinity(0, sizeof(mine), &mine) != 0) return out;
  FILE* f = fopen(("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist").c_str(), "r");
  if (!f) return out;
  char buf[4096] = {0};
  const size_t got = fread(buf, 1, sizeof(buf) - 1, f);
  fclose(f);
  buf[got] = 0;
  // "0-23,96-119"
  for (char* p = buf; *p;) {
    char* e = nullptr;
    const long a = strtol(p, &e, 10);
    if (e == p) break;
    long b = a;
    if (*e == '-') {
      p = e + 1;
      b = strtol(p, &e, 10);
    }
    for (long c = a; c <= b && c < CPU_SETSIZE; ++c)
      if (CPU_ISSET((int)c, &mine)) out.push_back((int)c);
    p = e;
    while (*p == ',' || *p == '\n' || *p == ' ') ++p;
  }
  return out;
}
// NUMA node of the page holding p (-1: unknown): get_mempolicy(MPOL_F_NODE |
// MPOL_F_ADDR) by its syscall (no libnuma in the image).
inline int page_numa_node(const void* p) {
  if (!p) return -1;
  int node = -1;
  const long r = syscall(SYS_get_mempolicy, &node, nullptr, 0UL, p, 3UL /* MPOL_F_NODE | MPOL_F_ADDR */);
  return r == 0 ? node : -1;
}

inline int64_t now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}
// SV_STAGE_TRACE: per-call host staging timings to stderr (developer knob)
inline bool stage_trace() {
  static const bool t = getenv("SV_STAGE_TRACE") != nullptr;
  return t;
}
inline thread_local double g_trace_pack_us = 0;
// (both traces also print steady-clock microseconds, to line a bulk call's
// stages up with the latency lane's batches)
inline double trace_abs_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Bytes per helper task of a pack of at least 2 MB (SV_PACK_PART); smaller
// packs take 1 MB tasks.  With 1 MB tasks a 29k-signature batch (3.7 MB) was
// packed by 3 threads; 256 KB tasks spread it over the pool: host call 0.669-
// 0.707 -> 0.663-0.675 ms, 50k 0.88-0.92 -> 0.86-0.89 ms, while at 8k (1 MB)
// waking the pool cost 10 us (profiles/r05/host_call/pack_part/).
inline size_t pack_part() {
  static const size_t v = std::max<size_t>(4096, env_size("SV_PACK_PART", 1u << 18));
  return v;
}
// Pack stores bypass the CPU caches (SV_PACK_NT, default on): the pinned
// image is read by the GPU (DMA or in place), never again by the CPU, and a
// cached store first reads each destination line.  Measured on the GPU box's
// host, 128 MB copies: 16 threads 107 -> 180 GB/s, 8 threads 90 -> 127 GB/s
// (tools/nt_copy_probe.cpp, profiles/r06/feed/nt_copy_probe.txt).
inline bool pack_nt() {
  static const bool b = env_size("SV_PACK_NT", 1) != 0;
  return b;
}
// dst 16-byte aligned (else memcpy); the caller fences (_mm_sfence) before
// the data is handed to the device.
inline void nt_copy(uint8_t* dst, const uint8_t* src, size_t n) {
  if (((uintptr_t)dst & 15u) != 0) {
    std::memcpy(dst, src, n);
    return;
  }
  size_t i = 0;
  for (; i + 64 <= n; i += 64) {
    const __m128i a = _mm_loadu_si128((const __m128i*)(src + i));
    const __m128i b = _mm_loadu_si128((const __m128i*)(src + i + 16));
    const __m128i c = _mm_loadu_si128((const __m128i*)(src + i + 32));
    const __m128i d = _mm_loadu_si128((const __m128i*)(src + i + 48));
    _mm_stream_si128((__m128i*)(dst + i), a);
    _mm_stream_si128((__m128i*)(dst + i + 16), b);
    _mm_stream_si128((__m128i*)(dst + i + 32), c);
    _mm_stream_si128((__m128i*)(dst + i + 48), d);
  }
  for (; i + 16 <= n; i += 16) _mm_stream_si128((__m128i*)(dst + i), _mm_loadu_si128((const __m128i*)(src + i)));
  if (i < n) std::memcpy(dst + i, src + i, n - i);
}
// The copy of one pack task: streaming stores with SV_PACK_NT, fenced when
// the task ends (its stores are then ordered before its completion, which the
// pool publishes under a mutex, and so before the upload).
struct PackCopy {
  const bool nt = pack_nt();
  void operator()(uint8_t* d, const uint8_t* s, size_t k) const {
    if (nt) nt_copy(d, s, k);
    else std::memcpy(d, s, k);
  }
  ~PackCopy() {
    if (nt) _mm_sfence();
  }
};
// Helper tasks of a pack of `work` bytes at `part` bytes per task, on a pool
// of `threads` helpers (the caller packs too); cap != 0: at most that many.
inline size_t pack_parts(size_t threads, size_t cap, size_t work, size_t part) {
  return std::max<size_t>(1, std::min<size_t>(std::min(threads + 1, cap ? cap : threads + 1), work / part));
}

}  // namespace
}  // namespace sv
