// A fake of the HIP runtime header for tests/test_devbuf_cpu.py: hipMalloc / hipFree and hipHostMalloc / hipHostFree on the host
// heap that count what they do (in the same counters) and can be told to fail the k-th allocation from now.
#pragma once
#include <cstddef>
#include <cstdlib>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };

struct FakeHip {
  long live = 0, mallocs = 0, frees = 0;
  long fail_at = 0;          // > 0: that allocation from now fails (1 = the next one)
  size_t last_bytes = 0;
};
inline FakeHip& fake_hip() { static FakeHip f; return f; }

inline hipError_t hipMalloc(void** p, size_t bytes) {
  FakeHip& f = fake_hip();
  if (f.fail_at > 0 && --f.fail_at == 0) return hipErrorOutOfMemory;      // (*p is left as it was, as the runtime does)
  *p = std::malloc(bytes ? bytes : 1);
  ++f.live; ++f.mallocs;
  f.last_bytes = bytes;
  return hipSuccess;
}
inline hipError_t hipFree(void* p) {
  FakeHip& f = fake_hip();
  if (p) { std::free(p); --f.live; ++f.frees; }
  return hipSuccess;
}
constexpr unsigned hipHostMallocDefault = 0;
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
inline hipError_t hipHostFree(void* p) { return hipFree(p); }
