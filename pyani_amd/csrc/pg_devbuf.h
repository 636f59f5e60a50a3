// pg_devbuf.h — the owning buffer of libpyani_gpu.so: one hipMalloc block (PgDevBuf<T>) or one pinned hipHostMalloc block
// (PgPinnedBuf<T>) and its size, freed by the destructor.  The only place in the library that allocates or frees such memory.
// Depends on the HIP runtime header and the standard library only (tests/test_devbuf_cpu.py compiles it against a fake
// hipMalloc / hipFree / hipHostMalloc / hipHostFree).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

struct PgDevAlloc {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t free(void* p) { return hipFree(p); }
};
struct PgPinnedAlloc {
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static hipError_t free(void* p) { return hipHostFree(p); }
};

template <typename T, typename A = PgDevAlloc>
struct PgDevBuf {
  T* p = nullptr;
  size_t cap = 0;   // elements; != 0 only while p holds that many

  PgDevBuf() = default;
  PgDevBuf(const PgDevBuf&) = delete;
  PgDevBuf& operator=(const PgDevBuf&) = delete;
  PgDevBuf(PgDevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  PgDevBuf& operator=(PgDevBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    return *this;
  }
  ~PgDevBuf() { release(); }

  // Room for `need` elements.  A buffer that has it is left alone; otherwise the old block is freed and one of `alloc`
  // elements (at least 1) takes its place — the caller's growth rule; contents are NOT kept.  The size is recorded only
  // once the block exists: after a failure the buffer is empty (p == nullptr, cap == 0) and the next call allocates again.
  hipError_t reserve(size_t need, size_t alloc) {
    if (need <= cap) return hipSuccess;
    release();
    const size_t n = alloc > need ? alloc : (need ? need : 1);
    const hipError_t e = A::alloc(reinterpret_cast<void**>(&p), n * sizeof(T));
    if (e != hipSuccess) { p = nullptr; return e; }
    cap = n;
    return hipSuccess;
  }
  hipError_t reserve(size_t need) { return reserve(need, need); }
  // Room for n items of `per` elements each, plus `extra`: a short buffer grows to max(n, twice the items it held).
  hipError_t reserve_items(size_t n, size_t per, size_t extra = 0) {
    const size_t held = cap ? (cap - extra) / per : 0;
    return reserve(n * per + extra, 2 * held * per + extra);
  }

  void release() {   // frees the block; the buffer is empty afterwards
    if (p) (void)A::free(p);
    p = nullptr;
    cap = 0;
  }

  operator T*() const { return p; }   // kernel arguments, copies and pointer arithmetic take the buffer as its pointer
};

template <typename T>
using PgPinnedBuf = PgDevBuf<T, PgPinnedAlloc>;
