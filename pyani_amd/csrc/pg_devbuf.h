// pg_devbuf.h — the owning device buffer of libpyani_gpu.so: one hipMalloc block and its size, freed by the destructor.
// Depends on the HIP runtime header and the standard library only (tests/test_devbuf_cpu.py compiles it against a fake
// hipMalloc / hipFree).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

template <typename T>
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
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
    if (e != hipSuccess) { p = nullptr; return e; }
    cap = n;
    return hipSuccess;
  }
  hipError_t reserve(size_t need) { return reserve(need, need); }

  void release() {   // frees the block; the buffer is empty afterwards
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }

  operator T*() const { return p; }   // kernel arguments, copies and pointer arithmetic take the buffer as its pointer
};
