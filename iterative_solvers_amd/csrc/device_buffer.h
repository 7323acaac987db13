// device_buffer.h -- Buf<T>: the one owner of device and pinned host memory on the host side of the library.
// A Buf holds a pointer and how it is held: empty, owned device memory, owned pinned host memory, or borrowed (a view of memory
// somebody else releases: never freed here).  Move-only; no size, no stream, no pool.  It converts to T* wherever a raw pointer
// is wanted, so kernel arguments, struct fills, casts, pointer arithmetic and `if (!p)` read as they did with raw pointers.
// No HIP header: the four functions below are only declared.  mi355cg.hip defines them with the HIP calls; the CPU test of this
// header (tests/cpp/device_buffer_driver.cpp) with malloc.
#pragma once

#include <cstddef>

namespace mi355cg {

// Allocators: 0 on success with *out set; otherwise the library's HIP error code with the error text set (`what`, or a text of
// their own when it is nullptr), *out untouched and no sticky HIP error left behind.  zero: hipMemset on the NULL stream.
int mem_device_alloc(void** out, size_t bytes, bool zero, const char* what);
void mem_device_free(void* p);
int mem_pinned_alloc(void** out, size_t bytes, const char* what);
void mem_pinned_free(void* p);

template <typename T>
class Buf {
    enum Kind : unsigned char { kEmpty, kDevice, kPinned, kBorrowed };
    T* p_ = nullptr;
    Kind kind_ = kEmpty;

    void take(Buf& o) { p_ = o.p_; kind_ = o.kind_; o.p_ = nullptr; o.kind_ = kEmpty; }
    void install(void* p, Kind k) { reset(); p_ = static_cast<T*>(p); kind_ = k; }

  public:
    Buf() = default;
    ~Buf() { reset(); }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept { take(o); }
    Buf& operator=(Buf&& o) noexcept { if (this != &o) { reset(); take(o); } return *this; }

    // n elements of device memory / the same zero-filled on the NULL stream / of pinned host memory.  What b held is released once
    // the new memory is there; a failure leaves b as it was.
    static int device(Buf& b, long long n, const char* what = nullptr) {
        void* p = nullptr;
        if (int rc = mem_device_alloc(&p, sizeof(T) * (size_t)n, false, what)) return rc;
        b.install(p, kDevice);
        return 0;
    }
    static int device_zeroed(Buf& b, long long n, const char* what = nullptr) {
        void* p = nullptr;
        if (int rc = mem_device_alloc(&p, sizeof(T) * (size_t)n, true, what)) return rc;
        b.install(p, kDevice);
        return 0;
    }
    static int pinned(Buf& b, long long n, const char* what = nullptr) {
        void* p = nullptr;
        if (int rc = mem_pinned_alloc(&p, sizeof(T) * (size_t)n, what)) return rc;
        b.install(p, kPinned);
        return 0;
    }
    void borrow(T* p) { reset(); p_ = p; kind_ = p ? kBorrowed : kEmpty; }
    void reset() {
        if (kind_ == kDevice) mem_device_free(p_);
        else if (kind_ == kPinned) mem_pinned_free(p_);
        p_ = nullptr; kind_ = kEmpty;
    }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }         // the pinned state words: c->summary_h->it
};

}  // namespace mi355cg
