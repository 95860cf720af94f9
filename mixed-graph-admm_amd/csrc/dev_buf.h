// Owning buffer of the engines' device and pinned memory: the block and its capacity in one object, so that no failed
// allocation or copy can leave a pointer and a size that disagree.  Plain C++ (tests/cpu/dev_buf_check.cpp replays the failure
// paths on the CPU with a counting policy); the HIP policies DevMem and PinnedMem: common.h.
//   Mem::alloc(void**, size_t bytes) and Mem::to_device(void* dst, const void* src, size_t bytes) return 0 on success;
//   Mem::release(void*) gives a block back.
// What reserve and upload return is Mem's error code as it came, or BUF_TOO_LARGE; the call sites turn it into their status.
// Neither waits for the device: where a kernel may still read the old block, the caller synchronises first.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

constexpr int BUF_TOO_LARGE = -1;      // n * sizeof(T) does not fit a size_t: refused before Mem is asked

template <class T, class Mem>
class Buf {
    T* p = nullptr;
    size_t cap = 0;      // elements of *p; 0 with p == nullptr, nowhere else

public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            std::swap(p, o.p);
            std::swap(cap, o.cap);
        }
        return *this;
    }
    ~Buf() { reset(); }

    T* get() const { return p; }
    size_t capacity() const { return cap; }
    explicit operator bool() const { return p != nullptr; }

    // at least n elements, contents not preserved.  The new block is allocated before the old one is released: on failure the
    // buffer is exactly as it was
    int reserve(size_t n) {
        if (n <= cap) return 0;
        if (n > (size_t)-1 / sizeof(T)) return BUF_TOO_LARGE;
        void* q = nullptr;
        if (const int rc = Mem::alloc(&q, n * sizeof(T))) return rc;
        reset();
        p = static_cast<T*>(q);
        cap = n;
        return 0;
    }
    // max(1, v.size()) elements with v at the front.  A block that has to grow is replaced only after the copy into the new
    // one succeeded; a failed copy leaves the buffer with the block and capacity it had (none, if it had none)
    int upload(const std::vector<T>& v) {
        Buf fresh;
        Buf& dst = v.size() <= cap && p ? *this : fresh;
        if (const int rc = dst.reserve(v.size() ? v.size() : 1)) return rc;
        if (!v.empty())
            if (const int rc = Mem::to_device(dst.p, v.data(), v.size() * sizeof(T))) return rc;
        if (&dst == &fresh) *this = std::move(fresh);
        return 0;
    }
    void reset() {
        if (p) Mem::release(p);
        p = nullptr;
        cap = 0;
    }
};
