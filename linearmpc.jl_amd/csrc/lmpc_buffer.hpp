// Memory and launch records a handle owns, free of HIP so that a host program can test them (tests/buffer_check.cpp):
// the owning buffer, the rule for several buffers behind one capacity field, the reset of the scratch sub-object, and
// the ring of launch records.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>

namespace lmpc {

// One block of `size()` elements from the policy Alloc:
//     static E allocate(void **p, void **dev, size_t bytes);     E{} (zero) is success; *dev = the block's device address
//     static void release(void *p);
// Grow-only: reserve() keeps a block that is large enough, and otherwise FREES THE OLD BLOCK FIRST and then allocates,
// so that the two never exist side by side.  After a failed allocation the buffer is empty.
template <class T, class Alloc>
class Buffer {
    T *p_ = nullptr, *dev_ = nullptr;
    size_t n_ = 0;

public:
    using Error = decltype(Alloc::allocate(nullptr, nullptr, size_t{}));
    Buffer() = default;
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    Buffer(Buffer &&o) noexcept : p_(o.p_), dev_(o.dev_), n_(o.n_) { o.p_ = o.dev_ = nullptr; o.n_ = 0; }
    Buffer &operator=(Buffer &&o) noexcept {
        if (this != &o) { reset(); std::swap(p_, o.p_); std::swap(dev_, o.dev_); std::swap(n_, o.n_); }
        return *this;
    }
    ~Buffer() { reset(); }

    Error reserve(size_t count) {
        if (count <= n_) return Error{};
        reset();
        void *p = nullptr, *d = nullptr;
        const Error e = Alloc::allocate(&p, &d, sizeof(T) * count);
        if (e != Error{}) return e;
        p_ = static_cast<T *>(p); dev_ = static_cast<T *>(d); n_ = count;
        return e;
    }
    void reset() {
        if (p_) Alloc::release(const_cast<void *>(static_cast<const volatile void *>(p_)));
        p_ = dev_ = nullptr; n_ = 0;
    }
    size_t size() const { return n_; }
    T *get() const { return p_; }
    T *dev() const { return dev_; }               // where the device sees the block (a device block: get() itself)
    operator T *() const { return p_; }
    // typed view of a byte buffer whose element type varies from call to call
    template <class U> U *as() const { return reinterpret_cast<U *>(p_); }
};

// Several buffers whose size one capacity field stands for.  reserve_group(cap, want, sized(b, count)...) leaves the
// group either whole at `want`, or -- after a failed allocation -- empty with cap = 0: never part-allocated with the old
// capacity still recorded.  Every member is freed before any is allocated.  A member that stays lazy (allocated by its
// first user) is listed with count 0: it is released with the group and left empty.
template <class B> struct Sized { B &buf; size_t count; };
template <class B> Sized<B> sized(B &buf, size_t count) { return Sized<B>{buf, count}; }

template <class Cap, class B0, class... B>
typename B0::Error reserve_group(Cap &cap, Cap want, Sized<B0> m0, Sized<B>... m) {
    using E = typename B0::Error;
    E e{};
    if (want <= cap) return e;
    cap = 0;
    m0.buf.reset(); (m.buf.reset(), ...);
    e = m0.buf.reserve(m0.count);
    ((e == E{} ? void(e = m.buf.reserve(m.count)) : void()), ...);
    if (e != E{}) { m0.buf.reset(); (m.buf.reset(), ...); return e; }
    cap = want;
    return e;
}

// A struct of buffers with their capacity and phase fields (the handle's scratch): every block freed, every field back
// at its default, whatever the struct holds
template <class S> void reset_all(S &s) { s = S{}; }

// The KEPT most recent launch records of one kind, WORDS words each; word 0 is the record's number in the handle's
// life (1, 2, ...), stamped by push().  Host memory only.
template <int WORDS, int KEPT>
struct LaunchRing {
    int32_t rec[KEPT][WORDS] = {};
    long long n = 0;                              // records pushed so far
    void push(const int32_t (&r)[WORDS]) {
        int32_t *d = rec[n % KEPT];
        for (int q = 0; q < WORDS; q++) d[q] = r[q];
        d[0] = (int32_t)((n + 1) & 0x7fffffff);
        n++;
    }
    // the min(n, KEPT, max) most recent records into out, oldest first; how many
    int read(int32_t *out, int max) const {
        long long k = n < KEPT ? n : KEPT;
        if (k > max) k = max;
        for (long long q = 0; q < k; q++)
            for (int w = 0; w < WORDS; w++) out[q * WORDS + w] = rec[(n - k + q) % KEPT][w];
        return (int)k;
    }
    int32_t *newest() { return n ? rec[(n - 1) % KEPT] : nullptr; }
};

}  // namespace lmpc
