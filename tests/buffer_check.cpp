// Host check of csrc/lmpc_buffer.hpp (tests/test_buffer_host.py builds it with the address and undefined-behaviour
// sanitizers and runs it): the owning buffer, the group rule, the scratch reset and the launch-record ring, on an
// allocator backed by malloc that counts its live blocks, logs its calls and fails the k-th allocation on request.
// Links neither HIP nor the library.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../linearmpc.jl_amd/csrc/lmpc_buffer.hpp"

static int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::printf("FAIL line %d: %s\n", __LINE__, #cond); g_failed++; } \
    } while (0)

static long g_live = 0;            // blocks allocated and not yet freed
static long g_allocs = 0;          // allocations attempted
static long g_fail_at = 0;         // the allocation with this number fails (0: none)
static long g_map_fail_at = 0;     // ... of the mapped allocator: its device-address step fails
static std::string g_log;          // 'a' per block handed out, 'f' per block freed, 'x' per refusal

struct TestAlloc {
    static int allocate(void **p, void **dev, size_t bytes) {
        if (++g_allocs == g_fail_at) { g_log += 'x'; *p = nullptr; return 2; }
        *p = std::malloc(bytes);
        *dev = *p;
        g_live++; g_log += 'a';
        return 0;
    }
    static void release(void *p) { std::free(p); g_live--; g_log += 'f'; }
};
// the shape of the mapped-host policy: a block, then its device address, and both or nothing
struct TestMapped {
    static int allocate(void **p, void **dev, size_t bytes) {
        const int e = TestAlloc::allocate(p, dev, bytes);
        if (e != 0) return e;
        if (g_allocs == g_map_fail_at) { TestAlloc::release(*p); *p = nullptr; return 3; }
        *dev = static_cast<char *>(*p) + 1;        // (some other address: the two are told apart below)
        return 0;
    }
    static void release(void *p) { TestAlloc::release(p); }
};
template <class T> using Buf = lmpc::Buffer<T, TestAlloc>;

static void reset_counters() { g_allocs = 0; g_fail_at = 0; g_map_fail_at = 0; g_log.clear(); }

static void check_buffer() {
    reset_counters();
    {
        Buf<double> b;
        CHECK(b.size() == 0 && b.get() == nullptr && !b);
        CHECK(b.reserve(0) == 0 && g_log.empty());
        CHECK(b.reserve(10) == 0 && b.size() == 10 && b && g_live == 1);
        double *p = b;
        p[9] = 1.0;                                         // (the sanitizer checks the size)
        CHECK(b + 3 == p + 3 && b.dev() == p);
        CHECK(b.reserve(10) == 0 && b.reserve(4) == 0 && b.get() == p && b.size() == 10 && g_log == "a");
        // a larger reserve frees before it allocates
        CHECK(b.reserve(20) == 0 && b.size() == 20 && g_log == "afa" && g_live == 1);
        b[19] = 2.0;
        // a failed allocation leaves the buffer empty; the next one succeeds
        g_fail_at = g_allocs + 1;
        CHECK(b.reserve(40) == 2 && b.size() == 0 && b.get() == nullptr && b.dev() == nullptr && g_live == 0 && g_log == "afafx");
        CHECK(b.reserve(40) == 0 && b.size() == 40 && g_live == 1);
        Buf<double> c(std::move(b));
        CHECK(b.size() == 0 && !b && c.size() == 40 && g_live == 1);
        b = std::move(c);
        CHECK(c.size() == 0 && b.size() == 40 && g_live == 1);
        lmpc::Buffer<unsigned char, TestAlloc> bytes;
        CHECK(bytes.reserve(64) == 0 && static_cast<void *>(bytes.as<float>()) == static_cast<void *>(bytes.get()));
        b.reset();
        CHECK(b.size() == 0 && !b && g_live == 1);
    }
    CHECK(g_live == 0);                                     // the destructor releases
}

static void check_group() {
    for (int first = 0; first <= 1; first++)                // from empty, and from a group that is whole at 5
        for (int pos = 1; pos <= 3; pos++) {
            reset_counters();
            Buf<int32_t> a, b;
            Buf<double> c, lazy;
            long cap = 0;
            if (first) {
                CHECK(lmpc::reserve_group(cap, 5l, lmpc::sized(a, 5), lmpc::sized(b, 10), lmpc::sized(c, 15), lmpc::sized(lazy, 0)) == 0);
                CHECK(cap == 5 && g_live == 3);
                CHECK(lazy.reserve(5) == 0);                // (its first user)
                CHECK(lmpc::reserve_group(cap, 3l, lmpc::sized(a, 3), lmpc::sized(b, 6), lmpc::sized(c, 9), lmpc::sized(lazy, 0)) == 0);
                CHECK(cap == 5 && a.size() == 5 && lazy.size() == 5);        // smaller: nothing happens
            }
            g_log.clear();
            g_fail_at = g_allocs + pos;
            CHECK(lmpc::reserve_group(cap, 9l, lmpc::sized(a, 9), lmpc::sized(b, 18), lmpc::sized(c, 27), lmpc::sized(lazy, 0)) == 2);
            CHECK(cap == 0 && !a && !b && !c && !lazy && g_live == 0);
            CHECK(a.size() == 0 && b.size() == 0 && c.size() == 0);
            // every old block is freed before the first new one is asked for
            const std::string frees(first ? 4 : 0, 'f');
            CHECK(g_log.compare(0, frees.size() + 1, frees + (pos == 1 ? "x" : "a")) == 0);
            CHECK(lmpc::reserve_group(cap, 9l, lmpc::sized(a, 9), lmpc::sized(b, 18), lmpc::sized(c, 27), lmpc::sized(lazy, 0)) == 0);
            CHECK(cap == 9 && a.size() == 9 && b.size() == 18 && c.size() == 27 && !lazy && g_live == 3);
        }
    CHECK(g_live == 0);
}

static void check_mapped() {
    reset_counters();
    lmpc::Buffer<volatile int32_t, TestMapped> m;
    g_map_fail_at = 1;
    CHECK(m.reserve(16) == 3 && !m && m.dev() == nullptr && m.size() == 0 && g_live == 0 && g_log == "af");
    CHECK(m.reserve(16) == 0 && m && g_live == 1);
    CHECK(reinterpret_cast<volatile char *>(m.dev()) == reinterpret_cast<volatile char *>(m.get()) + 1);
    *m = 7; m[15] = 8;
    CHECK(*m == 7);
    m.reset();
    CHECK(!m && m.dev() == nullptr && g_live == 0);
}

// a scratch sub-object as the handle has it: buffers, capacities, phase fields with defaults other than 0
struct Scratch {
    Buf<double> theta, lazy;
    Buf<int32_t> list[2];
    long cap = 0;
    int countSet = 0;
    long warmN = -1;
    long seg[2] = {0, 0};
};
struct Handle : Scratch {
    Buf<double> pack;
    int option = 3;
};

static void check_scratch() {
    reset_counters();
    {
        Handle h;
        CHECK(h.pack.reserve(8) == 0);
        CHECK(lmpc::reserve_group(h.cap, 6l, lmpc::sized(h.theta, 6), lmpc::sized(h.list[0], 6), lmpc::sized(h.list[1], 6), lmpc::sized(h.lazy, 0)) == 0);
        CHECK(h.lazy.reserve(6) == 0);
        h.countSet = 1; h.warmN = 6; h.seg[1] = 4; h.option = 5;
        double *const pack = h.pack;
        CHECK(g_live == 5);
        lmpc::reset_all(static_cast<Scratch &>(h));
        CHECK(g_live == 1 && !h.theta && !h.lazy && !h.list[0] && !h.list[1]);
        CHECK(h.cap == 0 && h.countSet == 0 && h.warmN == -1 && h.seg[0] == 0 && h.seg[1] == 0);
        CHECK(h.pack.get() == pack && h.pack.size() == 8 && h.option == 5);         // what is not scratch stays
        CHECK(lmpc::reserve_group(h.cap, 2l, lmpc::sized(h.theta, 2), lmpc::sized(h.list[0], 2), lmpc::sized(h.list[1], 2), lmpc::sized(h.lazy, 0)) == 0);
        CHECK(h.cap == 2 && g_live == 4);
    }
    CHECK(g_live == 0);
}

template <int KEPT>
static void check_ring() {
    constexpr int W = 3;
    const int pushes[] = {0, 1, 4, 5, 9}, maxes[] = {0, 2, KEPT, KEPT + 1};
    for (int np : pushes) {
        lmpc::LaunchRing<W, KEPT> r;
        CHECK(r.newest() == nullptr);
        for (int i = 1; i <= np; i++) {
            const int32_t rec[W] = {-5, 10 * i, 100 * i};         // (word 0 is stamped by the ring)
            r.push(rec);
            CHECK(r.newest() != nullptr && r.newest()[0] == i && r.newest()[1] == 10 * i);
        }
        CHECK(r.n == np);
        for (int max : maxes) {
            int32_t out[(KEPT + 2) * W];
            for (int32_t &v : out) v = -1;
            int want = np < KEPT ? np : KEPT;
            if (want > max) want = max;
            CHECK(r.read(out, max) == want);
            for (int q = 0; q < want; q++) {                // the `want` most recent, oldest first
                const int seq = np - want + 1 + q;
                CHECK(out[q * W] == seq && out[q * W + 1] == 10 * seq && out[q * W + 2] == 100 * seq);
            }
            CHECK(out[want * W] == -1);                     // nothing written past them
        }
    }
    lmpc::LaunchRing<W, KEPT> r;                            // the row launcher's word in the newest front record
    const int32_t rec[W] = {0, 1, 2};
    r.push(rec); r.push(rec);
    r.newest()[2] = 77;
    int32_t out[2 * W];
    const int k = r.read(out, 2);
    CHECK(out[(k - 1) * W + 2] == 77 && out[(k - 1) * W] == 2);
}

int main() {
    check_buffer();
    check_group();
    check_mapped();
    check_scratch();
    check_ring<4>();
    check_ring<1>();
    CHECK(g_live == 0);
    if (g_failed) { std::printf("%d check(s) failed\n", g_failed); return 1; }
    std::printf("buffer_check ok\n");
    return 0;
}
