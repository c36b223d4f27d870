// test_buffer.cpp -- MappedBuf (bayesiannetwork_amd/csrc/bn_buffer.hpp) stand-alone: the owner of a block of mapped page-locked
// memory, its device alias and its capacity, over fakes of the four HIP calls it makes.  The fakes sit on malloc / free, count the
// live blocks and can make the next allocation or the next mapping fail, so the program links without the HIP runtime and does the
// same with and without a GPU (tests/test_cpp_buffer.py builds it with plain g++, and once more with -fsanitize=address,undefined).
// Checked: a failed allocation and a failed mapping leave the object empty and the block held before freed exactly once; the next
// reserve of the same size allocates again; reserve's growth policy; alloc(0); moves; destruction.
// Exit status 0 and "ok: ..." on success, the first violated expectation otherwise.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "bn_buffer.hpp"

using namespace bnmi;

static long g_checks = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++g_checks;                                                          \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

// ---- the fakes
static int g_live = 0, g_allocs = 0, g_frees = 0;
static size_t g_last_bytes = 0;
static bool g_fail_alloc = false, g_fail_map = false;   // the NEXT call of its kind fails (once)
constexpr uintptr_t kAliasShift = uintptr_t(1) << 40;   // the "device" address of a block: never dereferenced

extern "C" hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
    *p = nullptr;
    if (g_fail_alloc) { g_fail_alloc = false; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes);
    if (!*p) return hipErrorOutOfMemory;
    ++g_live; ++g_allocs;
    g_last_bytes = bytes;
    return hipSuccess;
}
extern "C" hipError_t hipHostFree(void* p) {
    std::free(p);
    --g_live; ++g_frees;
    return hipSuccess;
}
extern "C" hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) {
    if (g_fail_map) { g_fail_map = false; return hipErrorInvalidValue; }
    *d = reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(h) + kAliasShift);
    return hipSuccess;
}
extern "C" hipError_t hipFree(void* p) { return hipHostFree(p); }

template <class T>
static bool is_empty(const MappedBuf<T>& b) { return b.get() == nullptr && b.dev() == nullptr && b.capacity() == 0; }
template <class T>
static bool is_alias(const MappedBuf<T>& b) {
    return b.get() != nullptr && reinterpret_cast<uintptr_t>(b.dev()) == reinterpret_cast<uintptr_t>(b.get()) + kAliasShift;
}

static void check_alloc() {
    MappedBuf<double> b;
    CHECK(is_empty(b) && !b);
    CHECK(b.alloc(0) == hipSuccess);            // a buffer sized once: exactly max(count, 1) elements
    CHECK(g_last_bytes == sizeof(double) && b.capacity() == 1 && is_alias(b) && g_live == 1);
    b[0] = 2.5;                                 // converts to and indexes as the host pointer
    double* raw = b;
    CHECK(raw == b.get() && *b == 2.5);
    CHECK(b.alloc(37) == hipSuccess);           // the block before is freed
    CHECK(g_last_bytes == 37 * sizeof(double) && b.capacity() == 37 && is_alias(b) && g_live == 1 && g_frees == 1);
    struct Rec { int x, y; };
    MappedBuf<Rec> r;
    CHECK(r.alloc(3) == hipSuccess);
    r->x = 7;                                   // (-> as on the pointer)
    r[2].y = 9;
    CHECK(r.get()[0].x == 7 && r.capacity() == 3 && g_live == 2);
}

static void check_reserve_policy() {
    MappedBuf<char> c;
    CHECK(c.reserve(0) == hipSuccess && is_empty(c) && g_live == 0);   // nothing asked for, nothing held
    CHECK(c.reserve(1) == hipSuccess);
    CHECK(g_last_bytes == 4096 && c.capacity() == 4096 && is_alias(c));   // the floor
    const int allocs = g_allocs;
    char* const held = c.get();
    CHECK(c.reserve(4096) == hipSuccess && c.reserve(17) == hipSuccess);   // at or below the capacity: the same block
    CHECK(g_allocs == allocs && c.get() == held && c.capacity() == 4096);
    CHECK(c.reserve(4097) == hipSuccess);                                   // above it: twice what was asked for
    CHECK(g_allocs == allocs + 1 && g_last_bytes == 2 * 4097 && c.capacity() == 2 * 4097 && is_alias(c) && g_live == 1);
    MappedBuf<double> d;
    CHECK(d.reserve(100) == hipSuccess);                                    // 2 x 800 bytes < 4096
    CHECK(g_last_bytes == 4096 && d.capacity() == 512);
    CHECK(d.reserve(513) == hipSuccess);
    CHECK(g_last_bytes == 2 * 513 * sizeof(double) && d.capacity() == 1026 && g_live == 2);
}

// what the object holds when a step fails: nothing -- and the next call of the same size gets a block
template <class Grow>
static void check_failure(bool fail_map, Grow grow) {
    MappedBuf<int32_t> b;
    CHECK(grow(b, 1000) == hipSuccess && is_alias(b) && g_live == 1);
    const size_t cap = b.capacity();
    const int frees = g_frees;
    (fail_map ? g_fail_map : g_fail_alloc) = true;
    CHECK(grow(b, 3000) != hipSuccess);
    CHECK(is_empty(b) && !b);
    CHECK(g_live == 0 && g_frees == frees + (fail_map ? 2 : 1));   // the block before once; a block that could not be mapped too
    CHECK(grow(b, 1000) == hipSuccess);                            // (a capacity left standing would skip this allocation)
    CHECK(is_alias(b) && b.capacity() == cap && g_live == 1);
    b[999] = 1;
    // ... and a first allocation that fails
    MappedBuf<int32_t> f;
    (fail_map ? g_fail_map : g_fail_alloc) = true;
    CHECK(grow(f, 10) != hipSuccess && is_empty(f) && g_live == 1);
    CHECK(grow(f, 10) == hipSuccess && is_alias(f) && g_live == 2);
}

static void check_moves() {
    MappedBuf<double> a;
    CHECK(a.reserve(600) == hipSuccess);
    double* const host = a.get();
    double* const dev = a.dev();
    const size_t cap = a.capacity();
    MappedBuf<double> b(std::move(a));                     // construction
    CHECK(is_empty(a) && b.get() == host && b.dev() == dev && b.capacity() == cap && g_live == 1);
    MappedBuf<double> c;
    CHECK(c.alloc(5) == hipSuccess && g_live == 2);
    const int frees = g_frees;
    c = std::move(b);                                      // assignment: what c held is freed
    CHECK(is_empty(b) && c.get() == host && c.dev() == dev && c.capacity() == cap && g_live == 1 && g_frees == frees + 1);
    CHECK(b.reserve(600) == hipSuccess && b.capacity() == cap && g_live == 2);   // a moved-from object starts over
    c = MappedBuf<double>();                               // dropped by assigning an empty one
    CHECK(is_empty(c) && g_live == 1 && g_frees == frees + 2);
    {
        MappedBuf<double> d(std::move(b));
        CHECK(g_live == 1);
    }                                                      // destruction frees once
    CHECK(g_live == 0 && g_frees == frees + 3 && is_empty(b));
}

int main() {
    check_alloc();
    CHECK(g_live == 0);
    check_reserve_policy();
    CHECK(g_live == 0);
    const auto by_reserve = [](MappedBuf<int32_t>& b, size_t n) { return b.reserve(n); };
    const auto by_alloc = [](MappedBuf<int32_t>& b, size_t n) { return b.alloc(n); };
    for (bool fail_map : {false, true}) {
        check_failure(fail_map, by_reserve);
        CHECK(g_live == 0);
        check_failure(fail_map, by_alloc);
        CHECK(g_live == 0);
    }
    check_moves();
    CHECK(g_live == 0 && g_allocs == g_frees && !g_fail_alloc && !g_fail_map);
    std::printf("ok: %ld checks, %d blocks\n", g_checks, g_allocs);
    return 0;
}
