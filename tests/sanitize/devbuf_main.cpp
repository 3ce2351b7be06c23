// Stand-alone harness for the owner type of the context's device buffers (csrc/spt_devbuf.h), built with ASan + UBSan by
// tests/test_devbuf_sanitize.py; no HIP runtime is linked and nothing runs on a GPU.  hipMalloc / hipFree / hipMemcpy are defined here over
// malloc / free / memcpy with a count of the live allocations, and a counter makes the k-th allocation fail -- the path no GPU test reaches.
// Checks: grow keeps the pointer when need <= cap and otherwise frees and reallocates, `alloc` sizes the allocation while `need` is the
// capacity, a failed grow or upload leaves {nullptr, 0}, moves transfer ownership and free the assignee's old buffer, upload of 0 bytes
// allocates without copying, a struct of buffers assigned a fresh value frees them all, and nothing is live at the end.
#include "../../optix-test-smallpt_amd/csrc/spt_devbuf.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

static int g_bad = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_bad; } \
    } while (0)

static std::map<void*, size_t> g_live;      // allocation -> bytes
static long g_fail_in = 0;                  // > 0: the g_fail_in-th allocation from now fails
static unsigned long g_mallocs = 0, g_frees = 0, g_copies = 0;

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes)
{
    ++g_mallocs;
    if (g_fail_in > 0 && --g_fail_in == 0) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes);                // (exactly `bytes`: ASan sees a write past what the buffer asked for)
    if (!*p) return hipErrorOutOfMemory;
    g_live[*p] = bytes;
    return hipSuccess;
}
hipError_t hipFree(void* p)
{
    if (!p) return hipSuccess;
    ++g_frees;
    if (!g_live.erase(p)) { std::printf("FAILED: hipFree of %p, which is not live\n", p); ++g_bad; return hipErrorInvalidValue; }
    std::free(p);
    return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind)
{
    ++g_copies;
    std::memcpy(dst, src, bytes);
    return hipSuccess;
}
}

static size_t bytes_of(const void* p)
{
    const auto it = g_live.find(const_cast<void*>(p));
    return it == g_live.end() ? 0 : it->second;
}

static void grow_checks()
{
    DevBuf<float> b;
    CHECK(b.ptr == nullptr && b.cap == 0 && g_live.empty());
    CHECK(b.grow(0) == hipSuccess && b.ptr == nullptr && g_mallocs == 0);       // nothing needed, nothing allocated
    CHECK(b.grow(100) == hipSuccess && b.ptr && b.cap == 100 && bytes_of(b.ptr) == 400);
    float* const first = b.ptr;
    CHECK(b.grow(100) == hipSuccess && b.ptr == first && b.grow(7) == hipSuccess && b.ptr == first && b.cap == 100 && g_mallocs == 1);
    const unsigned long frees = g_frees;
    CHECK(b.grow(101) == hipSuccess && b.cap == 101 && g_frees == frees + 1 && g_live.size() == 1 && bytes_of(b.ptr) == 404);
    // `alloc` elements behind a capacity of `need`: the packed guides (3 planes per pixel), the chunk tables (3 * n + 512)
    CHECK(b.grow(200, 3 * 200 + 512) == hipSuccess && b.cap == 200 && bytes_of(b.ptr) == (3 * 200 + 512) * sizeof(float));
    float* const p = b;                                                          // the conversion launch functions take
    CHECK(p == b.ptr && b + 1 == b.ptr + 1 && (b ? 1 : 0) == 1);
    // the allocation fails: the old buffer is gone (contents are never kept), the buffer is empty, and it can grow again
    g_fail_in = 1;
    CHECK(b.grow(1000) == hipErrorOutOfMemory && b.ptr == nullptr && b.cap == 0 && g_live.empty());
    CHECK(!b && b.grow(5) == hipSuccess && b.cap == 5 && g_live.size() == 1);
    b.reset();
    CHECK(b.ptr == nullptr && b.cap == 0 && g_live.empty());
    b.reset();                                                                   // (twice is fine)
    CHECK(b.grow(3) == hipSuccess);
}                                                                                // ... and the destructor frees

static void upload_checks()
{
    const unsigned src[6] = {1, 2, 3, 4, 5, 6};
    DevBuf<unsigned> b;
    CHECK(b.upload(src, sizeof src) == hipSuccess && b.ptr && b.cap == 0 && bytes_of(b.ptr) == sizeof src);
    CHECK(std::memcmp(b.ptr, src, sizeof src) == 0);
    unsigned* const first = b.ptr;
    const unsigned long frees = g_frees;
    CHECK(b.upload(src, 8) == hipSuccess && g_frees == frees + 1 && g_live.size() == 1 && bytes_of(b.ptr) == 16);   // below 16 bytes: padded
    (void)first;
    const unsigned long copies = g_copies;
    CHECK(b.upload(nullptr, 0) == hipSuccess && b.ptr && bytes_of(b.ptr) == 16 && g_copies == copies);             // empty table: a valid address, no copy
    g_fail_in = 1;
    CHECK(b.upload(src, sizeof src) == hipErrorOutOfMemory && b.ptr == nullptr && b.cap == 0 && g_live.empty());
    // an uploaded table has no capacity: a grow replaces it
    CHECK(b.upload(src, sizeof src) == hipSuccess && b.grow(2) == hipSuccess && b.cap == 2 && bytes_of(b.ptr) == 8 && g_live.size() == 1);
}

struct Group {                              // the shape of the context's groups: buffers beside flags
    unsigned mask = 0;
    DevBuf<float> accum[6], frame[6];
    DevBuf<unsigned char> bytes;
};

static void move_checks()
{
    DevBuf<float> a, b;
    CHECK(a.grow(10) == hipSuccess && b.grow(20) == hipSuccess && g_live.size() == 2);
    float* const pa = a.ptr;
    float* const pb = b.ptr;
    DevBuf<float> m(std::move(a));                                               // move construction: the source is empty
    CHECK(m.ptr == pa && m.cap == 10 && a.ptr == nullptr && a.cap == 0 && g_live.size() == 2);
    b = std::move(m);                                                            // move assignment frees the assignee's old buffer
    CHECK(b.ptr == pa && b.cap == 10 && m.ptr == nullptr && m.cap == 0 && g_live.size() == 1 && bytes_of(pb) == 0);
    DevBuf<float>& self = b;
    b = std::move(self);                                                         // onto itself: kept
    CHECK(b.ptr == pa && b.cap == 10 && g_live.size() == 1);
    b = DevBuf<float>{};                                                         // a fresh value frees
    CHECK(b.ptr == nullptr && g_live.empty());

    // commit-or-nothing: locals uploaded one after another, moved into place after the last; a failure part-way drops the locals only
    const float table[8] = {};
    DevBuf<float> cur0, cur1;
    CHECK(cur0.upload(table, sizeof table) == hipSuccess && cur1.upload(table, 16) == hipSuccess);
    float* const old0 = cur0.ptr;
    float* const old1 = cur1.ptr;
    {
        DevBuf<float> n0, n1;
        g_fail_in = 2;
        const bool ok = n0.upload(table, sizeof table) == hipSuccess && n1.upload(table, sizeof table) == hipSuccess;
        CHECK(!ok && n0.ptr && !n1.ptr);
        if (ok) { cur0 = std::move(n0); cur1 = std::move(n1); }
    }
    CHECK(cur0.ptr == old0 && cur1.ptr == old1 && g_live.size() == 2);

    // a struct of several buffers assigned a fresh value frees them all and resets its flags; so does dropping a vector of buffers
    Group g;
    g.mask = 0x2Du;
    for (int k = 0; k < 6; ++k)
        if ((g.mask >> k) & 1u) CHECK(g.accum[k].grow(30) == hipSuccess && g.frame[k].grow(30) == hipSuccess);
    CHECK(g.bytes.grow(5) == hipSuccess && g_live.size() == 2 + 8 + 1);
    g = Group{};
    CHECK(g.mask == 0 && g.accum[0].ptr == nullptr && g.frame[5].ptr == nullptr && g.bytes.ptr == nullptr && g_live.size() == 2);
    std::vector<DevBuf<unsigned char>> tables;
    for (int i = 0; i < 9; ++i) {                                                // (reallocations of the vector move the owners)
        tables.emplace_back();
        CHECK(tables.back().upload(table, sizeof table) == hipSuccess);
    }
    CHECK(g_live.size() == 2 + 9);
    tables = std::vector<DevBuf<unsigned char>>{};
    CHECK(g_live.size() == 2);
}

int main()
{
    grow_checks();
    CHECK(g_live.empty());
    upload_checks();
    CHECK(g_live.empty());
    move_checks();
    CHECK(g_live.empty() && g_frees + 3 == g_mallocs);                           // (three allocations were made to fail)
    std::printf("allocations %lu, frees %lu, live %zu, mismatches %d, devbuf sanitizer run %s\n", g_mallocs, g_frees, g_live.size(), g_bad,
                g_bad == 0 && g_live.empty() ? "ok" : "FAILED");
    return g_bad == 0 && g_live.empty() ? 0 : 1;
}
