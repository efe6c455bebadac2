// Host-only driver for tests/test_devmem.py: seal-embedded_amd/csrc/se_devmem.h against a logging stub of the
// HIP runtime calls it makes (built with plain g++, no GPU, not linked against the runtime).  Every scenario prints
// "== <name>" and then one line per runtime call; allocations are named a1, a2, ... in the order they were made,
// streams s1, ... and events e1, ....
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <utility>

#include "se_devmem.h"

namespace {
std::map<const void *, std::pair<int, size_t>> g_alloc;   // live allocation -> (id, bytes)
int g_next_id = 0, g_next_stream = 0, g_next_event = 0;
bool g_fail_next_alloc = false;

int id_of(const void *p) { return g_alloc.count(p) ? g_alloc[p].first : -1; }

hipError_t stub_alloc(const char *what, void **p, size_t bytes)
{
    if (g_fail_next_alloc)
    {
        g_fail_next_alloc = false;
        printf("%s %zu -> error\n", what, bytes);
        return hipErrorOutOfMemory;
    }
    *p            = malloc(bytes);
    g_alloc[*p]   = {++g_next_id, bytes};
    printf("%s %zu -> a%d\n", what, bytes, g_next_id);
    return hipSuccess;
}

void stub_free(const char *what, void *p)
{
    const std::pair<int, size_t> a = g_alloc[p];
    bool zero = true;
    for (size_t i = 0; i < a.second; i++) zero = zero && ((const unsigned char *)p)[i] == 0;
    printf("%s a%d zero=%d\n", what, a.first, (int)zero);
    g_alloc.erase(p);
    free(p);
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return stub_alloc("hipMalloc", p, bytes); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return stub_alloc("hipHostMalloc", p, bytes); }
hipError_t hipFree(void *p)
{
    stub_free("hipFree", p);
    return hipSuccess;
}
hipError_t hipHostFree(void *p)
{
    stub_free("hipHostFree", p);
    return hipSuccess;
}
hipError_t hipMemset(void *p, int value, size_t bytes)
{
    printf("hipMemset a%d %d %zu of %zu\n", id_of(p), value, bytes, g_alloc[p].second);
    memset(p, value, bytes);
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int flags)
{
    *s = (hipStream_t)(uintptr_t)++g_next_stream;
    printf("hipStreamCreateWithFlags %u -> s%d\n", flags, g_next_stream);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s)
{
    printf("hipStreamDestroy s%d\n", (int)(uintptr_t)s);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags)
{
    *e = (hipEvent_t)(uintptr_t)++g_next_event;
    printf("hipEventCreateWithFlags %u -> e%d\n", flags, g_next_event);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    printf("hipEventDestroy e%d\n", (int)(uintptr_t)e);
    return hipSuccess;
}
}

using namespace seamd;

static void scenario(const char *name) { printf("== %s\n", name); }

int main()
{
    scenario("secret_grow");
    {
        DevBuf<uint32_t> b{Secret::yes};
        printf("grow %d\n", (int)b.grow(100));
        memset(b.get(), 0xAB, b.size() * sizeof(uint32_t));
        printf("grow %d\n", (int)b.grow(100));
        printf("grow %d\n", (int)b.grow(40));
        printf("grow %d\n", (int)b.grow(200));
        memset(b.get(), 0xAB, b.size() * sizeof(uint32_t));
        printf("size %zu\n", b.size());
    }
    scenario("plain");
    {
        DevBuf<uint16_t> b;
        (void)b.grow(10);
        memset(b.get(), 0xAB, 20);
        (void)b.grow(30);
        memset(b.get(), 0xAB, 60);
    }
    scenario("failed_alloc");
    {
        DevBuf<uint8_t> b{Secret::yes};
        (void)b.grow(16);
        g_fail_next_alloc = true;
        const hipError_t e = b.grow(32);
        printf("error %d null=%d size %zu\n", (int)(e == hipErrorOutOfMemory), (int)(b.get() == nullptr), b.size());
    }
    scenario("move");
    {
        DevBuf<uint64_t> a{Secret::yes};
        (void)a.grow(4);
        DevBuf<uint64_t> b(std::move(a));
        printf("moved null=%d size %zu\n", (int)(a.get() == nullptr), a.size());
        DevBuf<uint64_t> c;
        (void)c.grow(2);
        c = std::move(b);
        printf("moved null=%d size %zu\n", (int)(b.get() == nullptr), b.size());
        printf("holder size %zu\n", c.size());
    }
    scenario("pinned");
    {
        PinnedBuf<uint8_t> s{Secret::yes}, p;
        (void)s.grow(64);
        (void)p.grow(64);
        memset(s.get(), 0xAB, 64);
        memset(p.get(), 0xAB, 64);
        (void)s.grow(128);
        memset(s.get(), 0xAB, 128);
    }
    scenario("handles_empty");
    {
        Stream s;
        Event e;
        Stream t(std::move(s));
        printf("null=%d\n", (int)((hipStream_t)t == nullptr && (hipEvent_t)e == nullptr));
    }
    scenario("handles");
    {
        Stream s;
        Event e;
        (void)s.create(1);
        (void)s.create(1);
        (void)e.create(2);
        Stream t(std::move(s));
        Event f;
        f = std::move(e);
        printf("moved null=%d\n", (int)((hipStream_t)s == nullptr && (hipEvent_t)e == nullptr));
    }
    scenario("end");
    printf("live %zu\n", g_alloc.size());
    return 0;
}
