// ctx_mem_check.cpp -- drives csrc/gs_mem.h (the record of a context's allocations) with a counting malloc / free backend.
// Stand-alone: g++ -std=c++17 -fsanitize=address,undefined -I <root> host/ctx_mem_check.cpp && ./a.out   (exit 0 = all held)
#include <stdio.h>
#include <stdlib.h>

#include <set>

#include "gaussiansplattingmlx_amd/csrc/gs_mem.h"

namespace {

std::set<void*> g_device, g_pinned;      // what the backend has handed out and not got back
long g_allocs = 0, g_failAt = -1;        // allocations asked for so far; the one (0-based) that fails, -1: none
int g_waits = 0;

int take(std::set<void*>& s, void** p, size_t bytes)
{
    if (g_allocs++ == g_failAt) return 2;      // (an allocator's "out of memory")
    *p = malloc(bytes);
    s.insert(*p);
    return 0;
}
int give(std::set<void*>& s, void* p)
{
    if (!s.erase(p)) { fprintf(stderr, "backend: free of a pointer it never handed out\n"); exit(3); }
    free(p);
    return 0;
}
const GsMemBackend kBackend = {
    [](void** p, size_t bytes) { return take(g_device, p, bytes); },
    [](void* p) { return give(g_device, p); },
    [](void** p, size_t bytes, unsigned) { return take(g_pinned, p, bytes); },
    [](void* p) { return give(g_pinned, p); },
};
int wait_ok() { g_waits++; return 0; }

int g_failed = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed++; } \
    } while (0)

struct Buf { void* p = nullptr; long long cap = 0; size_t elem = 4; bool pinned = false; size_t bytes = 0; };

// the reported device bytes equal the sum over the live device buffers, and count no pinned one
void check_bytes(const GsMem& m, const Buf* b, int n)
{
    size_t dev = 0, entries = 0;
    for (int i = 0; i < n; i++) {
        if (!b[i].p) { CHECK(b[i].cap == 0); continue; }
        entries++;
        if (!b[i].pinned) dev += b[i].bytes;
    }
    CHECK(m.deviceBytes == dev);
    CHECK(m.live.size() == entries);
    CHECK(g_device.size() + g_pinned.size() == entries);
}

void scripted_mix()
{
    GsMem m;
    m.backend = &kBackend;
    const int n = 40;
    Buf b[n];
    unsigned r = 12345u;
    auto rnd = [&](unsigned k) { r = r * 1664525u + 1013904223u; return (r >> 8) % k; };
    for (int i = 0; i < n; i++) { b[i].elem = (size_t)1 << rnd(4); b[i].pinned = i % 5 == 4; }
    for (int step = 0; step < 2000; step++) {
        Buf& x = b[rnd(n)];
        const unsigned op = rnd(4);
        if (op == 0 && !x.p) {                     // plain allocation
            x.bytes = (size_t)(1 + rnd(300)) * x.elem;
            CHECK(m.alloc(&x.p, x.bytes, x.pinned, 0) == 0 && x.p);
            x.cap = (long long)(x.bytes / x.elem);
        } else if (op == 1 && x.p) {               // free
            CHECK(m.free(x.p));
            x.p = nullptr; x.cap = 0; x.bytes = 0;
        } else if (!x.pinned) {                    // grow: sometimes within the capacity, sometimes beyond it
            const long long want = 1 + rnd(400);
            void* before = x.p;
            const long long capBefore = x.cap;
            const long allocs = g_allocs;
            const int waits = g_waits;
            CHECK(m.grow(&x.p, &x.cap, want, x.elem, wait_ok) == 0);
            if (want <= capBefore) {               // ... touches nothing
                CHECK(x.p == before && x.cap == capBefore && g_allocs == allocs && g_waits == waits);
            } else {
                CHECK(x.p && x.cap == want && g_allocs == allocs + 1);
                CHECK(g_waits == waits + (before ? 1 : 0));      // waited for exactly where a buffer existed
                x.bytes = (size_t)want * x.elem;
            }
        }
        check_bytes(m, b, n);
    }
    m.freeAll();
    CHECK(m.deviceBytes == 0 && m.live.empty() && g_device.empty() && g_pinned.empty());
}

void failing_allocation()
{
    // nine allocations: buffers 0 .. 2 by alloc, 3 .. 5 by a first grow and a regrow each; every one of them fails once
    for (long failAt = 0; failAt < 9; failAt++) {
        GsMem m;
        m.backend = &kBackend;
        g_allocs = 0;
        g_failAt = failAt;
        Buf b[6];
        for (int i = 0; i < 6; i++) {
            const size_t before = m.deviceBytes;
            int e = i < 3 ? m.alloc(&b[i].p, 64 * (size_t)(i + 1)) : m.grow(&b[i].p, &b[i].cap, 8, 4, wait_ok);
            if (e) CHECK(e == 2 && b[i].p == nullptr && b[i].cap == 0 && m.deviceBytes == before);
            if (i < 3) continue;
            // the regrow: a failed allocation has taken the old buffer's bytes off and leaves pointer null, capacity 0
            const size_t mid = m.deviceBytes, old = (size_t)b[i].cap * 4;
            e = m.grow(&b[i].p, &b[i].cap, 16 * (i + 1), 4, wait_ok);
            if (e) CHECK(e == 2 && b[i].p == nullptr && b[i].cap == 0 && m.deviceBytes == mid - old);
            else CHECK(b[i].p && b[i].cap == 16 * (i + 1) && m.deviceBytes == mid - old + 64 * (size_t)(i + 1));
        }
        CHECK(g_allocs == 9);
        g_failAt = -1;
        m.freeAll();      // every buffer that did get allocated is still freed
        CHECK(m.deviceBytes == 0 && m.live.empty() && g_device.empty() && g_pinned.empty());
    }
}

void unknown_pointer()
{
    GsMem m;
    m.backend = &kBackend;
    void* mine = nullptr;
    CHECK(m.alloc(&mine, 32) == 0);
    int other = 0;
    CHECK(!m.free(&other));                 // refused: the backend's free is not reached (it would exit(3))
    CHECK(m.deviceBytes == 32 && m.live.size() == 1);
    CHECK(m.free(nullptr));                 // null: a no-op
    void* p = &other;
    long long cap = 4;
    CHECK(m.grow(&p, &cap, 8, 4, wait_ok) != 0 && p == &other);      // a grow does not free what it does not own either
    CHECK(m.free(mine) && !m.free(mine));   // the second free of the same pointer is refused too
    CHECK(m.deviceBytes == 0 && g_device.empty());
}

}  // namespace

int main()
{
    scripted_mix();
    failing_allocation();
    unknown_pointer();
    if (g_failed) { fprintf(stderr, "ctx_mem_check: %d checks failed\n", g_failed); return 1; }
    printf("ctx_mem_check ok: %ld allocations, %d waits\n", g_allocs, g_waits);
    return 0;
}
