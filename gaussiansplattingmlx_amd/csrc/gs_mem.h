// gs_mem.h -- the record of every allocation a context owns (device and pinned host).  Plain C++: the allocator is reached
// through a backend of four functions, which the library binds to HIP (api.hip) and host/ctx_mem_check.cpp to a counting malloc.
#pragma once
#include <stddef.h>

#include <vector>

// each returns 0 on success, otherwise the allocator's own error code (handed through to the caller)
struct GsMemBackend {
    int (*deviceAlloc)(void** p, size_t bytes);
    int (*deviceFree)(void* p);
    int (*pinnedAlloc)(void** p, size_t bytes, unsigned flags);
    int (*pinnedFree)(void* p);
};

struct GsMem {
    struct Entry { void* p; size_t bytes; bool pinned; };
    const GsMemBackend* backend = nullptr;
    std::vector<Entry> live;       // searched linearly: contexts hold some eighty buffers, and no training step allocates or frees
    size_t deviceBytes = 0;        // sum of the live device entries (pinned host memory is recorded, not counted)

    // *p = a new allocation of `bytes`, recorded; on failure *p is null, nothing is recorded and the backend's code is returned
    int alloc(void** p, size_t bytes, bool pinned = false, unsigned flags = 0)
    {
        *p = nullptr;
        const int e = pinned ? backend->pinnedAlloc(p, bytes, flags) : backend->deviceAlloc(p, bytes);
        if (e) { *p = nullptr; return e; }
        live.push_back({*p, bytes, pinned});
        if (!pinned) deviceBytes += bytes;
        return 0;
    }
    // forgets and frees p.  false: the record does not know p -- nothing is freed, the caller reports it (null is known: a no-op)
    bool free(void* p)
    {
        if (!p) return true;
        for (size_t i = 0; i < live.size(); i++) {
            if (live[i].p != p) continue;
            const Entry e = live[i];
            live[i] = live.back();
            live.pop_back();
            if (!e.pinned) deviceBytes -= e.bytes;
            (void)(e.pinned ? backend->pinnedFree(e.p) : backend->deviceFree(e.p));
            return true;
        }
        return false;
    }
    // Grow on demand: *p holds *cap elements of elemBytes and must hold `want`.  Nothing happens while want <= *cap; otherwise
    // wait() first if the buffer exists (queued work may still read it; non-zero = its error, returned with the buffer intact),
    // then free, *cap = 0, allocate `want`, *cap = want.  *cap is 0 whenever *p is null, so a failed allocation leaves no
    // capacity that lies.
    template <class Cap, class Wait>
    int grow(void** p, Cap* cap, long long want, size_t elemBytes, Wait&& wait)
    {
        if (want <= (long long)*cap) return 0;
        if (*p) {
            if (const int e = wait()) return e;
            if (!free(*p)) return -1;      // (not this record's buffer: left alone, and no allocator's code is -1)
            *p = nullptr;
        }
        *cap = 0;
        if (const int e = alloc(p, (size_t)want * elemBytes)) return e;
        *cap = (Cap)want;
        return 0;
    }
    // what is left when the context goes
    void freeAll()
    {
        while (!live.empty()) (void)free(live.back().p);
    }
};
