// snpm_scratch.hpp -- the device scratch of ONE panel scan as parts of one block: each part's place is worked out on the host
// before the block is asked for (scratch_commit of snpm_api_rows.hpp; the block is ctx->ws_scan).  Plain host arithmetic: no HIP
// symbol, no allocation, nothing that throws.
//
// What an entry point that uses it keeps to:
//  - every want() and the one scratch_commit come BEFORE the first copy, memset or launch of the call: a commit that grows frees
//    the old block, so it may not happen while the call's own work is queued.  A call sizes for the largest of its slabs;
//  - the call ends with the stream synchronised on every path that queued work: the next call may write the same bytes (a path
//    that a failed HIP call ends early is the exception it was before: the next commit that grows synchronises before it frees);
//  - a part holds nothing when the call begins (any scan's leftovers): the call writes every byte a kernel reads (DESIGN.md
//    section 29 lists who does, part by part).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace snpm {

struct Scratch {
    static constexpr int kMaxParts = 12;        // marker_select: 11 with its row list
    static constexpr size_t kAlign = 4096;      // every part starts on a multiple of it: never less aligned than a block of its own was

    // `count` elements behind `p`: p is null until assign().  A part of no elements still takes kAlign bytes, so its pointer is
    // valid and no other part's.  A 13th part, or bytes past SIZE_MAX, refuse the whole layout: ok() is false, assign() does nothing.
    template <class T>
    void want(T *&p, size_t count)
    {
        p = nullptr;
        const size_t room = SIZE_MAX - end;
        if (bad || n == kMaxParts || room < kAlign || count > (room - kAlign) / sizeof(T)) {
            bad = true;
            return;
        }
        where[n] = (void *)&p;
        off[n++] = end;
        const size_t bytes = count * sizeof(T);
        end += ((bytes ? bytes : 1) + kAlign - 1) / kAlign * kAlign;
    }
    bool ok() const { return !bad; }
    size_t total() const { return bad ? 0 : end; }
    // base: a block of total() bytes, aligned to kAlign for the parts to be
    void assign(void *base) const
    {
        for (int i = 0; i < n && !bad; ++i) {
            void *q = (char *)base + off[i];
            memcpy(where[i], &q, sizeof(q));    // (the T * behind where[i]: every object pointer has one representation here)
        }
    }

private:
    void *where[kMaxParts];
    size_t off[kMaxParts];
    size_t end = 0;
    int n = 0;
    bool bad = false;
};

}  // namespace snpm
