// scratch_host_driver.cpp -- the layout arithmetic of snpm_scratch.hpp alone, on the host: every layout is assigned on a block of
// exactly total() bytes, every byte of every part is written and no part may see another's pattern.  Built with ASan + UBSan and run
// as a child process by tests/test_scratch_cpu.py: a part that leaves the block or a pointer less aligned than its type is a report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "snpm_scratch.hpp"

using snpm::Scratch;

static int fails = 0;

static void report(const char *name, bool ok, size_t total)
{
    printf("case %s total=%zu %s\n", name, total, ok ? "ok" : "FAILED");
    if (!ok) ++fails;
}

struct Part {
    const void *p;
    size_t bytes;
};

// the block of exactly total() bytes; fills part i with its own byte, then checks every part still holds its own
struct Block {
    void *base = nullptr;
    explicit Block(const Scratch &s) { base = s.total() ? aligned_alloc(Scratch::kAlign, s.total()) : nullptr; s.assign(base); }
    ~Block() { free(base); }
};

static bool parts_sound(const Block &b, size_t total, const std::vector<Part> &parts)
{
    bool ok = true;
    for (size_t i = 0; i < parts.size(); ++i) {
        const uint8_t *p = (const uint8_t *)parts[i].p;
        ok = ok && p != nullptr && (uintptr_t)p % Scratch::kAlign == 0 && p >= (const uint8_t *)b.base &&
             p + (parts[i].bytes ? parts[i].bytes : 1) <= (const uint8_t *)b.base + total;
        if (!ok) return false;
        for (size_t j = 0; j < i; ++j) {             // (a part of no bytes still owns its first byte: it aliases nothing)
            const uint8_t *q = (const uint8_t *)parts[j].p;
            ok = ok && (p + (parts[i].bytes ? parts[i].bytes : 1) <= q || q + (parts[j].bytes ? parts[j].bytes : 1) <= p);
        }
    }
    for (size_t i = 0; i < parts.size(); ++i)
        for (size_t k = 0; k < parts[i].bytes; ++k) ((uint8_t *)parts[i].p)[k] = (uint8_t)(0x11 * (i + 1));
    for (size_t i = 0; i < parts.size(); ++i)
        for (size_t k = 0; k < parts[i].bytes; ++k) ok = ok && ((const uint8_t *)parts[i].p)[k] == (uint8_t)(0x11 * (i + 1));
    return ok;
}

int main()
{
    {   // one part of one byte
        Scratch s;
        uint8_t *a;
        s.want(a, 1);
        Block b(s);
        report("one-byte", s.ok() && s.total() == 4096 && parts_sound(b, s.total(), {{a, 1}}), s.total());
    }
    {   // 4095, 4096 and 4097 bytes in a row: one page, one page, two pages
        Scratch s;
        uint8_t *a, *c, *d;
        s.want(a, 4095);
        s.want(c, 4096);
        s.want(d, 4097);
        Block b(s);
        const bool ok = s.ok() && s.total() == 4 * 4096 && c == a + 4096 && d == a + 2 * 4096;
        report("page-edges", ok && parts_sound(b, s.total(), {{a, 4095}, {c, 4096}, {d, 4097}}), s.total());
    }
    {   // a part of no elements between two others: a valid pointer of its own
        Scratch s;
        int32_t *a, *z, *c;
        s.want(a, 5);
        s.want(z, 0);
        s.want(c, 7);
        Block b(s);
        const bool ok = s.ok() && s.total() == 3 * 4096 && z != nullptr && (uint8_t *)z == (uint8_t *)a + 4096 && (uint8_t *)c == (uint8_t *)a + 2 * 4096;
        report("zero-part", ok && parts_sound(b, s.total(), {{a, 20}, {z, 0}, {c, 28}}), s.total());
    }
    {   // twelve parts of growing size; with a thirteenth the layout is refused and nothing is assigned
        for (int extra = 0; extra < 2; ++extra) {
            Scratch s;
            double *p[13];
            std::vector<Part> parts;
            size_t want_total = 0;
            for (int i = 0; i < 12 + extra; ++i) {
                s.want(p[i], (size_t)i * 300 + 1);
                if (i < 12) want_total += (((size_t)i * 300 + 1) * 8 + 4095) / 4096 * 4096;
            }
            if (!extra) {
                Block b(s);
                for (int i = 0; i < 12; ++i) parts.push_back({p[i], ((size_t)i * 300 + 1) * 8});
                report("twelve-parts", s.ok() && s.total() == want_total && parts_sound(b, s.total(), parts), s.total());
            } else {
                uint8_t sentinel[8];
                s.assign(sentinel);
                bool none = !s.ok() && s.total() == 0;
                for (int i = 0; i < 13; ++i) none = none && p[i] == nullptr;
                report("thirteenth-refused", none, s.total());
            }
        }
    }
    {   // a byte size past SIZE_MAX
        Scratch s;
        double *a = (double *)8;
        s.want(a, SIZE_MAX / sizeof(double) + 1);
        uint8_t sentinel[8];
        s.assign(sentinel);
        report("overflow-bytes", !s.ok() && s.total() == 0 && a == nullptr, s.total());
    }
    {   // a byte size that fits, but not once rounded up to a page
        Scratch s;
        uint8_t *a = (uint8_t *)8;
        s.want(a, SIZE_MAX - 100);
        uint8_t sentinel[8];
        s.assign(sentinel);
        report("overflow-rounding", !s.ok() && s.total() == 0 && a == nullptr, s.total());
    }
    {   // a running total past SIZE_MAX: each part fits, the third does not; a later small part does not revive the layout
        Scratch s;
        unsigned long long *a, *c, *d;
        int32_t *e;
        s.want(a, SIZE_MAX / 24);
        s.want(c, SIZE_MAX / 24);
        const bool two = s.ok();
        s.want(d, SIZE_MAX / 24 + 4096);
        s.want(e, 1);
        uint8_t sentinel[8];
        s.assign(sentinel);
        report("overflow-total", two && !s.ok() && s.total() == 0 && a == nullptr && c == nullptr && d == nullptr && e == nullptr, s.total());
    }
    {   // typed pointers: each aligned to a page (UBSan checks the stores through them)
        Scratch s;
        uint8_t *a;
        int32_t *c;
        double *d;
        unsigned long long *e;
        const int32_t *k;                                    // (a pointer to const is a part like any other)
        s.want(a, 3);
        s.want(c, 3);
        s.want(d, 3);
        s.want(e, 3);
        s.want(k, 3);
        Block b(s);
        bool ok = s.ok() && s.total() == 5 * 4096;
        if (ok) {
            a[2] = 1; c[2] = 2; d[2] = 3.0; e[2] = 4ull;
            ok = a[2] == 1 && c[2] == 2 && d[2] == 3.0 && e[2] == 4ull;
        }
        report("typed", ok && parts_sound(b, s.total(), {{a, 3}, {c, 12}, {d, 24}, {e, 24}, {k, 12}}), s.total());
    }
    {   // no part at all
        Scratch s;
        report("empty", s.ok() && s.total() == 0, s.total());
    }
    printf("done fails=%d\n", fails);
    return fails ? 1 : 0;
}
