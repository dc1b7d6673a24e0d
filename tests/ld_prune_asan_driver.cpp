// snpm_ld_prune of csrc/snpm_host.cpp under AddressSanitizer + UBSan, as a stand-alone program (built and run as a child process by
// tests/test_ld_cpu.py): r2, eligible and keep are heap blocks of exactly n_rows x band x 8, n_rows and n_rows bytes, so a read
// in front of row 0 or behind the last cell is seen.  Random bands with nan cells, eligible masks, a threshold that equals a cell
// (the comparison is strict), band 1, n_rows 0 and 1; every answer is compared with the greedy loop written out here.
// Prints "case ... ok" per case and "done fails=0".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "snpmatch_hip.h"

static uint64_t g_rng = 0x2545F4914F6CDD1Dull;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

static int g_fails = 0;

static void run_case(int64_t n, int64_t band, int with_eligible, int exact_threshold)
{
    double *r2 = (double *)malloc((size_t)(n * band) * 8 + (n ? 0 : 1));
    uint8_t *eligible = with_eligible ? (uint8_t *)malloc((size_t)n + (n ? 0 : 1)) : nullptr, *keep = (uint8_t *)malloc((size_t)n + (n ? 0 : 1));
    for (int64_t i = 0; i < n * band; ++i) {
        const uint32_t u = rnd() % 100;
        r2[i] = u < 15 ? NAN : u < 30 ? 0.5 : (double)(rnd() % 1000) / 999.0;       // (0.5: cells that equal the threshold below)
    }
    for (int64_t i = 0; i < n && eligible; ++i) eligible[i] = (uint8_t)(rnd() % 4 ? 1 + rnd() % 255 : 0);
    memset(keep, 0xEE, (size_t)n);
    const double threshold = exact_threshold ? 0.5 : 0.3;
    const int rc = snpm_ld_prune(n, band, r2, eligible, threshold, keep);
    std::vector<uint8_t> want((size_t)n, 0);
    long bad = rc != SNPM_OK;
    for (int64_t k = 0; k < n; ++k) {
        bool ok = !eligible || eligible[k];
        for (int64_t j = k - band < 0 ? 0 : k - band; j < k; ++j)
            if (want[(size_t)j] && r2[j * band + (k - j - 1)] > threshold) ok = false;
        want[(size_t)k] = ok;
        bad += keep[k] != want[(size_t)k];
    }
    long kept = 0;
    for (int64_t k = 0; k < n; ++k) kept += keep[k];
    printf("case rows=%lld band=%lld eligible=%d exact=%d kept=%ld %s\n", (long long)n, (long long)band, with_eligible, exact_threshold, kept, bad ? "MISMATCH" : "ok");
    g_fails += bad != 0;
    free(r2); free(eligible); free(keep);
}

int main()
{
    for (int64_t n : {0, 1, 2, 3, 64, 257})
        for (int64_t band : {1, 2, 5, 64, 300})
            for (int flags = 0; flags < 4; ++flags) run_case(n, band, flags & 1, flags >> 1);
    // the refusals, and NULL buffers where there is no row
    uint8_t k1[1];
    double r1[1] = {0.0};
    int bad = snpm_ld_prune(-1, 1, r1, nullptr, 0.2, k1) != SNPM_ERR_BADARG;
    bad += snpm_ld_prune(1, 0, r1, nullptr, 0.2, k1) != SNPM_ERR_BADARG;
    bad += snpm_ld_prune(1, 1, nullptr, nullptr, 0.2, k1) != SNPM_ERR_BADARG;
    bad += snpm_ld_prune(1, 1, r1, nullptr, 0.2, nullptr) != SNPM_ERR_BADARG;
    bad += snpm_ld_prune(0, 1, nullptr, nullptr, 0.2, nullptr) != SNPM_OK;
    printf("case refusals %s\n", bad ? "MISMATCH" : "ok");
    g_fails += bad != 0;
    printf("done fails=%d\n", g_fails);
    return g_fails ? 1 : 0;
}
