// Driver for the per-sample FORMAT DP mode of the VCF reader (csrc/snpm_vcf.cpp: snpm_vcf_parse_calls_dp / snpm_vcf_fill_calls_dp),
// built by tests/test_ghmm_cpu.py with -fsanitize=address,undefined and run directly: any out-of-bounds access, leak or undefined
// behaviour on the files it is given ends the run with a non-zero status.  Prints per file what the test compares.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "snpmatch_hip.h"

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; ++a) {
        const char *base = strrchr(argv[a], '/');
        base = base ? base + 1 : argv[a];
        snpm_vcf *v = nullptr;
        const int rc = snpm_vcf_parse_calls_dp(argv[a], &v);
        if (rc != SNPM_OK) {
            printf("%s rc=%d\n", base, rc);
            continue;
        }
        int64_t n = 0;
        int cw = 0, flags = 0, ns = 0;
        snpm_vcf_dims(v, &n, &cw, nullptr, &flags, &ns);
        const int64_t ld = ns + 3;                                   // padded rows: the bytes behind a row stay as they are
        std::vector<int32_t> dp((size_t)(n * ld), 0x5A5A5A5A);
        std::vector<uint8_t> codes((size_t)(n * ld), 0xEE);
        std::vector<uint32_t> chr((size_t)(n * cw));
        std::vector<int64_t> pos((size_t)n);
        int bad = snpm_vcf_fill_calls(v, chr.data(), pos.data(), codes.data(), ld) != SNPM_OK;
        bad |= snpm_vcf_fill_calls_dp(v, dp.data(), ld) != SNPM_OK;
        bad |= snpm_vcf_fill_calls_dp(v, dp.data(), ns - 1) != SNPM_ERR_BADARG;        // a row narrower than the samples
        bad |= snpm_vcf_fill_calls_dp(v, nullptr, ld) != SNPM_ERR_BADARG;
        long long sum = 0;
        for (int64_t r = 0; r < n; ++r) {
            for (int s = 0; s < ns; ++s) sum += dp[(size_t)(r * ld + s)];
            for (int64_t s = ns; s < ld; ++s) bad |= dp[(size_t)(r * ld + s)] != 0x5A5A5A5A;
        }
        printf("%s rc=%d records=%lld samples=%d flags_dp=%d sum=%lld first=%d,%d,%d%s\n", base, rc, (long long)n, ns, (flags >> 4) & 1, sum,
               n ? dp[0] : 0, n && ns > 1 ? dp[1] : 0, n && ns > 2 ? dp[2] : 0, bad ? " BAD" : "");
        snpm_vcf_free(v);
        // the plain call-code parse of the same file holds no depths: the fill refuses it
        if (snpm_vcf_parse_calls(argv[a], &v) == SNPM_OK) {
            if (snpm_vcf_fill_calls_dp(v, dp.data(), ld) != SNPM_ERR_BADARG) printf("%s BAD: depths from a parse without them\n", base);
            snpm_vcf_free(v);
        }
    }
    printf("done\n");
    return 0;
}
