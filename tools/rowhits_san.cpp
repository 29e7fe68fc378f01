// rowhits_san.cpp — the host twins of the row-pair entry points (dmx_rowpairdist_host,
// dmx_rowhits_host) on a few small cases, for a host ASan + UBSan build:
// `make -C nanopore-barcoding-orc_amd sanitize-rowhits` builds the library's host code and this
// program with the sanitizers and runs it.  Exit 0 = every result as expected and no report.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dmx.h"

static int fails = 0;
#define EXPECT(x)                                                   \
    do {                                                            \
        if (!(x)) {                                                 \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
            ++fails;                                                \
        }                                                           \
    } while (0)

// Rows over A/C/G/T/N, '-' and R/Y as mask bytes, closed up.
struct Rows {
    std::vector<uint8_t> masks;
    std::vector<uint64_t> off{0};
    void add(const std::string& s) {
        for (const char ch : s) {
            const char* at = std::strchr("ACGTN", ch);
            masks.push_back(at ? (uint8_t)(1u << (at - "ACGTN"))
                               : ch == 'R' ? 5 : ch == 'Y' ? 10 : 0);
        }
        off.push_back(masks.size());
    }
};

static uint32_t dist(const Rows& R, int mode, uint32_t q, uint32_t t, uint8_t flag,
                     int expect = DMX_OK) {
    uint32_t out = 12345u;
    const int rc = dmx_rowpairdist_host(mode, R.off.size() - 1, R.masks.data(), R.off.data(), &q,
                                        &t, &flag, nullptr, 1, &out, 1);
    EXPECT(rc == expect);
    return out;
}

int main() {
    Rows R;
    for (const char* s : {"ACGT", "ANGT", "A-GT", "ARGT", "AYGT", "ACGTACGT", "TTTTACGGTT", "G",
                          "AACCGGTTAACCGGTTAACCGGTTAACCGGTTAACCGGTTAACCGGTTAACCGGTTAACCGGTTA", ""})
        R.add(s);
    EXPECT(dist(R, DMX_PD_NW, 0, 0, 0) == 0 && dist(R, DMX_PD_NW, 0, 1, 0) == 1);
    EXPECT(dist(R, DMX_PD_NW, 2, 2, 0) == 1);                       // a gap equals nothing
    EXPECT(dist(R, DMX_PD_NW, 0, 3, 0) == 1 && dist(R, DMX_PD_NW, 0, 4, 0) == 0);
    EXPECT(dist(R, DMX_PD_NW, 0, 5, 0) == 4 && dist(R, DMX_PD_HW, 0, 5, 0) == 0);
    EXPECT(dist(R, DMX_PD_HW, 5, 0, 0) == 4);                       // the longer query
    EXPECT(dist(R, DMX_PD_HW, 0, 6, 0) == 1);                       // ACGG in the target
    EXPECT(dist(R, DMX_PD_HW, 0, 6, DMX_PD_RC) == 1);               // AACCGTAAAA: ACCG / CCGT
    EXPECT(dist(R, DMX_PD_NW, 7, 8, DMX_PD_RC) == 64);              // 1 against 65 columns
    EXPECT(dist(R, DMX_PD_NW, 8, 8, 0) == 0);
    dist(R, 2, 0, 0, 0, DMX_E_INVALID);
    dist(R, DMX_PD_NW, 0, 10, 0, DMX_E_INVALID);                    // a row outside
    dist(R, DMX_PD_NW, 0, 0, 2, DMX_E_INVALID);                     // an unknown flag
    dist(R, DMX_PD_NW, 0, 9, 0, DMX_E_UNSUPPORTED);                 // an empty row
    EXPECT(dmx_rowpairdist_host(DMX_PD_NW, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                0, nullptr, 4) == DMX_OK);
    {   // caps, several threads, repeated pairs
        const uint32_t q[6] = {0, 0, 5, 0, 8, 7}, t[6] = {5, 5, 0, 6, 8, 8}, caps[6] = {0, 9, 2, 0, 0, 3};
        uint32_t out[6];
        EXPECT(dmx_rowpairdist_host(DMX_PD_NW, R.off.size() - 1, R.masks.data(), R.off.data(), q, t,
                                    nullptr, caps, 6, out, 3) == DMX_OK);
        EXPECT(out[0] == 1 && out[1] == 4 && out[2] == 3 && out[3] == 1 && out[4] == 0 && out[5] == 4);
    }
    {   // dmx_rowhits_host: ascending hits, ties forward, cap -1 never, room too small
        const uint32_t q[5] = {0, 0, 0, 7, 0}, t[5] = {5, 6, 6, 8, 0};
        int32_t cap[5] = {0, 1, 0, -1, 0};
        uint32_t pair[5] = {9, 9, 9, 9, 9}, d[5];
        uint8_t rev[5];
        size_t n = 77;
        EXPECT(dmx_rowhits_host(DMX_PD_HW, R.off.size() - 1, R.masks.data(), R.off.data(), q, t, cap,
                                5, pair, d, rev, 5, &n, 2) == DMX_OK);
        EXPECT(n == 3 && pair[0] == 0 && pair[1] == 1 && pair[2] == 4);
        EXPECT(d[0] == 0 && d[1] == 1 && d[2] == 0 && rev[0] == 0 && rev[1] == 0 && rev[2] == 0);
        pair[0] = 9;
        EXPECT(dmx_rowhits_host(DMX_PD_HW, R.off.size() - 1, R.masks.data(), R.off.data(), q, t, cap,
                                5, pair, d, rev, 2, &n, 2) == DMX_E_INVALID);
        EXPECT(n == 3 && pair[0] == 9);
        cap[2] = -2;
        EXPECT(dmx_rowhits_host(DMX_PD_HW, R.off.size() - 1, R.masks.data(), R.off.data(), q, t, cap,
                                5, pair, d, rev, 5, &n, 2) == DMX_E_INVALID);
        EXPECT(n == 0);
        EXPECT(dmx_rowhits_host(DMX_PD_HW, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                                nullptr, nullptr, 0, &n, 1) == DMX_OK && n == 0);
    }
    if (fails) return 1;
    std::puts("rowhits_san: ok");
    return 0;
}
