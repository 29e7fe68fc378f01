// speciesgroups_san.cpp — the host twins of the species-group entry points (dmx_hithist_host,
// dmx_pairhits_cross_host, dmx_hitgroups_within_host) on a few small cases, for a
// host ASan + UBSan build: `make -C nanopore-barcoding-orc_amd sanitize-speciesgroups` builds the
// library's host code and this program with the sanitizers and runs it.  Exit 0 = every result
// as expected and no report.
#include <cstdio>
#include <cstdlib>
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

int main() {
    const uint32_t X = DMX_LG_NONE;
    // six reads; reads 0..2 are group 0, 3..4 group 1, 5 in no group.  Pairs (q, t, outcome):
    const std::vector<uint32_t> q = {0, 0, 1, 3, 2, 4, 0, 1}, t = {1, 2, 2, 4, 3, 5, 5, 0};
    const std::vector<uint32_t> outc = {2, 5, 3u | DMX_LG_REV, 1, 4, 6, 9, X};
    const std::vector<uint32_t> label = {0, 0, 0, 1, 1, X};
    {   // the histogram: a row of 10 classes per read, class = 9 - d; the call adds
        std::vector<uint32_t> bin_off(6);
        std::vector<uint16_t> bins(60);
        for (uint32_t r = 0; r < 6; ++r) {
            bin_off[r] = 10 * r;
            for (uint32_t d = 0; d < 10; ++d) bins[10 * r + d] = (uint16_t)(9 - d);
        }
        std::vector<uint64_t> hist(10, 1);
        EXPECT(dmx_hithist_host(t.data(), outc.data(), q.size(), 6, bin_off.data(), bins.data(),
                                bins.size(), 10, hist.data()) == DMX_OK);
        EXPECT(hist == (std::vector<uint64_t>{2, 1, 1, 2, 2, 2, 2, 2, 2, 1}));
        const std::vector<uint64_t> before = hist;
        // the largest index is 5 * 10 + 9 = 59: 60 entries serve it, 59 do not
        EXPECT(dmx_hithist_host(t.data(), outc.data(), q.size(), 6, bin_off.data(), bins.data(), 59,
                                10, hist.data()) == DMX_E_INVALID);
        EXPECT(dmx_hithist_host(t.data(), outc.data(), q.size(), 6, bin_off.data(), bins.data(), 60,
                                8, hist.data()) == DMX_E_INVALID);   // class 8 of 8
        EXPECT(dmx_hithist_host(t.data(), outc.data(), q.size(), 5, bin_off.data(), bins.data(), 60,
                                10, hist.data()) == DMX_E_INVALID);  // target 5 of 5 reads
        EXPECT(dmx_hithist_host(t.data(), outc.data(), q.size(), 6, bin_off.data(), bins.data(), 60,
                                1025, hist.data()) == DMX_E_INVALID);
        EXPECT(hist == before);
        EXPECT(dmx_hithist_host(nullptr, nullptr, 0, 0, nullptr, nullptr, 0, 4, hist.data()) == DMX_OK);
        EXPECT(hist == before);
    }
    {   // the cross hits at cap2: pairs 4 (2 -> 3, d 4), 5 (4 -> 5, d 6); pair 6 (d 9) is too far
        const std::vector<int32_t> cap2 = {5, 5, 5, 5, 5, 6};
        uint32_t pair[8], d[8];
        uint8_t rev[8];
        size_t n = 99;
        EXPECT(dmx_pairhits_cross_host(q.data(), t.data(), outc.data(), q.size(), 6, label.data(),
                                       cap2.data(), pair, d, rev, 8, &n) == DMX_OK);
        EXPECT(n == 2 && pair[0] == 4 && d[0] == 4 && rev[0] == 0 && pair[1] == 5 && d[1] == 6);
        n = 99;
        pair[0] = 77;
        EXPECT(dmx_pairhits_cross_host(q.data(), t.data(), outc.data(), q.size(), 6, label.data(),
                                       cap2.data(), pair, d, rev, 1, &n) == DMX_E_INVALID);
        EXPECT(n == 2 && pair[0] == 77);   // the room needed is reported, nothing is written
        const std::vector<int32_t> none(6, -1);
        EXPECT(dmx_pairhits_cross_host(q.data(), t.data(), outc.data(), q.size(), 6, label.data(),
                                       none.data(), nullptr, nullptr, nullptr, 0, &n) == DMX_OK);
        EXPECT(n == 0);
    }
    {   // the components: inside group 0 the hits with d <= tie2[t]; read 2 has no edge of its own
        std::vector<uint32_t> tie2 = {X, 2, X, X, 1, X}, labels(8, 12345u);
        EXPECT(dmx_hitgroups_within_host(q.data(), t.data(), outc.data(), q.size(), 6, tie2.data(),
                                         label.data(), nullptr, nullptr, 0, 6, labels.data()) == DMX_OK);
        EXPECT((std::vector<uint32_t>(labels.begin(), labels.begin() + 6) ==
                std::vector<uint32_t>{0, 0, X, 3, 3, X}));
        // two clones of read 5, one per group: nodes 6 and 7 do not join the groups
        const std::vector<uint32_t> xa = {0, 4}, xb = {6, 7};
        EXPECT(dmx_hitgroups_within_host(q.data(), t.data(), outc.data(), q.size(), 6, tie2.data(),
                                         label.data(), xa.data(), xb.data(), 2, 8, labels.data()) == DMX_OK);
        EXPECT((labels == std::vector<uint32_t>{0, 0, X, 3, 3, X, 0, 3}));
        const std::vector<uint32_t> far = {8};
        EXPECT(dmx_hitgroups_within_host(q.data(), t.data(), outc.data(), q.size(), 6, tie2.data(),
                                         label.data(), xa.data(), far.data(), 1, 8, labels.data()) ==
               DMX_E_INVALID);
        EXPECT(dmx_hitgroups_within_host(q.data(), t.data(), outc.data(), q.size(), 6, tie2.data(),
                                         label.data(), nullptr, nullptr, 0, 5, labels.data()) ==
               DMX_E_INVALID);
    }
    if (fails) return 1;
    std::puts("speciesgroups_san: ok");
    return 0;
}
