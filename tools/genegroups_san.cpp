// genegroups_san.cpp — the host twins of the gene-group entry points (dmx_edgegroups_host,
// dmx_pairhits_host, dmx_hitgroups_host) on a few small graphs, for a host
// ASan + UBSan build: `make -C nanopore-barcoding-orc_amd sanitize-genegroups` builds the
// library's host code and this program with the sanitizers and runs it.  Exit 0 = every result
// as expected and no report.
#include <cstdio>
#include <cstdlib>
#include <numeric>
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

static std::vector<uint32_t> groups(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b,
                                    uint32_t n, int expect = DMX_OK) {
    std::vector<uint32_t> labels(n, 12345u);
    const int rc = dmx_edgegroups_host(a.data(), b.data(), a.size(), n, labels.data());
    EXPECT(rc == expect);
    return labels;
}

int main() {
    const uint32_t X = DMX_LG_NONE;
    EXPECT(groups({}, {}, 0).empty());
    EXPECT(groups({}, {}, 3) == (std::vector<uint32_t>{X, X, X}));
    EXPECT(groups({4}, {2}, 6) == (std::vector<uint32_t>{X, X, 2, X, 2, X}));
    EXPECT(groups({3}, {3}, 5) == (std::vector<uint32_t>{X, X, X, 3, X}));
    EXPECT(groups({1, 2, 1, 7, 8}, {2, 1, 2, 8, 7}, 10) ==
           (std::vector<uint32_t>{X, 1, 1, X, X, X, X, 7, 7, X}));
    groups({0, 5}, {1, 2}, 5, DMX_E_INVALID);   // an endpoint out of range: refused, nothing read
    {   // a star with an isolated node, and a path in scrambled index order
        std::vector<uint32_t> a, b;
        for (uint32_t k = 0; k < 40; ++k)
            if (k != 17) a.push_back(40), b.push_back(k);
        auto l = groups(a, b, 41);
        for (uint32_t v = 0; v < 41; ++v) EXPECT(l[v] == (v == 17 ? X : 0u));
        const uint32_t n = 300;
        std::vector<uint32_t> perm(n);
        std::iota(perm.begin(), perm.end(), 0u);
        uint32_t s = 12345;
        for (uint32_t i = n - 1; i > 0; --i) {
            s = s * 1664525u + 1013904223u;
            std::swap(perm[i], perm[(s >> 8) % (i + 1)]);
        }
        a.assign(perm.begin(), perm.end() - 1);
        b.assign(perm.begin() + 1, perm.end());
        l = groups(a, b, n);
        for (uint32_t v = 0; v < n; ++v) EXPECT(l[v] == 0u);
    }
    {   // dmx_hitgroups_host: two cliques joined by one hit that only a loose tie keeps
        std::vector<uint32_t> q, t, outc;
        for (uint32_t base : {0u, 10u})
            for (uint32_t x = base; x < base + 5; ++x)
                for (uint32_t y = x + 1; y < base + 5; ++y) q.push_back(x), t.push_back(y), outc.push_back(4);
        q.push_back(3), t.push_back(12), outc.push_back(9u | DMX_LG_REV);   // the bridge
        q.push_back(6), t.push_back(7), outc.push_back(DMX_LG_NONE);        // no hit: no edge
        std::vector<uint32_t> tie(16, 4), labels(16, 12345u);
        EXPECT(dmx_hitgroups_host(q.data(), t.data(), outc.data(), q.size(), tie.data(), 16,
                                  labels.data()) == DMX_OK);
        for (uint32_t v = 0; v < 16; ++v) EXPECT(labels[v] == (v < 5 ? 0u : v >= 10 && v < 15 ? 10u : X));
        tie[12] = 9;
        EXPECT(dmx_hitgroups_host(q.data(), t.data(), outc.data(), q.size(), tie.data(), 16,
                                  labels.data()) == DMX_OK);
        for (uint32_t v = 0; v < 16; ++v) EXPECT(labels[v] == (v < 5 || (v >= 10 && v < 15) ? 0u : X));
        t[0] = 16;   // a read outside the batch: refused
        EXPECT(dmx_hitgroups_host(q.data(), t.data(), outc.data(), q.size(), tie.data(), 16,
                                  labels.data()) == DMX_E_INVALID);
        EXPECT(dmx_hitgroups_host(nullptr, nullptr, nullptr, 0, tie.data(), 16, labels.data()) == DMX_OK);
        for (uint32_t v = 0; v < 16; ++v) EXPECT(labels[v] == X);
    }
    {   // dmx_pairhits_host on a packed batch: a forward hit, a reverse hit, a miss, caps of -1
        const char* rd[4] = {"ACGTTGCAAGGCTTAACCGGTTACGATCGA", "ACGTTGCAAGGCTTAACCGGTAACGATCGA",
                             "TCGATCGTAACCGGTTAAGCCTTGCAACGT", "GGGGGGGGGGCCCCCCCCCCAAAAAAAAAA"};
        std::vector<uint8_t> blob;
        std::vector<uint64_t> off;
        std::vector<uint32_t> len;
        for (const char* s : rd) {
            off.push_back(blob.size());
            len.push_back(30);
            blob.insert(blob.end(), s, s + 30);
        }
        const size_t words = dmx_pack_words(blob.size(), 4);
        std::vector<uint32_t> seq(words), nm(words);
        std::vector<uint64_t> poff(4);
        EXPECT(dmx_pack(blob.data(), off.data(), len.data(), 4, seq.data(), nm.data(), poff.data()) >= 0);
        const uint32_t q[4] = {0, 0, 0, 0}, t[4] = {1, 2, 3, 1};
        const int32_t hit[4] = {6, 6, 6, -1}, half[4] = {15, 3, 15, -1};
        uint32_t outc[4], best[4];
        uint64_t n_hits = 0;
        EXPECT(dmx_pairhits_host(seq.data(), nm.data(), poff.data(), len.data(), 4, q, t, hit, half, 4,
                                 outc, best, &n_hits, 2) == DMX_OK);
        EXPECT(n_hits == 2 && outc[0] == 1u && outc[1] == (0u | DMX_LG_REV) && outc[2] == X && outc[3] == X);
        EXPECT(best[0] == X && best[1] == 1u && best[2] == 0u && best[3] == X);
    }
    if (fails) return 1;
    std::puts("genegroups_san: ok");
    return 0;
}
