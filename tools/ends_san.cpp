// Host sanitizer program for the end-window stage: dmx_ends_host and the panel
// set-up's host side (dmx_panel_reach with restricted adapters) under ASan + UBSan, no GPU.
// Built and run by `make -C nanopore-barcoding-orc_amd sanitize-ends`.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "dmx.h"

static int fails = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "ends_san: line %d: %s\n", __LINE__, #cond); \
            ++fails;                                                       \
        }                                                                  \
    } while (0)

struct Batch {
    std::vector<uint32_t> seq, nm;
    std::vector<uint64_t> offs;
    std::vector<uint32_t> lens;
};

static Batch pack(const std::vector<std::string>& reads) {
    Batch b;
    std::string blob;
    std::vector<uint64_t> in_offs;
    uint64_t total = 0;
    for (const auto& r : reads) {
        in_offs.push_back(blob.size());
        b.lens.push_back((uint32_t)r.size());
        blob += r;
        total += r.size();
    }
    const size_t words = dmx_pack_words(total, reads.size());
    b.seq.assign(words, 0);
    b.nm.assign(words, 0);
    b.offs.assign(reads.size(), 0);
    const int rc = dmx_pack((const uint8_t*)blob.data(), in_offs.data(), b.lens.data(),
                            reads.size(), b.seq.data(), b.nm.data(), b.offs.data());
    EXPECT(rc == DMX_OK);
    return b;
}

static std::string rand_dna(std::mt19937& g, int n, bool with_n = false) {
    std::string s;
    for (int i = 0; i < n; ++i) s += (with_n && g() % 17 == 0) ? 'N' : "ACGT"[g() % 4];
    return s;
}

int main() {
    std::mt19937 g(20261020);
    const int types[6] = {DMX_FRONT | DMX_ANCHORED, DMX_FRONT | DMX_NONINTERNAL,
                          DMX_BACK | DMX_ANCHORED, DMX_BACK | DMX_NONINTERNAL, DMX_FRONT,
                          DMX_BACK};
    const double rates[5] = {0.0, 0.1, 0.25, 2.0, 0.4};
    size_t matched = 0, total = 0;
    for (int it = 0; it < 60; ++it) {
        const int lens_pick[6] = {1, 3, 20, 63, 64, 1 + (int)(g() % 64)};
        std::vector<std::string> ads;
        std::vector<const char*> ptr;
        std::vector<int> lens, wheres, mos;
        const int n_ad = 1 + (int)(g() % 6);
        for (int a = 0; a < n_ad; ++a) {
            ads.push_back(rand_dna(g, lens_pick[g() % 6]));
            if (it % 7 == 0 && ads.back().size() > 4) ads.back()[2] = 'N';
            wheres.push_back(types[g() % 6]);
        }
        const int mo = 1 + (int)(g() % 6);
        for (int a = 0; a < n_ad; ++a) {
            ptr.push_back(ads[a].c_str());
            lens.push_back((int)ads[a].size());
            // the unrestricted adapters share -O; restricted ones may carry their own
            mos.push_back((wheres[a] & DMX_NONINTERNAL) ? 1 + (int)(g() % 8) : mo);
        }
        std::vector<std::string> reads = {"", "A", "N"};
        for (int r = 0; r < 40; ++r) {
            const int a = (int)(g() % n_ad);
            std::string piece = ads[a];
            for (auto& ch : piece)
                if (ch == 'N') ch = 'G';
            if (piece.size() > 2 && g() % 2) piece[g() % piece.size()] = 'T';
            if (piece.size() > 4 && g() % 3 == 0) piece.erase(g() % piece.size(), 1);
            const std::string body = rand_dna(g, (int)(g() % 90), true);
            reads.push_back((wheres[a] & DMX_FRONT) ? piece + body : body + piece);
        }
        const Batch b = pack(reads);
        std::vector<dmx_result> out(reads.size());
        const int rc = dmx_ends_host(ptr.data(), lens.data(), wheres.data(),
                                     it % 2 ? mos.data() : nullptr, n_ad, rates[it % 5], mo,
                                     it % 3 != 0, b.seq.data(), b.nm.data(), b.offs.data(),
                                     b.lens.data(), reads.size(), out.data());
        EXPECT(rc == DMX_OK);
        for (size_t r = 0; r < reads.size(); ++r) {
            const dmx_result& x = out[r];
            ++total;
            EXPECT(x.bin1 >= -1 && x.bin1 < n_ad && x.bin2 == -1);
            if (x.bin1 < 0) continue;
            ++matched;
            const int m = lens[x.bin1], w = wheres[x.bin1], n = (int)reads[r].size();
            EXPECT(0 <= x.m1.astart && x.m1.astart <= x.m1.astop && x.m1.astop <= m);
            EXPECT(0 <= x.m1.rstart && x.m1.rstart <= x.m1.rstop && x.m1.rstop <= n);
            if ((w & DMX_FRONT) && (w & (DMX_ANCHORED | DMX_NONINTERNAL))) EXPECT(x.m1.rstart == 0);
            if ((w & DMX_BACK) && (w & (DMX_ANCHORED | DMX_NONINTERNAL))) EXPECT(x.m1.rstop == n);
            if (w & DMX_ANCHORED) EXPECT(x.m1.astart == 0 && x.m1.astop == m);
        }
        // the panel set-up's host side: the reach of the unrestricted sub-panel
        int32_t reach[6];
        const int prc = dmx_panel_reach(ptr.data(), lens.data(), wheres.data(), n_ad, rates[it % 5],
                                        mo, it % 3 != 0 ? DMX_RC : 0, reach, 6);
        EXPECT(prc == DMX_OK || prc == DMX_E_UNSUPPORTED);
        if (prc == DMX_OK) EXPECT(reach[3] <= reach[5] && reach[4] <= reach[5]);
    }
    // refusals
    const char* one[1] = {"ACGT"};
    const int l1[1] = {4};
    const int bad[3] = {DMX_FRONT | DMX_ANCHORED | DMX_NONINTERNAL, DMX_ANCHORED,
                        DMX_FRONT | DMX_BACK | DMX_NONINTERNAL};
    const Batch b = pack({"ACGTACGT"});
    dmx_result out;
    for (int i = 0; i < 3; ++i)
        EXPECT(dmx_ends_host(one, l1, &bad[i], nullptr, 1, 0.1, 3, 0, b.seq.data(), b.nm.data(),
                             b.offs.data(), b.lens.data(), 1, &out) == DMX_E_INVALID);
    EXPECT(std::strstr(dmx_last_error(nullptr), "dmx_ends_host") != nullptr);
    EXPECT(matched > total / 4 && matched < total);
    std::printf("ends_san: %zu records, %zu matched, %d failure(s)\n", total, matched, fails);
    return fails ? 1 : 0;
}
