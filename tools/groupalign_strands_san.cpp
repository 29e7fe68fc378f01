// groupalign_strands_san.cpp — dmx_groupalign_strands_host (a strand per member)
// on a few groups with reversed members of 1, 63, 64 and 65 nt, for a host ASan + UBSan build:
// `make -C nanopore-barcoding-orc_amd sanitize-groupalign` builds the library's host code and
// this program with the sanitizers and runs it.  A flagged member must give what the unflagged
// entry point gives on a batch in which that read lies reverse-complemented.  Exit 0 = every
// result as expected and no report.
#include <cstdio>
#include <cstdlib>
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

static std::string revcomp(const std::string& s) {
    std::string r(s.rbegin(), s.rend());
    for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : c;
    return r;
}

struct Batch {
    std::vector<uint32_t> seq, nm, len;
    std::vector<uint64_t> off;
    explicit Batch(const std::vector<std::string>& reads) {
        std::vector<uint8_t> blob;
        std::vector<uint64_t> at;
        for (const auto& s : reads) {
            at.push_back(blob.size());
            len.push_back((uint32_t)s.size());
            blob.insert(blob.end(), s.begin(), s.end());
        }
        const size_t words = dmx_pack_words(blob.size(), reads.size());
        seq.assign(words, 0), nm.assign(words, 0), off.assign(reads.size(), 0);
        EXPECT(dmx_pack(blob.data(), at.data(), len.data(), reads.size(), seq.data(), nm.data(),
                        off.data()) >= 0);
    }
};

struct Result {
    int rc = 0;
    std::vector<uint64_t> col_off, op_off;
    std::vector<uint8_t> mask, ops;
    std::vector<uint16_t> count, first;
    std::vector<uint32_t> dist;
    bool operator==(const Result& o) const {
        return rc == o.rc && col_off == o.col_off && op_off == o.op_off && mask == o.mask &&
               ops == o.ops && count == o.count && first == o.first && dist == o.dist;
    }
};

static Result run(const Batch& b, const std::vector<uint8_t>& seeds,
                  const std::vector<uint64_t>& seed_off, const std::vector<uint32_t>& members,
                  const uint8_t* flags, const std::vector<uint64_t>& member_off, int threads) {
    const size_t ng = seed_off.size() - 1, cap = 4096;
    Result r;
    r.col_off.assign(ng + 1, 0), r.op_off.assign(members.size() + 1, 0);
    r.mask.assign(cap, 0), r.count.assign(5 * cap, 0), r.first.assign(5 * cap, 0);
    r.ops.assign(4 * cap, 0), r.dist.assign(members.size(), 0);
    r.rc = dmx_groupalign_strands_host(b.seq.data(), b.nm.data(), b.off.data(), b.len.data(),
                                       b.len.size(), ng, seeds.data(), seed_off.data(),
                                       members.data(), flags, member_off.data(), 0,
                                       r.col_off.data(), r.mask.data(), r.count.data(),
                                       r.first.data(), cap, r.dist.data(), r.op_off.data(),
                                       r.ops.data(), r.ops.size(), threads);
    if (r.rc == DMX_OK) {
        r.mask.resize(r.col_off[ng]), r.count.resize(5 * r.col_off[ng]);
        r.first.resize(5 * r.col_off[ng]), r.ops.resize(r.op_off[members.size()]);
    }
    return r;
}

int main() {
    // reads of 1, 63, 64 and 65 nt with N at the ends and at the word boundary, and a forward one
    std::vector<std::string> reads;
    uint32_t s = 2024;
    for (size_t m : {1u, 63u, 64u, 65u, 40u}) {
        std::string r(m, 'A');
        for (char& c : r) {
            s = s * 1664525u + 1013904223u;
            c = "ACGT"[(s >> 16) & 3u];
        }
        if (m > 1) r[0] = r[m - 1] = 'N';
        if (m > 64) r[63] = r[64] = 'N';
        reads.push_back(r);
    }
    std::vector<std::string> turned(reads);
    for (size_t k = 0; k < 4; ++k) turned[k] = revcomp(reads[k]);
    const Batch fwd(reads), rev(turned);

    // seeds: single-bit masks, a gap and an IUPAC column; groups of 2, 3, 0 and 1 members
    std::vector<uint8_t> seeds;
    std::vector<uint64_t> seed_off{0};
    for (size_t g = 0; g < 4; ++g) {
        const std::string& from = turned[(g + 1) % 4];
        for (size_t k = 0; k < from.size(); ++k) {
            const char c = from[k];
            uint8_t mk = c == 'A' ? 1 : c == 'C' ? 2 : c == 'G' ? 4 : c == 'T' ? 8 : 16;
            if (k % 11 == 5) mk = 0;        // '-'
            if (k % 13 == 7) mk = 1 | 4;    // R
            seeds.push_back(mk);
        }
        seed_off.push_back(seeds.size());
    }
    const std::vector<uint32_t> members{1, 4, 2, 0, 3, 3};
    const std::vector<uint64_t> member_off{0, 2, 5, 5, 6};
    const std::vector<uint8_t> flags{DMX_PD_RC, 0, DMX_PD_RC, DMX_PD_RC, DMX_PD_RC, DMX_PD_RC};

    const Result want = run(rev, seeds, seed_off, members, nullptr, member_off, 1);
    EXPECT(want.rc == DMX_OK);
    for (int threads : {1, 3}) {
        const Result got = run(fwd, seeds, seed_off, members, flags.data(), member_off, threads);
        EXPECT(got == want);
    }
    // no flags and all-zero flags are the unflagged entry point's result
    const std::vector<uint8_t> zeros(members.size(), 0);
    EXPECT(run(fwd, seeds, seed_off, members, zeros.data(), member_off, 2) ==
           run(fwd, seeds, seed_off, members, nullptr, member_off, 2));
    // an unknown flag bit is refused, naming group and member
    std::vector<uint8_t> bad(flags);
    bad[3] = 2;
    EXPECT(run(fwd, seeds, seed_off, members, bad.data(), member_off, 1).rc == DMX_E_INVALID);
    const char* msg = dmx_last_error(nullptr);
    EXPECT(msg && std::strstr(msg, "group 1") && std::strstr(msg, "member 1"));
    if (fails) return 1;
    std::puts("groupalign_strands_san: ok");
    return 0;
}
