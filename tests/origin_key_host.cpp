// Host-only check of the band-mode key format (dmx_device.h make_key_o / key_t_o / key_delta):
// compiled and run by tests/test_origin_key_host.py.  Exits 0 and prints "ok", or prints the
// first counterexample and exits 1.
#include <cstdio>

#include "dmx_device.h"

using namespace dmx;

static int fail(const char* what, long long a, long long b, long long c) {
    std::printf("FAIL %s: %lld %lld %lld\n", what, a, b, c);
    return 1;
}

int main() {
    // 1. round trip of (t, delta), the other fields untouched, over the field's whole range
    const uint64_t ts[] = {0, 1, 2, 57, 58, 59, 4095, 4096, (1ull << 32) - 1, 1ull << 32,
                           (1ull << 32) + 64, (1ull << 33) - 1, (1ull << 36) - 1};
    for (uint64_t t : ts)
        for (int d = -kBandMaxCost; d <= kBandMaxCost; ++d) {
            const uint64_t k = make_key_o(-3, 1, 7, 200, t, d);
            if (key_t_o(k) != t || key_delta(k) != d) return fail("round trip", (long long)t, d, 0);
            if (key_score(k) != -3 || key_orient(k) != 1 || key_cost(k) != 7 ||
                key_adapter(k) != 200)
                return fail("upper fields", (long long)t, d, 0);
            if (k == ~0ull) return fail("a real key equals the empty slot", (long long)t, d, 0);
        }
    // 2. on every pair of cells that differs in any field other than delta, make_key_o orders
    //    as make_key does, whatever the two deltas are
    struct Cell { int s, o, c, a; uint64_t t; };
    const int scores[] = {-128, -1, 0, 1, 59};
    const int adapters[] = {0, 1, 63};
    const uint64_t t2[] = {0, 1, 58, (1ull << 32) + 5};
    Cell cells[5 * 2 * 8 * 3 * 4];
    int n = 0;
    for (int s : scores)
        for (int o = 0; o < 2; ++o)
            for (int c = 0; c <= kBandMaxCost; ++c)
                for (int a : adapters)
                    for (uint64_t t : t2) cells[n++] = Cell{s, o, c, a, t};
    for (int x = 0; x < n; ++x)
        for (int y = 0; y < n; ++y) {
            if (x == y) continue;
            const Cell &p = cells[x], &q = cells[y];
            const bool want = make_key(p.s, p.o, p.c, p.a, p.t) < make_key(q.s, q.o, q.c, q.a, q.t);
            for (int d1 = -kBandMaxCost; d1 <= kBandMaxCost; ++d1)
                for (int d2 = -kBandMaxCost; d2 <= kBandMaxCost; ++d2)
                    if ((make_key_o(p.s, p.o, p.c, p.a, p.t, d1) <
                         make_key_o(q.s, q.o, q.c, q.a, q.t, d2)) != want)
                        return fail("order", x, y, d1 * 100 + d2);
        }
    // 3. the bound key (an upper bound of the score, the smallest delta code) is <= every real
    //    key of the same cell
    for (int x = 0; x < n; ++x) {
        const Cell& p = cells[x];
        for (int ub = p.s; ub <= 64; ++ub) {
            const uint64_t bound = make_key_o(ub, p.o, p.c, p.a, p.t, kKeyDeltaMin);
            for (int d = -kBandMaxCost; d <= kBandMaxCost; ++d)
                if (bound > make_key_o(p.s, p.o, p.c, p.a, p.t, d)) return fail("bound", x, ub, d);
        }
    }
    std::printf("ok %d cells\n", n);
    return 0;
}
