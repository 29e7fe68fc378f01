// Host sanitizer program for the context's buffer ownership: DevBuf and
// InputSet under ASan + UBSan on a machine without a GPU, where every device allocation fails.
// A failed reserve must read as an empty buffer and swaps must carry pointer and capacity
// together.  dmx_open is only seen to refuse and to leave *out null: without a device it returns
// before it makes a context, so its clean-up of a half-built context is not run here.
// Built and run by `make -C nanopore-barcoding-orc_amd sanitize-ctx`.
#include <cstdint>
#include <cstdio>

#include "../nanopore-barcoding-orc_amd/csrc/dmx_internal.h"

static int fails = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::fprintf(stderr, "ctx_buffers_san: line %d: %s\n", __LINE__, #cond); \
            ++fails;                                                              \
        }                                                                         \
    } while (0)

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
        std::printf("ctx_buffers_san: a device is present, nothing to check here\n");
        return 0;
    }
    dmx_ctx* c = reinterpret_cast<dmx_ctx*>(0x1);
    EXPECT(dmx_open(0, &c) != DMX_OK);
    EXPECT(c == nullptr);

    dmx::DevBuf<uint32_t> a, b;
    EXPECT(a.reserve(1024) != hipSuccess);
    EXPECT(a.p == nullptr && a.cap == 0);
    EXPECT(a.reserve(0) != hipSuccess);
    EXPECT(a.p == nullptr && a.cap == 0);
    EXPECT(dmx::min_cap(a, b) == 0);

    // a pointer that is never dereferenced nor freed: taken out again before the buffers go
    uint32_t fake[4] = {};
    a.p = fake;
    a.cap = 4;
    EXPECT(a.reserve(3) == hipSuccess && a.p == fake && a.cap == 4);   // room already: untouched
    a.swap(b);
    EXPECT(a.p == nullptr && a.cap == 0 && b.p == fake && b.cap == 4);
    EXPECT(dmx::min_cap(a, b) == 0 && dmx::min_cap(b) == 4);

    dmx::InputSet x, y;
    x.lens.swap(b);   // x.lens = fake
    x.n_words = 7;
    EXPECT(x.cap_reads() == 0 && x.cap_words() == 0);
    x.swap(y);
    EXPECT(x.lens.p == nullptr && x.lens.cap == 0 && x.n_words == 0);
    EXPECT(y.lens.p == fake && y.lens.cap == 4 && y.n_words == 7);
    y.lens.p = nullptr;
    y.lens.cap = 0;

    std::printf("ctx_buffers_san: %d failure(s)\n", fails);
    return fails ? 1 : 0;
}
