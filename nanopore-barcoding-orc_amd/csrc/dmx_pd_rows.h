// dmx_pd_rows.h — the rows of masks a call gives, as they lie on the device:
// dmx_rowdist, dmx_rowpairdist / dmx_rowhits and dmx_rowassign share this one type.
#pragma once
#include <cstring>

#include "dmx_internal.h"

namespace dmx {

// A row on the device: where it starts in the mask array and its length (rowpair_rc_kernel).
struct RrRow {
    uint64_t off;
    uint32_t n, pad;
};

// The rows some pair of the call names, closed up in first-use order; every row starts at a
// multiple of 16 columns and is padded to one with zeros (the forward pass loads 16 mask bytes at
// a time).  Their reverse complements lie `total` columns behind them once write_rc has run.
// place() starts a call: nothing of the call before is kept but the capacity of the buffers.
struct PdRows {
    static constexpr uint64_t kAbsent = ~(uint64_t)0;
    std::vector<uint64_t> goff;   // per row of the call: its first column, kAbsent = not uploaded
    std::vector<RrRow> used;      // the uploaded rows
    std::vector<uint8_t> image;   // their `total` bytes
    uint64_t total = 0;
    bool written = false;         // this call's reverse complements are on the device
    DevBuf<uint8_t> mask;
    DevBuf<RrRow> rows;

    // Host only.  rowlen: every row's length (exact for a row that is named); a[i], then b[i]
    // when b is given, are the rows pair i names.
    void place(const uint8_t* masks, const uint64_t* row_off, const std::vector<uint32_t>& rowlen,
               const uint32_t* a, const uint32_t* b, size_t n_pairs) {
        goff.assign(rowlen.size(), kAbsent);
        used.clear();
        total = 0;
        written = false;
        auto take = [&](uint32_t g) {
            if (goff[g] != kAbsent) return;
            goff[g] = total;
            used.push_back(RrRow{total, rowlen[g], 0u});
            total += ((uint64_t)rowlen[g] + 15u) & ~(uint64_t)15u;
        };
        for (size_t i = 0; i < n_pairs; ++i) {
            take(a[i]);
            if (b) take(b[i]);
        }
        image.assign(total, 0);
        for (size_t g = 0; g < goff.size(); ++g)
            if (goff[g] != kAbsent) std::memcpy(image.data() + goff[g], masks + row_off[g], rowlen[g]);
    }
    uint64_t off(uint32_t g, bool reversed) const { return goff[g] + (reversed ? total : 0u); }
    uint64_t cols() const { return written ? 2 * total : total; }   // the columns written so far

    // Room for the rows and their copies, and the image's upload on the context's stream (not
    // waited for: `image` stays as it is until the next place()).
    int upload(Ctx* c, const char* who);
    // The reverse complement of every uploaded row, once per call: a second call does nothing.
    // Adds the kernel's time to *ms.  Synchronises.  ev: two events of the caller's.
    int write_rc(Ctx* c, const char* who, const hipEvent_t* ev, float* ms);
};

}  // namespace dmx
