// The merge-rank encoder's rank table as the uploads build it (merge_encode.hip):
// the filter of a merge list and its open-addressing table, on the host alone — no gbpe_ctx,
// no HIP call — so that tools/micro/merge_table_check.cpp runs it under a sanitizer on a CPU.
// The hash and the probing below are also the device's (me_find).
//
// Two layouts of the 16-byte slot, by the width of the ids a table may hold:
//   narrow (gbpe_bpe_upload, ids <= 0xFFFF):            {a << 16 | b, rank, new id, 1}
//   wide   (gbpe_bpe_upload_wide, ids <= 0xFFFFFF):     {a, b, rank, new id}
// In both .w == 0 says empty: a new id is at least 256, and the pair (0, 0) is a key like any other.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define ME_HD __host__ __device__
#else
#define ME_HD
#endif

constexpr uint32_t ME_NARROW_MAX_ID = 0xFFFFu;
constexpr uint32_t ME_WIDE_MAX_ID = 0xFFFFFFu;   // GBPE_BPE_MAX_ID (gpubpe.h)

ME_HD inline uint32_t me_fmix32(uint32_t x) {   // Murmur3 finaliser (gbpe_fmix32)
    x = (x ^ (x >> 16)) * 0x7feb352du;
    x = (x ^ (x >> 15)) * 0x846ca68bu;
    return x ^ (x >> 16);
}
// narrow: of the packed pair.  wide: of all 32 bits of a and of b (a times an odd constant is a
// bijection of a; ids below 2^24 leave a * K + b collision-free but for a sparse set of differences)
ME_HD inline uint32_t me_hash_narrow(uint32_t pid) { return me_fmix32(pid); }
ME_HD inline uint32_t me_hash_wide(uint32_t a, uint32_t b) { return me_fmix32(a * 0x9E3779B1u + b); }
// the p-th slot of the probe sequence that starts at h (triangular: visits every slot of a power of two)
ME_HD inline uint32_t me_probe(uint32_t h, uint32_t p, uint32_t mask) { return (h + ((p * (p + 1)) >> 1)) & mask; }

struct MeSlot {   // uint4's layout
    uint32_t x, y, z, w;
};

struct MeHostTable {
    std::vector<MeSlot> slots;     // a power of two, at least 2 n_merges + 16: load below one half
    std::vector<uint32_t> cross;   // 65536 bits: (u << 8 | v) set iff a live merge joins a token ending in u to one starting with v
    uint32_t live = 0;
};

enum MeBuildError { ME_BUILD_OK = 0, ME_BUILD_RANGE, ME_BUILD_BYTE_ID, ME_BUILD_REPEATED_ID };

// merges = [a, b, new id] x n_merges, every value at most max_id (ME_NARROW_MAX_ID with the narrow
// layout, at most ME_WIDE_MAX_ID with the wide one).  A list the encoder is not exact for — a value
// above max_id, a new id below 256, a new id some earlier entry gave — is refused: the first such
// entry's index goes to *bad (and a repeated or byte id to *bad_id) and nothing is built.  Of the
// others an entry is live when both operands exist (a byte, the new id of an earlier live entry) and
// its pair was not live before: the first rank of a pair wins (tokenizer-manager.js:30-33).
// The per-id arrays hold max id of the list + 1 entries: at most 16 MiB each.
inline MeBuildError me_build_table(const uint32_t* merges, uint32_t n_merges, uint32_t max_id, bool wide, MeHostTable* t,
                                   uint32_t* bad, uint32_t* bad_id) {
    enum : uint8_t { EXISTS = 1, GIVEN = 2 };   // GIVEN: the new id of an entry, live or not
    uint32_t top = 255;
    for (uint64_t i = 0; i < 3 * (uint64_t)n_merges; ++i)
        if (merges[i] <= max_id && merges[i] > top) top = merges[i];
    std::vector<uint8_t> state((size_t)top + 1, 0);
    for (uint32_t r = 0; r < n_merges; ++r) {
        const uint32_t a = merges[3 * (uint64_t)r], b = merges[3 * (uint64_t)r + 1], id = merges[3 * (uint64_t)r + 2];
        *bad = r;
        *bad_id = id;
        if (a > max_id || b > max_id || id > max_id) return ME_BUILD_RANGE;
        // a new id must be fresh: one that was in the stream before (a byte, an earlier entry's) breaks
        // "ranks in order = lowest-rank adjacent pair first", and its first / last byte would be two things
        if (id < 256u) return ME_BUILD_BYTE_ID;
        if (state[id] & GIVEN) return ME_BUILD_REPEATED_ID;
        state[id] = GIVEN;
    }
    // (every new id is distinct and in [256, max_id]: n_merges < 2^24, so 2 n_merges + 16 fits)
    uint32_t slots = 16;
    while (slots < 2u * n_merges + 16) slots <<= 1;
    const uint32_t mask = slots - 1;
    t->slots.assign(slots, MeSlot{0, 0, 0, 0});
    t->cross.assign(65536 / 32, 0);
    t->live = 0;
    std::vector<uint8_t> first((size_t)top + 1, 0), last((size_t)top + 1, 0);
    for (uint32_t b = 0; b < 256; ++b) {
        first[b] = last[b] = (uint8_t)b;
        state[b] = EXISTS;
    }
    for (uint32_t r = 0; r < n_merges; ++r) {
        const uint32_t a = merges[3 * (uint64_t)r], b = merges[3 * (uint64_t)r + 1], id = merges[3 * (uint64_t)r + 2];
        if (!(state[a] & EXISTS) || !(state[b] & EXISTS)) continue;   // an operand that does not exist yet: never fires
        const uint32_t pid = (a << 16) | b;   // (narrow only)
        const uint32_t h = (wide ? me_hash_wide(a, b) : me_hash_narrow(pid)) & mask;
        bool dup = false;
        for (uint32_t p = 0; p < slots; ++p) {
            MeSlot& s = t->slots[me_probe(h, p, mask)];
            if (s.w == 0) {
                s = wide ? MeSlot{a, b, r, id} : MeSlot{pid, r, id, 1};
                break;
            }
            if (wide ? (s.x == a && s.y == b) : s.x == pid) {
                dup = true;
                break;
            }
        }
        if (dup) continue;   // the first rank of a pair wins
        ++t->live;
        const uint32_t k = ((uint32_t)last[a] << 8) | first[b];
        t->cross[k >> 5] |= 1u << (k & 31u);
        state[id] |= EXISTS;   // (fresh: no earlier entry set these)
        first[id] = first[a];
        last[id] = last[b];
    }
    return ME_BUILD_OK;
}
