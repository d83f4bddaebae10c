// merge_table.h's me_build_table on the id-width boundary lists, stand-alone and host-only, meant
// to be compiled and run under AddressSanitizer and UBSan on a CPU (a per-id array sized for 16-bit
// ids and indexed by a 24-bit one would overrun here):
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Igpu-bpe_amd/csrc tools/micro/merge_table_check.cpp -o merge_table_check && ./merge_table_check
//
// Each list is built in the wide layout (and in the narrow one when it fits), every live pair is
// looked up again with the device's hash and probing, and a lowest-rank-first encode over the table
// (the walk's algorithm) must give the tokens written out by hand — the lists and tokens of
// tests/test_merge_wide.py.  Prints one line per list and "ok"; any mismatch exits 1.
#include "merge_table.h"

#include <cstdio>
#include <cstdlib>
#include <string>

namespace {

struct Hit {
    uint32_t rank, id;
};
constexpr uint32_t NONE = 0xFFFFFFFFu;

Hit find(const MeHostTable& t, bool wide, uint32_t a, uint32_t b) {
    const uint32_t mask = (uint32_t)t.slots.size() - 1, pid = (a << 16) | b;
    const uint32_t h = (wide ? me_hash_wide(a, b) : me_hash_narrow(pid)) & mask;
    for (uint32_t p = 0; p <= mask; ++p) {
        const MeSlot& s = t.slots[me_probe(h, p, mask)];
        if (s.w == 0) break;
        if (wide ? (s.x == a && s.y == b) : s.x == pid) return wide ? Hit{s.z, s.w} : Hit{s.y, s.z};
    }
    return Hit{NONE, 0};
}

std::vector<uint32_t> encode(const MeHostTable& t, bool wide, const std::string& text) {
    std::vector<uint32_t> tok(text.begin(), text.end());
    for (auto& v : tok) v &= 0xFFu;
    for (;;) {
        uint32_t best = NONE, ba = 0, bb = 0, bnew = 0;
        for (size_t j = 0; j + 1 < tok.size(); ++j) {
            const Hit e = find(t, wide, tok[j], tok[j + 1]);
            if (e.rank < best) best = e.rank, ba = tok[j], bb = tok[j + 1], bnew = e.id;
        }
        if (best == NONE) return tok;
        std::vector<uint32_t> out;
        for (size_t j = 0; j < tok.size();) {
            if (j + 1 < tok.size() && tok[j] == ba && tok[j + 1] == bb) out.push_back(bnew), j += 2;
            else out.push_back(tok[j++]);
        }
        tok.swap(out);
    }
}

struct Case {
    const char* name;
    std::vector<uint32_t> merges;   // [a, b, new id] ...
    std::string text;
    std::vector<uint32_t> want;
    uint32_t live;
};

int failures = 0;

void fail(const char* name, const char* what) {
    std::printf("FAIL %s: %s\n", name, what);
    ++failures;
}

void run(const Case& c, bool wide) {
    MeHostTable t;
    uint32_t bad = 0, bad_id = 0;
    const uint32_t n = (uint32_t)(c.merges.size() / 3);
    const MeBuildError e = me_build_table(c.merges.data(), n, wide ? ME_WIDE_MAX_ID : ME_NARROW_MAX_ID, wide, &t, &bad, &bad_id);
    if (e != ME_BUILD_OK) return fail(c.name, "rejected");
    if (t.live != c.live) fail(c.name, "live count");
    const std::vector<uint32_t> got = encode(t, wide, c.text);
    if (got != c.want) fail(c.name, "tokens");
    std::printf("%-28s %-6s slots %zu live %u tokens", c.name, wide ? "wide" : "narrow", t.slots.size(), t.live);
    for (uint32_t v : got) std::printf(" 0x%X", v);
    std::printf("\n");
}

void rejected(const char* name, std::vector<uint32_t> merges, uint32_t max_id, bool wide, MeBuildError want, uint32_t index) {
    MeHostTable t;
    uint32_t bad = ~0u, bad_id = 0;
    const MeBuildError e = me_build_table(merges.data(), (uint32_t)(merges.size() / 3), max_id, wide, &t, &bad, &bad_id);
    if (e != want || bad != index || !t.slots.empty()) fail(name, "status, index or a table built");
    std::printf("%-28s %-6s refused at merge %u (error %d)\n", name, wide ? "wide" : "narrow", bad, (int)e);
}

}  // namespace

int main() {
    const uint32_t A = 'a', B = 'b', C = 'c', MAX = ME_WIDE_MAX_ID;
    const std::vector<Case> wide_cases = {
        // (0x10001, 5) and (1, 5): the same 16-bit-packed key
        {"packed_key_a_overflows", {A, B, 0x10001, 0x10001, 5, 0x20000, 1, 5, 0x20001}, std::string("ab\x05\x01\x05", 5),
         {0x20000, 0x20001}, 3},
        // (2, 0x10007) and (3, 7): b's high bits bleed into a
        {"packed_key_b_bleeds", {A, B, 0x10007, 2, 0x10007, 0x300, 3, 7, 0x301}, std::string("\x02" "ab\x03\x07", 5),
         {0x300, 0x301}, 3},
        {"a_differs_in_bits_16_23", {A, B, 0x010100, B, A, 0x020100, 0x010100, 5, 0x400, 0x020100, 5, 0x401},
         std::string("ab\x05" "ba\x05", 6), {0x400, 0x401}, 4},
        {"b_differs_in_bits_16_23", {A, B, 0x010100, B, A, 0x020100, 3, 0x010100, 0x400, 3, 0x020100, 0x401},
         std::string("\x03" "ab\x03" "ba", 6), {0x400, 0x401}, 4},
        // 0xFFFF, 0x10000 and the largest id as a new id and as an operand that fires
        {"boundary_ids", {A, B, 0xFFFF, B, A, 0x10000, A, A, MAX, 0xFFFF, C, 0x500, 0x10000, C, 0x501, MAX, C, 0x502},
         "abcbacaac", {0x500, 0x501, 0x502}, 6},
        {"max_id_both_operands", {A, B, MAX, MAX, MAX, MAX - 1, MAX - 1, MAX, 0x100}, "ababab", {0x100}, 3},
        {"no_merges", {}, std::string("a\0\0", 3), {A, 0, 0}, 0},
    };
    for (const Case& c : wide_cases) run(c, true);
    // lists that fit 16 bits give the same tokens in both layouts
    const std::vector<Case> both = {
        {"nul_nul", {0, 0, 256}, std::string("\0\0\0", 3), {256, 0}, 1},
        {"ffff_operand", {A, B, 0xFFFF, 0xFFFF, 0xFFFF, 256, 0xFFFF, A, 257}, "ababa", {256, A}, 3},
        {"repeated_pair_dead_id", {A, B, 300, A, B, 301, 301, C, 302, 300, C, 303}, "abc", {303}, 2},
        {"operand_created_later", {300, C, 301, A, B, 300}, "abc", {300, C}, 1},
    };
    for (const Case& c : both) run(c, false), run(c, true);
    rejected("a_above_wide_bound", {MAX + 1, B, 256}, MAX, true, ME_BUILD_RANGE, 0);
    rejected("b_above_wide_bound", {A, B, 256, A, MAX + 1, 257}, MAX, true, ME_BUILD_RANGE, 1);
    rejected("id_above_wide_bound", {A, B, 256, B, B, 257, A, A, MAX + 1}, MAX, true, ME_BUILD_RANGE, 2);
    rejected("id_0xFFFFFFFF", {A, B, 0xFFFFFFFFu}, MAX, true, ME_BUILD_RANGE, 0);
    rejected("narrow_0x10000", {A, B, 256, A, A, 0x10000}, ME_NARROW_MAX_ID, false, ME_BUILD_RANGE, 1);
    rejected("new_id_255", {A, B, 256, 256, A, 255}, MAX, true, ME_BUILD_BYTE_ID, 1);
    rejected("repeated_wide_id", {A, B, 0x10000, B, A, 257, A, A, 0x10000}, MAX, true, ME_BUILD_REPEATED_ID, 2);
    rejected("repeated_after_missing", {9000, A, MAX, A, B, 256, B, B, MAX}, MAX, true, ME_BUILD_REPEATED_ID, 2);
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
