// Merge-rank BPE encode on MI355X: TokenizerManager.encode
// (src/bpe/tokenizer/tokenizer-manager.js:13-61), the UI tab's encoder.
//
// The reference applies every learned merge in order to the whole byte string
// (one left-to-right pass per merge).  Two facts make that parallel and exact:
//   * a merge's new pairs involve its new token, whose id is only used by
//     later merges — so applying ranks in order equals repeatedly applying the
//     lowest-rank adjacent pair (all its occurrences, left to right);
//   * a token can only ever span the boundary between bytes (u, v) if some
//     merge (a, b) has last(a) = u and first(b) = v.  Every other boundary is a
//     cut no merge crosses, so the text splits into independent segments.
// A merge whose operand is created by a LATER merge (or never) never fires in
// the reference; such merges are dropped on upload, as are repeated pairs
// (the first rank wins, tokenizer-manager.js:30-33).
// Both facts need every new id to be fresh: at least 256 and given by one entry of the
// list only.  An id that was in the stream before (a byte's, an earlier entry's) lets a
// later rank's merge feed an earlier one's pair, and has no single first and last byte;
// the uploads reject such a list (GBPE_E_INVALID).  On every other list the result
// is exact, the pair (0,0) included: a slot's .w, not its key, says that it is occupied.
//
// The pipeline (me_run): the mask of the call → k_me_long → the walk → scan.h's two-level scan of the
// chunks' token counts → k_me_compact (and k_me_tok_off, the documents' token offsets).
//
// The walk (me_walk): one lane per chunk of CS bytes.  A lane owns the segments that START in its
// chunk (the last may run past the chunk's end), copies each into scratch at the place of its bytes
// and BPE-encodes it there: me_short, one pass per rank applied, rank lookups in an L2-resident
// open-addressing table.  The walk exists once; five template switches make its instantiations:
//   WORDS  a byte mask of word starts adds cuts, so that the result is the
//          concatenation of each word's own encoding; without it the whole string is one text.
//   CS     4096 without a mask.  Words are a few bytes long, so with one a lane's range and not
//          its segments sets the serial length: 4096, 1024 or 256 (GBPE_DEBUG me_cs; ME_CS_WORDS ships).
//   DOCS   many documents in one call: a document start is one more cut, and the lane
//          notes how many tokens it had written at each; k_me_tok_off adds the chunk's prefix.
//   SP     special tokens: special.hip marks the accepted matches, and a match's span
//          is one segment whose one token is the special's id.
//   WIDE   ids above 0xFFFF: the table's slot carries both full operands,
//          {a, b, rank, new id}, and a pair is keyed by 64 bits; the narrow form keeps a << 16 | b
//          in one word.  merge_table.h builds either table on the host and holds the hash both
//          sides share.  me_heap is the other reader of the slots and takes the same switch.
//   SPANS  the byte span of every token: scratch holds {token, its start relative to
//          the chunk's base} pairs; me_short_spans carries the pair through its compaction, me_heap
//          writes a surviving node's index, a special's span its own start.
// Three __global__ symbols carry it: k_me_walk<WORDS, CS, WIDE> (no DOCS, no SP),
// k_me_walk_docs<CS, SP, WIDE> (WORDS and DOCS: a call with special tokens is launched as a batch
// of no documents) and k_me_walk_spans<CS, SP, WIDE> (WORDS, DOCS and SPANS: a call without
// documents or word starts runs under a mask of its own, zero for GBPE_WORDS_NONE).  me_launch is
// the one place that picks an instantiation.
//
// The long-segment arena: a segment longer than ME_LONG bytes (CJK paragraphs, base64, minified
// code: no cut for a long stretch) would cost its lane one full pass per rank applied; it is encoded
// with a rank-ordered heap over a linked list instead (me_heap: O(len log len), same order: lowest
// rank first, leftmost first).  k_me_long runs before the walk, finds those segments with the walk's
// own cut predicate (me_cut), and gives each an offset into an arena sized by their total length.
//
// The mask bits: a caller's mask or a mode's is 0 / nonzero per byte.  A batch call and a call with
// special tokens build their own (me_mask): bit 0 a word start within a document or a piece between
// specials, ME_DOC_BIT a document start, ME_SP_BIT / ME_SPIN_BIT a special's first / other bytes
// (k_me_sp_mask).  Any nonzero byte but ME_SPIN_BIT alone is a cut.

#include "common.h"
#include "merge_table.h"
#include "scan.h"

#include <type_traits>

#include <vector>

namespace {

constexpr int ME_TPB = 64;
constexpr uint32_t ME_CS = 4096;      // bytes per chunk (a lane's range of segment starts)
constexpr uint32_t ME_NONE = 0xFFFFFFFFu;
constexpr uint32_t ME_LONG = 1024;                  // longer segments take the heap path
// long segments that can start in one chunk of CS bytes: starts at least ME_LONG + 1 apart,
// so at most (CS - 1) / (ME_LONG + 1) + 1 <= CS / ME_LONG + 1 of them, under any cut predicate
constexpr uint32_t me_lslot(uint32_t cs) { return cs / ME_LONG + 1; }
constexpr uint32_t ME_CS_WORDS = 256;   // shipped chunk size of the word-bounded encode
constexpr uint32_t ME_DEAD = 0xFFFFFFFFu;

struct MeArena {   // per long segment at offset `off` (bytes of all long segments before it)
    uint32_t* tok;       // [off, off + len)
    uint32_t* nxt;
    uint32_t* prv;
    uint64_t* heap;      // [3 off, 3 (off + len)): initial pairs + two per merge
    const uint64_t* slot;   // per chunk: me_lslot(CS) offsets of the long segments starting in it
};

// merge_table.h's table.  Narrow slots (ids <= 0xFFFF) are {pid, rank, new id, occupied}, wide ones
//  {a, b, rank, new id}; .w 0 = empty in both (the pair (0,0) is a merge like any other)
struct MeTable {
    const uint4* slots;
    uint32_t mask;
    const uint32_t* cross;   // 65536-bit: (u << 8 | v) set iff some merge joins a token ending in u to one starting with v
};

// An adjacent pair as the walks look it up and remember it.  WIDE is a template parameter of every
// kernel that reads the slots: the narrow instantiations keep the one-word key a << 16 | b.
template <bool WIDE>
using me_key_t = std::conditional_t<WIDE, uint64_t, uint32_t>;

template <bool WIDE>
__device__ __forceinline__ me_key_t<WIDE> me_pair(uint32_t a, uint32_t b) {
    return ((me_key_t<WIDE>)a << (WIDE ? 32 : 16)) | b;
}

// {_, rank, new id, _} of the pair; rank ME_NONE: no such merge.  Overloaded on the key: the narrow
// lookup is the one the encoder has always had, the wide one tests the same word first (.w) and
// compares both operands.  merge_table.h's host build probes the same way.
__device__ __forceinline__ uint4 me_find(const MeTable& t, uint32_t pid) {
    uint32_t h = me_hash_narrow(pid) & t.mask;
    for (uint32_t p = 0; p <= t.mask; ++p) {
        const uint32_t idx = me_probe(h, p, t.mask);
        const uint4 e = t.slots[idx];
        if (e.w == 0u) break;   // (tested first: an empty slot's pid reads 0, the pair (0,0))
        if (e.x == pid) return e;
    }
    return make_uint4(0u, ME_NONE, 0u, 0u);
}

__device__ __forceinline__ uint4 me_find(const MeTable& t, uint64_t key) {
    const uint32_t a = (uint32_t)(key >> 32), b = (uint32_t)key;
    uint32_t h = me_hash_wide(a, b) & t.mask;
    for (uint32_t p = 0; p <= t.mask; ++p) {
        const uint4 e = t.slots[me_probe(h, p, t.mask)];
        if (e.w == 0u) break;
        if (e.x == a && e.y == b) return make_uint4(0u, e.z, e.w, 1u);
    }
    return make_uint4(0u, ME_NONE, 0u, 0u);
}

// Bits of a mask byte the library builds itself (a batch call, a call with special tokens): bit 0
// a word start, ME_DOC_BIT a document start, ME_SP_BIT the first byte of an accepted
// special token, ME_SPIN_BIT its other bytes.
constexpr uint32_t ME_DOC_BIT = 2u, ME_SP_BIT = 4u, ME_SPIN_BIT = 8u;

// a segment starts at byte i: a word start (WORDS), or no merge crosses (i - 1, i).  SP: never
// inside a special, whatever the pair says — a lane whose chunk begins there must skip to its end.
// With `w`, the mask byte goes back to the caller: the walk tests the byte of a segment's start
// without loading it again.  This is the one predicate of k_me_long and of the walk: k_me_long's
// arena offsets are the walk's only if both cut at the same bytes, so neither gets a form of its own.
template <bool WORDS, bool SP = false>
__device__ __forceinline__ bool me_cut(const uint8_t* __restrict__ in, const uint8_t* __restrict__ ws, const MeTable& t,
                                       uint64_t i, uint32_t* w = nullptr) {
    if (w) *w = ws[i];   // (before the test of i: the walk wants the byte at 0 as well)
    if (i == 0) return true;
    if (WORDS) {
        const uint32_t m = w ? *w : ws[i];
        if (m) return !SP || m != ME_SPIN_BIT;   // (k_me_sp_mask leaves that bit alone on a span's inner bytes)
    }
    const uint32_t k = ((uint32_t)in[i - 1] << 8) | in[i];
    return ((t.cross[k >> 5] >> (k & 31u)) & 1u) == 0u;
}

// the long segments (> ME_LONG bytes) starting in each chunk: arena offsets (a special's span is a
// segment of at most 128 bytes: never long)
template <bool WORDS, uint32_t CS, bool SP = false>
__global__ __launch_bounds__(ME_TPB) void k_me_long(const uint8_t* __restrict__ in, const uint8_t* __restrict__ ws,
                                                    uint64_t n, MeTable t, unsigned long long* __restrict__ total,
                                                    uint64_t* __restrict__ slot, uint64_t nchunks) {
    const uint64_t c = (uint64_t)blockIdx.x * ME_TPB + threadIdx.x;
    if (c >= nchunks) return;
    const uint64_t lo = c * CS, hi = min(lo + CS, n);
    uint64_t s = lo;
    while (s < hi && !me_cut<WORDS, SP>(in, ws, t, s)) ++s;
    uint32_t k = 0;
    while (s < hi) {
        uint64_t z = s + 1;
        while (z < n && !me_cut<WORDS, SP>(in, ws, t, z)) ++z;
        if (z - s > ME_LONG) slot[c * me_lslot(CS) + k++] = atomicAdd(total, (unsigned long long)(z - s));
        s = z;
    }
}

// one long segment on one lane: a min-heap of (rank << 32 | position) over the
// adjacent pairs of a doubly linked token list.  Popping the lowest rank, then
// the leftmost position, applies every merge in rank order and each rank's
// occurrences left to right, as the reference's one pass per merge does: a
// merge's new pairs hold its new token, which only later ranks use.  Stale
// entries (the pair at that position changed) are skipped on pop.
// SPANS: `out` is an array of uint2, {token, rel + the index of its node}: the node's index is its
// token's first byte.
template <bool WIDE, bool SPANS = false>
__device__ uint32_t me_heap(const uint8_t* __restrict__ in, uint32_t len, const MeTable& t, uint32_t* __restrict__ tk,
                            uint32_t* __restrict__ nx, uint32_t* __restrict__ pv, uint64_t* __restrict__ hp,
                            uint32_t* __restrict__ out, uint32_t rel = 0) {
    for (uint32_t i = 0; i < len; ++i) {
        tk[i] = in[i];
        nx[i] = i + 1;
        pv[i] = i ? i - 1 : ME_NONE;
    }
    uint32_t h = 0;
    auto push = [&](uint64_t key) {
        uint32_t i = h++;
        while (i) {
            const uint32_t p = (i - 1) >> 1;
            if (hp[p] <= key) break;
            hp[i] = hp[p];
            i = p;
        }
        hp[i] = key;
    };
    auto rank_at = [&](uint32_t i, uint32_t j) -> uint4 { return me_find(t, me_pair<WIDE>(tk[i], tk[j])); };
    for (uint32_t i = 0; i + 1 < len; ++i) {
        const uint4 e = rank_at(i, i + 1);
        if (e.y != ME_NONE) push(((uint64_t)e.y << 32) | i);
    }
    while (h) {
        const uint64_t key = hp[0];
        const uint64_t last = hp[--h];
        if (h) {   // sift the last entry down from the root
            uint32_t i = 0;
            for (;;) {
                uint32_t c = 2 * i + 1;
                if (c >= h) break;
                if (c + 1 < h && hp[c + 1] < hp[c]) ++c;
                if (last <= hp[c]) break;
                hp[i] = hp[c];
                i = c;
            }
            hp[i] = last;
        }
        const uint32_t r = (uint32_t)(key >> 32), i = (uint32_t)key;
        if (tk[i] == ME_DEAD) continue;
        const uint32_t j = nx[i];
        if (j >= len) continue;
        const uint4 e = rank_at(i, j);
        if (e.y != r) continue;   // stale: the pair at i changed
        tk[i] = e.z;
        tk[j] = ME_DEAD;
        const uint32_t q = nx[j];
        nx[i] = q;
        if (q < len) pv[q] = i;
        const uint32_t p = pv[i];
        if (p != ME_NONE) {
            const uint4 ep = rank_at(p, i);
            if (ep.y != ME_NONE) push(((uint64_t)ep.y << 32) | p);
        }
        if (q < len) {
            const uint4 eq = rank_at(i, q);
            if (eq.y != ME_NONE) push(((uint64_t)eq.y << 32) | i);
        }
    }
    uint32_t cnt = 0;
    if constexpr (SPANS) {
        uint2* out2 = reinterpret_cast<uint2*>(out);
        for (uint32_t i = 0; i < len; i = nx[i]) out2[cnt++] = make_uint2(tk[i], rel + i);
        return cnt;
    }
    for (uint32_t i = 0; i < len; i = nx[i]) out[cnt++] = tk[i];   // position 0 is never merged away
    return cnt;
}

// one short segment (at most ME_LONG tokens) in place: the lowest rank among its adjacent pairs,
// every occurrence, left to right, until no pair has a rank.  Returns the new length.
// The shape of the two loops is a measured one ("The short-segment loop"): as a function,
// the text the kernels used to hold compiled to two more scalar instructions in the second loop and
// ran 0.6 - 1.9 % slower at 1024 and 256 bytes per lane; this form is not slower on any leg.
template <bool WIDE>
__device__ __forceinline__ uint32_t me_short(uint32_t* tok, uint32_t len, const MeTable& t) {
    if (len >= 2) do {
        uint32_t best = ME_NONE;
        me_key_t<WIDE> bpid = 0;
        uint32_t bnew = 0;
        for (uint32_t j = 0; j + 1 < len; ++j) {
            const me_key_t<WIDE> pid = me_pair<WIDE>(tok[j], tok[j + 1]);
            const uint4 e = me_find(t, pid);
            if (e.y < best) { best = e.y; bpid = pid; bnew = e.z; }
        }
        if (best == ME_NONE) break;
        uint32_t w = 0, j = 0;
        while (j < len) {
            uint32_t v = tok[j++];
            if (j < len && me_pair<WIDE>(v, tok[j]) == bpid) {
                v = bnew;
                ++j;
            }
            tok[w++] = v;   // (w < j: behind what is still to be read)
        }
        len = w;
    } while (len >= 2);
    return len;
}

// me_short on {token, start} pairs (SPANS): the same two loops, and a token's start moves
// with it — a merged pair keeps its left operand's.  One 8-byte element and not two arrays: the walk is
// bound by its lanes' scattered loads and stores, and a pair costs the second loop no more of them.
template <bool WIDE>
__device__ __forceinline__ uint32_t me_short_spans(uint2* tok, uint32_t len, const MeTable& t) {
    if (len >= 2) do {
        uint32_t best = ME_NONE;
        me_key_t<WIDE> bpid = 0;
        uint32_t bnew = 0;
        for (uint32_t j = 0; j + 1 < len; ++j) {
            const me_key_t<WIDE> pid = me_pair<WIDE>(tok[j].x, tok[j + 1].x);
            const uint4 e = me_find(t, pid);
            if (e.y < best) { best = e.y; bpid = pid; bnew = e.z; }
        }
        if (best == ME_NONE) break;
        uint32_t w = 0, j = 0;
        while (j < len) {
            uint2 v = tok[j++];
            if (j < len && me_pair<WIDE>(v.x, tok[j].x) == bpid) {
                v.x = bnew;
                ++j;
            }
            tok[w++] = v;   // (w < j: behind what is still to be read)
        }
        len = w;
    } while (len >= 2);
    return len;
}

// the first document whose offset is p (p is one of doc_off[0, n_docs))
__device__ __forceinline__ uint64_t me_first_doc(const uint64_t* __restrict__ doc_off, uint64_t n_docs, uint64_t p) {
    uint64_t lo = 0, hi = n_docs;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (doc_off[mid] < p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Per-document token offsets of the batch call: bit 1 of a mask byte
// says a document starts there.  A document start is a segment start of the chunk that
// holds it, so its first token is that chunk's scanned prefix plus what the chunk's lane
// had written when it got there: doc_written[first document at that offset].
struct MeDocs {
    const uint64_t* doc_off;
    uint64_t n_docs;
    uint32_t* written;
};
struct MeSp {   // the special tokens of a call (SP)
    const uint8_t* mark;   // gbpe_specials_mark's array
    const uint32_t* ids;   // by index
};

// The walk: one lane per chunk of CS bytes encodes the segments that start in its chunk, each in
// place in scratch, and counts its tokens.  DOCS: also the tokens written before each document
// start.  SP: a segment that begins with ME_SP_BIT is a special's span (its other bytes are no cut,
// the byte after it is one): its id is the segment's one token.  It belongs to the chunk that holds
// its first byte, and one token for at least one byte keeps the tokens of a chunk behind the bytes
// it has consumed.  SPANS: scratch is an array of uint2, and entry b0 + k is the chunk's k-th token
// with its first byte, less b0.
template <bool WORDS, uint32_t CS, bool DOCS, bool SP, bool WIDE, bool SPANS = false>
__device__ __forceinline__ void me_walk(const uint8_t* __restrict__ in, const uint8_t* __restrict__ ws, uint64_t n,
                                        const MeTable& t, uint32_t* __restrict__ scratch, uint32_t* __restrict__ counts,
                                        uint64_t* __restrict__ base, uint64_t nchunks, const MeArena& ar,
                                        const MeDocs& docs, const MeSp& sp) {
    const uint64_t c = (uint64_t)blockIdx.x * ME_TPB + threadIdx.x;
    if (c >= nchunks) return;
    const uint64_t lo = c * CS, hi = min(lo + CS, n);
    uint64_t s = lo;
    uint32_t ws_s = 0, ws_z = 0;   // (SP) the mask bytes at s and at z
    while (s < hi && !me_cut<WORDS, SP>(in, ws, t, s, SP ? &ws_s : nullptr)) ++s;   // first segment start in the chunk
    base[c] = s;
    const uint64_t b0 = s;   // this chunk's tokens go to scratch[b0 ...]: never past the bytes consumed
    uint32_t written = 0, nlong = 0;
    while (s < hi) {
        uint64_t z = s + 1;
        while (z < n && !me_cut<WORDS, SP>(in, ws, t, z, SP ? &ws_z : nullptr)) ++z;   // the segment [s, z) may run past hi
        if constexpr (DOCS) {
            const uint32_t w0 = SP ? ws_s : ws[s];
            ws_s = ws_z;   // (z == n: not read, and the loop ends)
            if (w0 & ME_DOC_BIT) docs.written[me_first_doc(docs.doc_off, docs.n_docs, s)] = written;
            if (SP && (w0 & ME_SP_BIT)) {
                if constexpr (SPANS)
                    reinterpret_cast<uint2*>(scratch)[b0 + written++] = make_uint2(sp.ids[sp.mark[s] - 1u], (uint32_t)(s - b0));
                else
                    scratch[b0 + written++] = sp.ids[sp.mark[s] - 1u];
                s = z;
                continue;
            }
        }
        uint32_t* tok = scratch + b0 + written;
        const uint32_t len = (uint32_t)(z - s);
        if constexpr (SPANS) {
            uint2* tp = reinterpret_cast<uint2*>(scratch) + b0 + written;
            const uint32_t rel = (uint32_t)(s - b0);   // (below CS: s and b0 lie in the chunk)
            if (len > ME_LONG) {
                const uint64_t off = ar.slot[c * me_lslot(CS) + nlong++];
                written += me_heap<WIDE, true>(in + s, len, t, ar.tok + off, ar.nxt + off, ar.prv + off, ar.heap + 3 * off,
                                               reinterpret_cast<uint32_t*>(tp), rel);
            } else {
                for (uint32_t j = 0; j < len; ++j) tp[j] = make_uint2(in[s + j], rel + j);
                written += me_short_spans<WIDE>(tp, len, t);
            }
            s = z;
            continue;
        }
        if (len > ME_LONG) {
            const uint64_t off = ar.slot[c * me_lslot(CS) + nlong++];
            written += me_heap<WIDE>(in + s, len, t, ar.tok + off, ar.nxt + off, ar.prv + off, ar.heap + 3 * off, tok);
        } else {
            for (uint32_t j = 0; j < len; ++j) tok[j] = in[s + j];
            written += me_short<WIDE>(tok, len, t);
        }
        s = z;
    }
    counts[c] = written;
}

// The walk's two symbols: without and with the documents' and specials' arguments.
template <bool WORDS, uint32_t CS, bool WIDE = false>
__global__ __launch_bounds__(ME_TPB) void k_me_walk(const uint8_t* __restrict__ in, const uint8_t* __restrict__ ws,
                                                    uint64_t n, MeTable t, uint32_t* __restrict__ scratch,
                                                    uint32_t* __restrict__ counts, uint64_t* __restrict__ base,
                                                    uint64_t nchunks, MeArena ar) {
    me_walk<WORDS, CS, false, false, WIDE>(in, ws, n, t, scratch, counts, base, nchunks, ar, MeDocs{}, MeSp{});
}

template <uint32_t CS, bool SP = false, bool WIDE = false>
__global__ __launch_bounds__(ME_TPB) void k_me_walk_docs(const uint8_t* __restrict__ in, const uint8_t* __restrict__ ws,
                                                         uint64_t n, MeTable t, uint32_t* __restrict__ scratch,
                                                         uint32_t* __restrict__ counts, uint64_t* __restrict__ base,
                                                         uint64_t nchunks, MeArena ar, MeDocs docs, MeSp sp) {
    me_walk<true, CS, true, SP, WIDE>(in, ws, n, t, scratch, counts, base, nchunks, ar, docs, sp);
}

// the spans form: the word and document walk on {token, start} pairs (scratch: n uint2)
template <uint32_t CS, bool SP = false, bool WIDE = false>
__global__ __launch_bounds__(ME_TPB) void k_me_walk_spans(const uint8_t* __restrict__ in, const uint8_t* __restrict__ ws,
                                                          uint64_t n, MeTable t, uint32_t* __restrict__ scratch,
                                                          uint32_t* __restrict__ counts, uint64_t* __restrict__ base,
                                                          uint64_t nchunks, MeArena ar, MeDocs docs, MeSp sp) {
    me_walk<true, CS, true, SP, WIDE, true>(in, ws, n, t, scratch, counts, base, nchunks, ar, docs, sp);
}

// the caller's mask as 0 / 1 (any alignment), four bytes per lane: bit 1 stays free for the document starts
__global__ __launch_bounds__(256) void k_me_mask01(const uint8_t* __restrict__ ws, uint64_t n, uint8_t* __restrict__ m) {
    const uint64_t i = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 4 <= n) {
        uint32_t v = 0;
        for (int k = 0; k < 4; ++k) v |= (ws[i + k] != 0 ? 1u : 0u) << (8 * k);
        *reinterpret_cast<uint32_t*>(m + i) = v;   // (m is a pooled block: aligned)
    } else {
        for (uint64_t j = i; j < n; ++j) m[j] = ws[j] != 0;
    }
}

// The accepted specials into the mode's 0 / 1 mask, 16 bytes per lane: a special's
// first byte becomes `word start | ME_SP_BIT`, its other bytes ME_SPIN_BIT alone (whatever the
// mode's mask held under the span goes), and the byte after its last is a word start.  Runs
// before the document starts are ORed in; mark and m are pooled blocks (16-byte aligned).
__global__ __launch_bounds__(256) void k_me_sp_mask(const uint8_t* __restrict__ mark, uint64_t n, uint8_t* __restrict__ m) {
    const uint64_t i0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (i0 >= n) return;
    uint32_t prev = i0 ? mark[i0 - 1] : 0u;
    if (i0 + 16 <= n) {
        const uint4 kv = *reinterpret_cast<const uint4*>(mark + i0);
        const uint32_t k4[4] = {kv.x, kv.y, kv.z, kv.w};
        if ((kv.x | kv.y | kv.z | kv.w | prev) == 0u) return;   // no special here: the mask stands
        const uint4 mv = *reinterpret_cast<const uint4*>(m + i0);
        uint32_t m4[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t sh = 8 * (k & 3);
            const uint32_t mk = (k4[k / 4] >> sh) & 0xFFu;
            uint32_t v = (m4[k / 4] >> sh) & 0xFFu;
            if (mk == 255u) v = ME_SPIN_BIT;
            else if (mk) v = 1u | ME_SP_BIT;
            else if (prev) v |= 1u;
            m4[k / 4] = (m4[k / 4] & ~(0xFFu << sh)) | (v << sh);
            prev = mk;
        }
        *reinterpret_cast<uint4*>(m + i0) = make_uint4(m4[0], m4[1], m4[2], m4[3]);
    } else {
        for (uint64_t i = i0; i < n; ++i) {
            const uint32_t mk = mark[i];
            if (mk == 255u) m[i] = ME_SPIN_BIT;
            else if (mk) m[i] = 1u | ME_SP_BIT;
            else if (prev) m[i] |= 1u;
            prev = mk;
        }
    }
}

// one lane per document and one for the closing entry: a document that starts inside the
// bytes begins at its chunk's prefix + what the walk stored for the first document at its
// offset (empty documents share it); one that starts at n begins at the total
__global__ __launch_bounds__(256) void k_me_tok_off(const uint64_t* __restrict__ doc_off, uint64_t n_docs, uint64_t n,
                                                    uint32_t cs, const uint32_t* __restrict__ doc_written,
                                                    const uint32_t* __restrict__ local,
                                                    const uint64_t* __restrict__ blocksum,
                                                    const uint64_t* __restrict__ total, uint64_t* __restrict__ tok_off) {
    const uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (d > n_docs) return;
    const uint64_t p = d < n_docs ? doc_off[d] : n;
    if (p >= n) {
        tok_off[d] = *total;
        return;
    }
    const uint64_t d0 = (d == 0 || doc_off[d - 1] < p) ? d : me_first_doc(doc_off, n_docs, p);
    const uint64_t c = p / cs;
    tok_off[d] = blocksum[c / SCAN_BLK] + local[c] + doc_written[d0];
}

__global__ __launch_bounds__(256) void k_me_compact(const uint32_t* __restrict__ scratch,
                                                    const uint32_t* __restrict__ counts,
                                                    const uint64_t* __restrict__ base, const uint32_t* __restrict__ local,
                                                    const uint64_t* __restrict__ blocksum, uint64_t nchunks,
                                                    uint32_t* __restrict__ out, uint64_t out_cap) {
    const uint64_t chunk = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= nchunks) return;
    const int lane = threadIdx.x & 63;
    const uint64_t off = blocksum[chunk / SCAN_BLK] + local[chunk];
    const uint32_t cnt = counts[chunk];
    const uint32_t* src = scratch + base[chunk];
    for (uint32_t j = lane; j < cnt; j += 64) {
        const uint64_t d = off + j;
        if (d < out_cap) out[d] = src[j];
    }
}

// the spans form: scratch holds {token, relative start}; tok_start[d] = the chunk's base + the start, beside out[d]
__global__ __launch_bounds__(256) void k_me_compact_spans(const uint2* __restrict__ scratch,
                                                          const uint32_t* __restrict__ counts,
                                                          const uint64_t* __restrict__ base,
                                                          const uint32_t* __restrict__ local,
                                                          const uint64_t* __restrict__ blocksum, uint64_t nchunks,
                                                          uint32_t* __restrict__ out, uint64_t* __restrict__ tok_start,
                                                          uint64_t out_cap) {
    const uint64_t chunk = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= nchunks) return;
    const int lane = threadIdx.x & 63;
    const uint64_t off = blocksum[chunk / SCAN_BLK] + local[chunk];
    const uint32_t cnt = counts[chunk];
    const uint64_t b0 = base[chunk];
    for (uint32_t j = lane; j < cnt; j += 64) {
        const uint64_t d = off + j;
        if (d < out_cap) {
            const uint2 v = scratch[b0 + j];
            out[d] = v.x;
            tok_start[d] = b0 + v.y;
        }
    }
}

}  // namespace

struct gbpe_bpe {
    gbpe_ctx* ctx = nullptr;
    uint4* slots = nullptr;
    uint32_t mask = 0;
    uint32_t* cross = nullptr;
    uint32_t n_live = 0;
    bool wide = false;   // the slots' layout, and so the walks' instantiation
};

static_assert(sizeof(MeSlot) == sizeof(uint4), "merge_table.h's slot is the device's uint4");
static_assert(ME_WIDE_MAX_ID == GBPE_BPE_MAX_ID, "merge_table.h's bound is the header's");

// both uploads: merge_table.h's filter and table on the host, then the copies
static int me_upload(gbpe_ctx* ctx, const uint32_t* merges, uint32_t n_merges, bool wide, gbpe_bpe** out) {
    if (!ctx || !out || (n_merges && !merges)) return gbpe_set_error(ctx, GBPE_E_INVALID, "bpe upload: bad arguments");
    *out = nullptr;
    const uint32_t max_id = wide ? ME_WIDE_MAX_ID : ME_NARROW_MAX_ID;
    MeHostTable tab;
    uint32_t bad = 0, bad_id = 0;
    switch (me_build_table(merges, n_merges, max_id, wide, &tab, &bad, &bad_id)) {
    case ME_BUILD_OK: break;
    case ME_BUILD_RANGE:
        return gbpe_set_error(ctx, GBPE_E_INVALID, "bpe upload: merge %u has an id above 0x%X", bad, max_id);
    case ME_BUILD_BYTE_ID:
        return gbpe_set_error(ctx, GBPE_E_INVALID, "bpe upload: merge %u has the new id %u, a byte's", bad, bad_id);
    case ME_BUILD_REPEATED_ID:
        return gbpe_set_error(ctx, GBPE_E_INVALID, "bpe upload: merge %u gives the new id %u a second time", bad, bad_id);
    }
    auto* bp = new (std::nothrow) gbpe_bpe();
    if (!bp) return gbpe_set_error(ctx, GBPE_E_OOM, "host allocation failed");
    bp->ctx = ctx;
    bp->mask = (uint32_t)tab.slots.size() - 1;
    bp->n_live = tab.live;
    bp->wide = wide;
    const size_t slot_bytes = tab.slots.size() * sizeof(uint4), cross_bytes = tab.cross.size() * sizeof(uint32_t);
    hipError_t e = dev_malloc(ctx, &bp->slots, slot_bytes);
    if (e == hipSuccess) e = dev_malloc(ctx, &bp->cross, cross_bytes);
    if (e == hipSuccess) e = hipMemcpy(bp->slots, tab.slots.data(), slot_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(bp->cross, tab.cross.data(), cross_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(bp->slots);
        hipFree(bp->cross);
        delete bp;
        return gbpe_set_error(ctx, GBPE_E_DEVICE, "bpe upload failed: %s", hipGetErrorString(e));
    }
    *out = bp;
    return GBPE_OK;
}

extern "C" int gbpe_bpe_upload(gbpe_ctx* ctx, const uint32_t* merges, uint32_t n_merges, gbpe_bpe** out) {
    return me_upload(ctx, merges, n_merges, false, out);
}

extern "C" int gbpe_bpe_upload_wide(gbpe_ctx* ctx, const uint32_t* merges, uint32_t n_merges, gbpe_bpe** out) {
    return me_upload(ctx, merges, n_merges, true, out);
}

extern "C" void gbpe_bpe_free(gbpe_bpe* bp) {
    if (!bp) return;
    hipFree(bp->slots);
    hipFree(bp->cross);
    delete bp;
}

// ── the pipeline on device buffers: one driver for every entry point ──

namespace {

inline uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

struct MeWork {   // the device arrays of one call, each 16-byte aligned inside one pooled block
    uint32_t* scratch;    // n: a chunk's tokens from its first segment start (<= 1 per byte); spans: n uint2
    uint32_t* counts;     // nchunks
    uint64_t* base;       // nchunks
    uint32_t* local;      // nchunks
    uint64_t* blocksum;   // nblk + 1, then the token total
    uint64_t* total;
    uint64_t* slot;       // nchunks * me_lslot(cs): arena offsets of the long segments
    unsigned long long* back;   // 16 bytes read back after k_me_long: the long-segment total, the offsets' verdict
    // a batch call (n_docs > 0) or one with special tokens only
    uint32_t* doc_written;   // n_docs
    uint8_t* mask;           // n
    uint8_t* flags;          // n, when asked for: the document starts (GPT-4 rules: and the specials' edges)
    // special tokens only
    uint8_t* mark;           // n: gbpe_specials_mark's array
    uint8_t* cand;           // n
    // a spans call: scratch holds uint2 {token, start}, entry base[c] + k being chunk c's k-th
    // token and its first byte less base[c].  A token starts inside a segment that starts in the chunk, so
    // the start is below CS + the chunk's longest segment.  The walk holds a segment's length in 32 bits;
    // the entry points keep n at most ME_SPANS_MAX_N = 2^32 - 1 - 4096, so the sum cannot wrap a u32 either.
    bool spans;
};
constexpr uint64_t ME_SPANS_MAX_N = 0xFFFFFFFFull - 4096u;

hipError_t me_layout(gbpe_ctx* ctx, GbpeArray<uint8_t>& blk, uint64_t n, uint32_t cs, uint64_t nchunks, uint64_t nblk,
                     uint64_t n_docs, bool flags, bool special, bool spans, MeWork* w) {
    const uint64_t o_counts = up16((spans ? 8 : 4) * n), o_base = o_counts + up16(4 * nchunks), o_local = o_base + up16(8 * nchunks);
    const uint64_t o_bsum = o_local + up16(4 * nchunks), o_slot = o_bsum + up16(8 * (nblk + 2));
    const uint64_t o_back = o_slot + up16(8 * nchunks * me_lslot(cs)), o_docw = o_back + 16;
    const uint64_t o_mask = o_docw + up16(4 * n_docs), o_flags = o_mask + up16(n), o_mark = o_flags + (flags ? up16(n) : 0);
    const uint64_t o_end = o_mark + (special ? 2 * up16(n) : 0);
    const hipError_t e = blk.reserve(ctx, (n_docs || special ? o_end : o_back) + 16);
    if (e != hipSuccess) return e;
    uint8_t* p = blk.p;
    *w = MeWork{(uint32_t*)p, (uint32_t*)(p + o_counts), (uint64_t*)(p + o_base), (uint32_t*)(p + o_local),
                (uint64_t*)(p + o_bsum), (uint64_t*)(p + o_bsum) + nblk + 1, (uint64_t*)(p + o_slot),
                (unsigned long long*)(p + o_back), nullptr, nullptr, nullptr, nullptr, nullptr, spans};
    if (n_docs || special) w->doc_written = (uint32_t*)(p + o_docw), w->mask = p + o_mask;
    if (flags) w->flags = p + o_flags;
    if (special) w->mark = p + o_mark, w->cand = p + o_mark + up16(n);
    return hipSuccess;
}

// the heap arena for long_total bytes in long segments (none: no block) and the layout's slots
hipError_t me_arena(gbpe_ctx* ctx, GbpeArray<uint8_t>& blk, uint64_t long_total, const uint64_t* slot, MeArena* ar) {
    *ar = MeArena{};
    ar->slot = slot;
    if (!long_total) return hipSuccess;
    const hipError_t e = blk.reserve(ctx, long_total * (3 * sizeof(uint32_t) + 3 * sizeof(uint64_t)) + 64);
    if (e != hipSuccess) return e;
    ar->heap = (uint64_t*)blk.p;
    ar->tok = (uint32_t*)(ar->heap + 3 * long_total);
    ar->nxt = ar->tok + long_total;
    ar->prv = ar->nxt + long_total;
    return hipSuccess;
}

// The kernels of a call, chosen here and nowhere else.  Without an arena (`ar` null: this kernel's
// total sizes it) k_me_long, with special tokens under the SP predicate, the cuts of the SP walk.
// With one, the walk: k_me_walk; with the documents of a batch call (always the word form)
// k_me_walk_docs; with special tokens its SP form, for one buffer too (no document bit is set then:
// `docs` is not read).  `wide`: the layout of t's slots, gbpe_bpe::wide.  A spans call (w.spans) walks
// with k_me_walk_spans, the document form whatever the call holds, SP with special tokens.
template <bool WORDS, uint32_t CS>
void me_launch(hipStream_t s, const uint8_t* in, const uint8_t* ws, uint64_t n, const MeTable& t, bool wide,
               const MeWork& w, uint64_t nchunks, const MeArena* ar, const MeDocs* docs, const MeSp* sp) {
    const dim3 grid((uint32_t)gbpe_div_up(nchunks, ME_TPB)), tpb(ME_TPB);
    if (!ar) {
        if constexpr (WORDS) {
            if (sp) {
                hipLaunchKernelGGL((k_me_long<true, CS, true>), grid, tpb, 0, s, in, ws, n, t, w.back, w.slot, nchunks);
                return;
            }
        }
        hipLaunchKernelGGL((k_me_long<WORDS, CS>), grid, tpb, 0, s, in, ws, n, t, w.back, w.slot, nchunks);
        return;
    }
    auto walk = [&](auto wide_c) {
        constexpr bool WIDE = decltype(wide_c)::value;
        if constexpr (WORDS) {
            if (w.spans) {
                if (sp)
                    hipLaunchKernelGGL((k_me_walk_spans<CS, true, WIDE>), grid, tpb, 0, s, in, ws, n, t, w.scratch, w.counts,
                                       w.base, nchunks, *ar, docs ? *docs : MeDocs{}, *sp);
                else
                    hipLaunchKernelGGL((k_me_walk_spans<CS, false, WIDE>), grid, tpb, 0, s, in, ws, n, t, w.scratch, w.counts,
                                       w.base, nchunks, *ar, docs ? *docs : MeDocs{}, MeSp{});
                return;
            }
            if (sp) {
                hipLaunchKernelGGL((k_me_walk_docs<CS, true, WIDE>), grid, tpb, 0, s, in, ws, n, t, w.scratch, w.counts,
                                   w.base, nchunks, *ar, docs ? *docs : MeDocs{}, *sp);
                return;
            }
            if (docs) {
                hipLaunchKernelGGL((k_me_walk_docs<CS, false, WIDE>), grid, tpb, 0, s, in, ws, n, t, w.scratch, w.counts,
                                   w.base, nchunks, *ar, *docs, MeSp{});
                return;
            }
        }
        hipLaunchKernelGGL((k_me_walk<WORDS, CS, WIDE>), grid, tpb, 0, s, in, ws, n, t, w.scratch, w.counts, w.base,
                           nchunks, *ar);
    };
    if (wide) walk(std::true_type{});
    else walk(std::false_type{});
}

// the instantiation of a call: no mask at ME_CS, or the word form at cs
#define ME_DISPATCH(words, cs, ...)                                     \
    do {                                                                \
        if (!(words)) me_launch<false, ME_CS>(__VA_ARGS__);             \
        else if ((cs) == 4096u) me_launch<true, 4096u>(__VA_ARGS__);    \
        else if ((cs) == 1024u) me_launch<true, 1024u>(__VA_ARGS__);    \
        else me_launch<true, 256u>(__VA_ARGS__);                        \
    } while (0)

struct MeDocJob {   // the documents of a batch call, n_docs > 0
    const uint64_t* d_doc_off;   // [0, n_docs]
    uint64_t n_docs;
    uint64_t* d_tok_off;         // [0, n_docs]
};

// w.mask of a batch call and of one with special tokens (`docs`, `sp`: at least one).  Bit 0 =
// the mode's mask of every document — of every piece between accepted specials — alone (mode NONE:
// nothing) | the starts of the documents, of the specials and of the pieces after them;
// ME_DOC_BIT = a document starts here; ME_SP_BIT / ME_SPIN_BIT = a special's first / other bytes.
// The GPT-4, cl100k and o200k rules see a piece alone through the document form of the pre-tokeniser: w.flags holds
// the document starts, then (k_sp_accept) the pieces' too.  The other modes' masks look one byte
// back at most, so forcing a piece's first byte is all they need.  The first kernel checks the
// offsets into the second word of w.back (zeroed by the caller).
// the modes whose mask comes from a pre-tokeniser's kernels (pretok.hip)
bool me_pretok(uint32_t mode) { return mode == GBPE_WORDS_GPT4 || mode == GBPE_WORDS_CL100K || mode == GBPE_WORDS_O200K; }

int me_mask(gbpe_ctx* ctx, const uint8_t* d_in, uint64_t n, const uint8_t* d_ws, uint32_t mode, const MeDocJob* docs,
            const gbpe_specials* sp, const MeWork& w) {
    hipStream_t s = ctx->stream;
    uint32_t* d_invalid = (uint32_t*)(w.back + 1);
    int rc = GBPE_OK;
    if (w.flags) GBPE_HIP(ctx, hipMemsetAsync(w.flags, 0, n, s));
    if (docs) rc = gbpe_doc_flags_launch(ctx, docs->d_doc_off, docs->n_docs, n, w.flags, w.flags ? 1u : 0u, d_invalid);
    if (rc == GBPE_OK && sp)
        rc = gbpe_specials_launch(ctx, sp, d_in, n, docs ? w.flags : nullptr, w.cand, w.mark,
                                  me_pretok(mode) ? w.flags : nullptr);
    if (rc != GBPE_OK) return rc;
    if (mode == GBPE_WORDS_GPT4) {
        rc = gbpe_pretok_gpt4_docs_launch(ctx, d_in, n, w.flags, w.mask);
    } else if (mode == GBPE_WORDS_CL100K) {
        rc = gbpe_pretok_cl100k_launch(ctx, d_in, n, w.flags, w.mask);
    } else if (mode == GBPE_WORDS_O200K) {
        rc = gbpe_pretok_o200k_launch(ctx, d_in, n, w.flags, w.mask);
    } else if (mode == GBPE_WORDS_NONE) {
        GBPE_HIP(ctx, hipMemsetAsync(w.mask, 0, n, s));
    } else if (mode == GBPE_WORDS_MASK) {
        hipLaunchKernelGGL(k_me_mask01, dim3((uint32_t)gbpe_div_up(n, 1024)), dim3(256), 0, s, d_ws, n, w.mask);
    } else {
        rc = gbpe_word_boundary_launch(ctx, d_in, n, w.mask);
    }
    if (rc == GBPE_OK && sp)
        hipLaunchKernelGGL(k_me_sp_mask, dim3((uint32_t)gbpe_div_up(n, 4096)), dim3(256), 0, s, (const uint8_t*)w.mark, n,
                           w.mask);
    if (rc == GBPE_OK && docs) rc = gbpe_doc_flags_launch(ctx, docs->d_doc_off, docs->n_docs, n, w.mask, ME_DOC_BIT, nullptr);
    return rc;
}

// d_in[0, n) (and, mode MASK, d_ws[0, n)) → d_out[0, min(total, out_cap)); n > 0, the mode checked.
// With `docs`, also d_doc_off[0, n_docs] → d_tok_off[0, n_docs]: the tokens are the word kernels'
// under me_mask's mask; with `sp` (special tokens), of the pieces between the accepted specials.  The offsets' verdict comes back with the long-segment total, the
// call's first synchronise, before anything is written to d_out or d_tok_off.  `what` names the
// entry point in error texts.  `spans`: also d_tok_start[0, min(total, out_cap)), each token's first
// byte; the call runs the word and document form under a 0 / 1 mask of its own.
int me_run(gbpe_ctx* ctx, gbpe_bpe* bp, const gbpe_specials* sp, const char* what, const uint8_t* d_in, uint64_t n,
           const uint8_t* d_ws, uint32_t mode, uint32_t* d_out, uint64_t out_cap, const MeDocJob* docs, uint64_t* n_out,
           bool spans = false, uint64_t* d_tok_start = nullptr) {
    hipStream_t s = ctx->stream;
    const bool words = spans || docs || sp || mode != GBPE_WORDS_NONE;   // (a document start, a special's edge is a cut)
    uint32_t cs = ME_CS;
    if (words) {
        cs = (uint32_t)gbpe_debug_knob("me_cs", ME_CS_WORDS);   // (read per call: the bench and the tests run all three)
        if (cs != 4096u && cs != 1024u && cs != 256u)
            return gbpe_set_error(ctx, GBPE_E_INVALID, "GBPE_DEBUG me_cs: %u is not 4096, 1024 or 256", cs);
    }
    const uint64_t nchunks = gbpe_div_up(n, cs);
    const uint64_t nblk = gbpe_div_up(nchunks, SCAN_BLK);
    GbpeArray<uint8_t> work, mask, arena;
    MeWork w;
    // (flags: the pre-tokenisers' piece starts; the document starts the matcher must not cross)
    GBPE_HIP(ctx, me_layout(ctx, work, n, cs, nchunks, nblk, docs ? docs->n_docs : 0,
                            (docs || sp) && (me_pretok(mode) || (docs && sp)), sp != nullptr, spans, &w));
    const MeTable t{bp->slots, bp->mask, bp->cross};
    const uint64_t cell = docs ? 16 : 8;   // of w.back: a batch call also reads the offsets' verdict

    GBPE_HIP(ctx, hipEventRecord(ctx->ev[0], s));
    int rc = GBPE_OK;
    if (docs || sp) {
        GBPE_HIP(ctx, hipMemsetAsync(w.back, 0, cell, s));
        rc = me_mask(ctx, d_in, n, d_ws, mode, docs, sp, w);
        d_ws = w.mask;
    } else if (spans && (mode == GBPE_WORDS_NONE || mode == GBPE_WORDS_MASK)) {
        // the document walk reads the mask's bits: nothing for NONE, the caller's as 0 / 1
        GBPE_HIP(ctx, mask.reserve(ctx, n));
        if (mode == GBPE_WORDS_NONE) GBPE_HIP(ctx, hipMemsetAsync(mask.p, 0, n, s));
        else hipLaunchKernelGGL(k_me_mask01, dim3((uint32_t)gbpe_div_up(n, 1024)), dim3(256), 0, s, d_ws, n, mask.p);
        d_ws = mask.p;
    } else if (mode == GBPE_WORDS_HEURISTIC || me_pretok(mode)) {
        GBPE_HIP(ctx, mask.reserve(ctx, n));
        rc = mode == GBPE_WORDS_GPT4     ? gbpe_pretok_gpt4_launch(ctx, d_in, n, mask.p)
             : mode == GBPE_WORDS_CL100K ? gbpe_pretok_cl100k_launch(ctx, d_in, n, nullptr, mask.p)
             : mode == GBPE_WORDS_O200K  ? gbpe_pretok_o200k_launch(ctx, d_in, n, nullptr, mask.p)
                                         : gbpe_word_boundary_launch(ctx, d_in, n, mask.p);
        d_ws = mask.p;
    }
    if (rc != GBPE_OK) {
        hipStreamSynchronize(s);   // (the pooled blocks are given back on return)
        return rc;
    }
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[1], s));
    // long segments: their total length sizes the heap arena (none: no arena)
    const MeDocs md{docs ? docs->d_doc_off : nullptr, docs ? docs->n_docs : 0, w.doc_written};
    const MeSp ms{w.mark, sp ? gbpe_specials_ids(sp) : nullptr};
    const MeDocs* pd = docs ? &md : nullptr;
    const MeSp* ps = sp ? &ms : nullptr;
    hipError_t e = docs || sp ? hipSuccess : hipMemsetAsync(w.back, 0, cell, s);
    if (e == hipSuccess) {
        ME_DISPATCH(words, cs, s, d_in, d_ws, n, t, bp->wide, w, nchunks, nullptr, pd, ps);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ctx->ev[2], s);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->enc_host_total, w.back, cell, hipMemcpyDeviceToHost, s);
    const hipError_t e1 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e1;
    uint64_t back[2] = {0, 0};   // {long-segment total, bad offsets}
    memcpy(back, ctx->enc_host_total, cell);
    if (e == hipSuccess && (uint32_t)back[1]) return gbpe_doc_offsets_error(ctx, what, (uint32_t)back[1]);   // nothing was written
    MeArena ar{};
    if (e == hipSuccess) e = me_arena(ctx, arena, back[0], w.slot, &ar);
    if (e == hipSuccess) e = hipEventRecord(ctx->ev[3], s);
    if (e == hipSuccess) {
        ME_DISPATCH(words, cs, s, d_in, d_ws, n, t, bp->wide, w, nchunks, &ar, pd, ps);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ctx->ev[4], s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_chunk_scan1, dim3((uint32_t)nblk), dim3(SCAN_TPB), 0, s, (const uint32_t*)w.counts, nchunks,
                           w.local, w.blocksum);
        hipLaunchKernelGGL(k_chunk_scan2, dim3(1), dim3(SCAN_TPB), 0, s, w.blocksum, nblk, w.total);
        if (out_cap && spans)
            hipLaunchKernelGGL(k_me_compact_spans, dim3((uint32_t)gbpe_div_up(nchunks, 4)), dim3(256), 0, s,
                               (const uint2*)w.scratch, (const uint32_t*)w.counts,
                               (const uint64_t*)w.base, (const uint32_t*)w.local, (const uint64_t*)w.blocksum, nchunks,
                               d_out, d_tok_start, out_cap);
        else if (out_cap)
            hipLaunchKernelGGL(k_me_compact, dim3((uint32_t)gbpe_div_up(nchunks, 4)), dim3(256), 0, s,
                               (const uint32_t*)w.scratch, (const uint32_t*)w.counts, (const uint64_t*)w.base,
                               (const uint32_t*)w.local, (const uint64_t*)w.blocksum, nchunks, d_out, out_cap);
        if (docs)   // (runs whether or not the tokens fit: tok_off is complete on GBPE_E_CAPACITY)
            hipLaunchKernelGGL(k_me_tok_off, dim3((uint32_t)gbpe_div_up(docs->n_docs + 1, 256)), dim3(256), 0, s,
                               docs->d_doc_off, docs->n_docs, n, cs, (const uint32_t*)w.doc_written,
                               (const uint32_t*)w.local, (const uint64_t*)w.blocksum, (const uint64_t*)w.total,
                               docs->d_tok_off);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ctx->ev[5], s);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->enc_host_total, w.total, 8, hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);   // (always: the pooled blocks are given back on return)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess)
        return gbpe_set_error(ctx, e == hipErrorOutOfMemory ? GBPE_E_OOM : GBPE_E_DEVICE, "%s failed: %s", what,
                              hipGetErrorString(e));
    float a = 0, b = 0, c = 0, d = 0;
    hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[1]);
    hipEventElapsedTime(&b, ctx->ev[1], ctx->ev[2]);
    hipEventElapsedTime(&c, ctx->ev[3], ctx->ev[4]);
    hipEventElapsedTime(&d, ctx->ev[4], ctx->ev[5]);
    ctx->bpe_ms[0] = a;
    ctx->bpe_ms[1] = (double)b + c;
    ctx->bpe_ms[2] = d;
    uint64_t tot = 0;
    memcpy(&tot, ctx->enc_host_total, 8);
    *n_out = tot;
    if (tot > out_cap)
        return gbpe_set_error(ctx, GBPE_E_CAPACITY, "bpe encode%s: output needs %llu tokens", docs ? " batch" : "",
                              (unsigned long long)tot);
    return GBPE_OK;
}

int me_words_check(gbpe_ctx* ctx, const void* word_starts, uint32_t mode) {
    if (mode > GBPE_WORDS_CL100K && mode != GBPE_WORDS_O200K)   // (5 is no mode: gpubpe.h)
        return gbpe_set_error(ctx, GBPE_E_INVALID, "bpe encode: unknown words mode %u", mode);
    if ((word_starts != nullptr) != (mode == GBPE_WORDS_MASK))
        return gbpe_set_error(ctx, GBPE_E_INVALID, "bpe encode: word_starts goes with GBPE_WORDS_MASK, and only with it");
    return GBPE_OK;
}

}  // namespace

// ── the entry points: one buffer or many documents (`batch`), each with and without a
//    special table (`special`: sp must be one), on device or on host buffers ──
namespace {

// What every entry point checks before it does anything, in the order a bad call's status and text
// depend on.  `device`: out, doc_off and tok_off are device pointers, read there by words.
int me_check(gbpe_ctx* ctx, const gbpe_bpe* bp, const gbpe_specials* sp, bool special, bool batch, bool device,
             const void* bytes, uint64_t n, const void* doc_off, uint64_t n_docs, const void* word_starts,
             uint32_t words_mode, const void* out, uint64_t out_cap, const void* tok_off, uint64_t* n_out) {
    if (special && !sp) {
        if (n_out) *n_out = 0;
        return gbpe_set_error(ctx, GBPE_E_INVALID, "bpe encode (special): no special table");
    }
    if (!ctx || !bp || !n_out || (batch && (!tok_off || (n_docs && !doc_off))) || (n && (!batch || n_docs) && !bytes) ||
        (out_cap && !out))
        return gbpe_set_error(ctx, GBPE_E_INVALID, "null argument");
    *n_out = 0;
    const int rc = me_words_check(ctx, word_starts, words_mode);
    if (rc != GBPE_OK || !device) return rc;
    if ((uintptr_t)out & 3u) return gbpe_set_error(ctx, GBPE_E_INVALID, "d_out must be 4-byte aligned");
    if (batch && (((uintptr_t)doc_off | (uintptr_t)tok_off) & 7u))
        return gbpe_set_error(ctx, GBPE_E_INVALID, "d_doc_off and d_tok_off must be 8-byte aligned");
    return GBPE_OK;
}

int me_device(gbpe_ctx* ctx, gbpe_bpe* bp, const gbpe_specials* sp, bool special, bool batch, const void* d_bytes,
              uint64_t n, const void* d_doc_off, uint64_t n_docs, const void* d_word_starts, uint32_t words_mode,
              void* d_out, uint64_t out_cap, void* d_tok_off, uint64_t* n_out, bool spans = false,
              void* d_tok_start = nullptr) {
    const int rc = me_check(ctx, bp, sp, special, batch, true, d_bytes, n, d_doc_off, n_docs, d_word_starts, words_mode,
                            d_out, out_cap, d_tok_off, n_out);
    if (rc != GBPE_OK) return rc;
    if (spans && ((uintptr_t)d_tok_start & 7u)) return gbpe_set_error(ctx, GBPE_E_INVALID, "d_tok_start must be 8-byte aligned");
    if (n == 0 || (batch && n_docs == 0)) {
        if (batch) {
            GBPE_HIP(ctx, hipMemsetAsync(d_tok_off, 0, (n_docs + 1) * 8, ctx->stream));
            GBPE_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        return GBPE_OK;
    }
    const MeDocJob docs{(const uint64_t*)d_doc_off, n_docs, (uint64_t*)d_tok_off};
    return me_run(ctx, bp, sp, batch ? "bpe encode batch" : "bpe encode (words)", (const uint8_t*)d_bytes, n, (const uint8_t*)d_word_starts, words_mode,
                  (uint32_t*)d_out, out_cap, batch ? &docs : nullptr, n_out, spans, (uint64_t*)d_tok_start);
}

// Host buffers: one upload of the offsets (a batch call), the bytes (and the mask), me_run, and back
// come the token offsets (a batch call) and the tokens that fit: at most one per byte.
int me_host(gbpe_ctx* ctx, gbpe_bpe* bp, const gbpe_specials* sp, bool special, bool batch, const uint8_t* bytes, uint64_t n,
            const uint64_t* doc_off, uint64_t n_docs, const uint8_t* word_starts, uint32_t words_mode, uint32_t* out,
            uint64_t out_cap, uint64_t* tok_off, uint64_t* n_out, bool spans = false, uint64_t* tok_start = nullptr) {
    int rc = me_check(ctx, bp, sp, special, batch, false, bytes, n, doc_off, n_docs, word_starts, words_mode, out, out_cap,
                      tok_off, n_out);
    if (rc != GBPE_OK) return rc;
    const char* what = batch ? "bpe encode batch" : "bpe encode (words)";
    if (n == 0 || (batch && n_docs == 0)) {
        if (batch)
            for (uint64_t d = 0; d <= n_docs; ++d) tok_off[d] = 0;
        return GBPE_OK;
    }
    if (batch) {
        rc = gbpe_doc_offsets_check(ctx, what, doc_off, n_docs, n);   // before anything is launched
        if (rc != GBPE_OK) return rc;
    }
    const uint64_t cap = out_cap < n ? out_cap : n;
    const uint64_t off_bytes = batch ? 8 * (n_docs + 1) : 0;
    const uint64_t o_tok = up16(off_bytes), o_in = 2 * o_tok, o_ws = o_in + up16(n);
    const uint64_t o_out = o_ws + (word_starts ? up16(n) : 0), o_ts = o_out + up16(4 * cap);   // (spans: the starts)
    GbpeArray<uint8_t> io;
    GBPE_HIP(ctx, io.reserve(ctx, (spans ? o_ts + 8 * cap : o_out + 4 * cap) + 16));
    hipStream_t s = ctx->stream;
    uint8_t* d_ws = word_starts ? io.p + o_ws : nullptr;
    hipError_t e = batch ? hipMemcpyAsync(io.p, doc_off, off_bytes, hipMemcpyHostToDevice, s) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(io.p + o_in, bytes, n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && word_starts) e = hipMemcpyAsync(d_ws, word_starts, n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        const MeDocJob docs{(const uint64_t*)io.p, n_docs, (uint64_t*)(io.p + o_tok)};
        rc = me_run(ctx, bp, sp, what, io.p + o_in, n, d_ws, words_mode, (uint32_t*)(io.p + o_out), cap,
                    batch ? &docs : nullptr, n_out, spans, (uint64_t*)(io.p + o_ts));
        if (rc != GBPE_OK && rc != GBPE_E_CAPACITY) return rc;   // (synchronised there)
        if (batch) e = hipMemcpyAsync(tok_off, io.p + o_tok, off_bytes, hipMemcpyDeviceToHost, s);
        const uint64_t fit = *n_out < cap ? *n_out : cap;
        if (e == hipSuccess && fit) e = hipMemcpyAsync(out, io.p + o_out, fit * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && fit && spans) e = hipMemcpyAsync(tok_start, io.p + o_ts, fit * 8, hipMemcpyDeviceToHost, s);
    }
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return gbpe_set_error(ctx, GBPE_E_DEVICE, "%s failed: %s", what, hipGetErrorString(e));
    return rc;
}

// What the spans calls check before me_check: the call's shape is read off its pointers —
// documents when doc_off is given, a special table when `specials` is — and n stays where a token's
// relative start fits a u32 (MeWork::spans).
int me_spans_check(gbpe_ctx* ctx, uint64_t n, const void* doc_off, uint64_t n_docs, const void* tok_start, uint64_t out_cap,
                   const void* tok_off, uint64_t* n_out) {
    if (n_out) *n_out = 0;
    if ((doc_off != nullptr) != (tok_off != nullptr))
        return gbpe_set_error(ctx, GBPE_E_INVALID, "bpe encode (spans): doc_off and tok_off go together");
    if (!doc_off && n_docs) return gbpe_set_error(ctx, GBPE_E_INVALID, "bpe encode (spans): n_docs without doc_off");
    if (out_cap && !tok_start) return gbpe_set_error(ctx, GBPE_E_INVALID, "null argument");
    if (n > ME_SPANS_MAX_N)
        return gbpe_set_error(ctx, GBPE_E_INVALID, "bpe encode (spans): %llu bytes, above the limit of %llu",
                              (unsigned long long)n, (unsigned long long)ME_SPANS_MAX_N);
    return GBPE_OK;
}

}  // namespace

extern "C" int gbpe_bpe_encode_spans(gbpe_ctx* ctx, gbpe_bpe* bp, gbpe_specials* sp, const uint8_t* bytes, uint64_t n,
                                     const uint64_t* doc_off, uint64_t n_docs, const uint8_t* word_starts,
                                     uint32_t words_mode, uint32_t* out, uint64_t* tok_start, uint64_t out_cap,
                                     uint64_t* tok_off, uint64_t* n_out) {
    const int rc = me_spans_check(ctx, n, doc_off, n_docs, tok_start, out_cap, tok_off, n_out);
    if (rc != GBPE_OK) return rc;
    return me_host(ctx, bp, sp, sp != nullptr, doc_off != nullptr, bytes, n, doc_off, n_docs, word_starts, words_mode, out,
                   out_cap, tok_off, n_out, true, tok_start);
}

extern "C" int gbpe_bpe_encode_spans_device(gbpe_ctx* ctx, gbpe_bpe* bp, gbpe_specials* sp, const void* d_bytes, uint64_t n,
                                            const void* d_doc_off, uint64_t n_docs, const void* d_word_starts,
                                            uint32_t words_mode, void* d_out, void* d_tok_start, uint64_t out_cap,
                                            void* d_tok_off, uint64_t* n_out) {
    const int rc = me_spans_check(ctx, n, d_doc_off, n_docs, d_tok_start, out_cap, d_tok_off, n_out);
    if (rc != GBPE_OK) return rc;
    return me_device(ctx, bp, sp, sp != nullptr, d_doc_off != nullptr, d_bytes, n, d_doc_off, n_docs, d_word_starts,
                     words_mode, d_out, out_cap, d_tok_off, n_out, true, d_tok_start);
}

extern "C" int gbpe_bpe_encode_words_device(gbpe_ctx* ctx, gbpe_bpe* bp, const void* d_bytes, uint64_t n,
                                            const void* d_word_starts, uint32_t words_mode, void* d_out, uint64_t out_cap,
                                            uint64_t* n_out) {
    return me_device(ctx, bp, nullptr, false, false, d_bytes, n, nullptr, 0, d_word_starts, words_mode, d_out, out_cap,
                     nullptr, n_out);
}

extern "C" int gbpe_bpe_encode_special_device(gbpe_ctx* ctx, gbpe_bpe* bp, gbpe_specials* sp, const void* d_bytes, uint64_t n,
                                              const void* d_word_starts, uint32_t words_mode, void* d_out, uint64_t out_cap,
                                              uint64_t* n_out) {
    return me_device(ctx, bp, sp, true, false, d_bytes, n, nullptr, 0, d_word_starts, words_mode, d_out, out_cap, nullptr,
                     n_out);
}

extern "C" int gbpe_bpe_encode_words(gbpe_ctx* ctx, gbpe_bpe* bp, const uint8_t* bytes, uint64_t n,
                                     const uint8_t* word_starts, uint32_t words_mode, uint32_t* out, uint64_t out_cap,
                                     uint64_t* n_out) {
    return me_host(ctx, bp, nullptr, false, false, bytes, n, nullptr, 0, word_starts, words_mode, out, out_cap, nullptr,
                   n_out);
}

extern "C" int gbpe_bpe_encode_special(gbpe_ctx* ctx, gbpe_bpe* bp, gbpe_specials* sp, const uint8_t* bytes, uint64_t n,
                                       const uint8_t* word_starts, uint32_t words_mode, uint32_t* out, uint64_t out_cap,
                                       uint64_t* n_out) {
    return me_host(ctx, bp, sp, true, false, bytes, n, nullptr, 0, word_starts, words_mode, out, out_cap, nullptr, n_out);
}

// the whole string: no word cuts (the words contract, gpubpe.h)
extern "C" int gbpe_bpe_encode(gbpe_ctx* ctx, gbpe_bpe* bp, const uint8_t* bytes, uint64_t n, uint32_t* out,
                               uint64_t out_cap, uint64_t* n_out) {
    return gbpe_bpe_encode_words(ctx, bp, bytes, n, nullptr, GBPE_WORDS_NONE, out, out_cap, n_out);
}

extern "C" int gbpe_bpe_encode_words_batch_device(gbpe_ctx* ctx, gbpe_bpe* bp, const void* d_bytes, uint64_t n,
                                                  const void* d_doc_off, uint64_t n_docs, const void* d_word_starts,
                                                  uint32_t words_mode, void* d_out, uint64_t out_cap, void* d_tok_off,
                                                  uint64_t* n_out) {
    return me_device(ctx, bp, nullptr, false, true, d_bytes, n, d_doc_off, n_docs, d_word_starts, words_mode, d_out, out_cap,
                     d_tok_off, n_out);
}

extern "C" int gbpe_bpe_encode_special_batch_device(gbpe_ctx* ctx, gbpe_bpe* bp, gbpe_specials* sp, const void* d_bytes,
                                                    uint64_t n, const void* d_doc_off, uint64_t n_docs,
                                                    const void* d_word_starts, uint32_t words_mode, void* d_out,
                                                    uint64_t out_cap, void* d_tok_off, uint64_t* n_out) {
    return me_device(ctx, bp, sp, true, true, d_bytes, n, d_doc_off, n_docs, d_word_starts, words_mode, d_out, out_cap,
                     d_tok_off, n_out);
}

extern "C" int gbpe_bpe_encode_words_batch(gbpe_ctx* ctx, gbpe_bpe* bp, const uint8_t* bytes, uint64_t n,
                                           const uint64_t* doc_off, uint64_t n_docs, const uint8_t* word_starts,
                                           uint32_t words_mode, uint32_t* out, uint64_t out_cap, uint64_t* tok_off,
                                           uint64_t* n_out) {
    return me_host(ctx, bp, nullptr, false, true, bytes, n, doc_off, n_docs, word_starts, words_mode, out, out_cap, tok_off,
                   n_out);
}

extern "C" int gbpe_bpe_encode_special_batch(gbpe_ctx* ctx, gbpe_bpe* bp, gbpe_specials* sp, const uint8_t* bytes, uint64_t n,
                                             const uint64_t* doc_off, uint64_t n_docs, const uint8_t* word_starts,
                                             uint32_t words_mode, uint32_t* out, uint64_t out_cap, uint64_t* tok_off,
                                             uint64_t* n_out) {
    return me_host(ctx, bp, sp, true, true, bytes, n, doc_off, n_docs, word_starts, words_mode, out, out_cap, tok_off, n_out);
}

extern "C" int gbpe_bpe_encode_last_timing(gbpe_ctx* ctx, double* ms_starts, double* ms_walk, double* ms_compact) {
    if (!ctx) return GBPE_E_INVALID;
    if (ms_starts) *ms_starts = ctx->bpe_ms[0];
    if (ms_walk) *ms_walk = ctx->bpe_ms[1];
    if (ms_compact) *ms_compact = ctx->bpe_ms[2];
    return GBPE_OK;
}
