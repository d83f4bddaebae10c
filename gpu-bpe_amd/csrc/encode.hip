// Chunked greedy longest-match trie encode on MI355X (gfx950).
//
// Replaces tokenize.wgsl (trie_tokenizer_chunked :88-175, trie_prefix_sum
// :199-208, trie_tokenizer_compact :225-243) and the TrieTokenizer host
// pass (tokenizer.js:213-335).
//
// Layout: the reference walks a BFS trie of {firstChild, numChildren,
// tokenId} nodes with a binary search over sorted edges per byte
// (tokenize.wgsl:69-86: up to 8 dependent loads per byte).  On upload we
// recompile the same trie into a double-array table: state t's record is
// {check = parent state, base, tokenId}, and the child of state s on byte c
// is t = base(s) + c iff record[t].check == s — one 16-byte L2-resident load
// per byte consumed.  The 256 root transitions (and their depth-1 records)
// live in LDS, as in the reference's root LUT + depth-1 cache
// (tokenize.wgsl:51-63, 93-119).  Transitions are identical to the
// reference trie's, so token ids are bit-identical.

#include "common.h"
#include "scan.h"

#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <string>
#include <thread>

namespace {

constexpr int WALK_TPB = 256;
constexpr uint64_t kEncSlice = 128ull << 20;   // gbpe_encode's pipeline slice (host buffers)
constexpr uint32_t INV = 0xFFFFFFFFu;

template <typename T>
__global__ __launch_bounds__(WALK_TPB) void k_trie_walk(const uint8_t* __restrict__ in, uint64_t n, uint32_t cs,
                                                        const uint4* __restrict__ rec, uint32_t nrec,
                                                        const uint4* __restrict__ root, T* __restrict__ scratch,
                                                        uint32_t* __restrict__ counts, uint64_t nchunks) {
    __shared__ uint4 lut[256];   // byte -> {state, base, tokenId, present}
    lut[threadIdx.x] = root[threadIdx.x];
    __syncthreads();
    const uint64_t chunk = (uint64_t)blockIdx.x * WALK_TPB + threadIdx.x;
    if (chunk >= nchunks) return;
    const uint64_t c0 = chunk * cs;
    const uint64_t ce = min(c0 + cs, n);
    T* out = scratch + c0;
    const uint32_t* in32 = reinterpret_cast<const uint32_t*>(in);
    uint64_t widx = ~0ull;
    uint32_t word = 0;
    auto byte_at = [&](uint64_t p) -> uint32_t {
        const uint64_t wi = p >> 2;
        if (wi != widx) {
            if (wi * 4 + 4 <= n) {
                word = in32[wi];
            } else {   // the last partial word: byte loads inside [0, n)
                word = 0;
                for (uint64_t j = wi * 4; j < n; ++j) word |= (uint32_t)in[j] << ((j & 3u) * 8u);
            }
            widx = wi;
        }
        return (word >> ((p & 3u) * 8u)) & 0xFFu;
    };
    uint32_t cnt = 0;
    uint64_t pos = c0;
    while (pos < ce) {
        const uint32_t c = byte_at(pos);
        const uint4 e = lut[c];
        uint32_t lmt = INV;
        uint64_t lmp = pos;
        if (e.w) {
            uint32_t s = e.x, base = e.y;
            if (e.z != INV) {
                lmt = e.z;
                lmp = pos + 1;
            }
            uint64_t wp = pos + 1;
            while (wp < ce) {
                const uint32_t t = base + byte_at(wp);
                if (t >= nrec) break;
                const uint4 r = rec[t];
                if (r.x != s) break;
                s = t;
                base = r.y;
                ++wp;
                if (r.z != INV) {
                    lmt = r.z;
                    lmp = wp;
                }
            }
        }
        if (lmt != INV) {
            out[cnt++] = (T)lmt;
            pos = lmp;
        } else {   // no token starts here: emit the raw byte value (tokenize.wgsl:169-171)
            out[cnt++] = (T)c;
            ++pos;
        }
    }
    counts[chunk] = cnt;
}

// Packed 8-byte double-array records (built by gbpe_trie_upload):
//   x = check (22 bits) | tokenId bits 0-9 << 22,  y = base (22 bits) | tokenId bits 10-19 << 22
// check 0x3FFFFF = empty slot, tokenId 0xFFFFF = none, base 0 = leaf (no children).
__device__ __forceinline__ uint32_t rec_check(uint2 r) { return r.x & 0x3FFFFFu; }
__device__ __forceinline__ uint32_t rec_base(uint2 r) { return r.y & 0x3FFFFFu; }
__device__ __forceinline__ uint32_t rec_tid(uint2 r) { return (r.x >> 22) | ((r.y >> 22) << 10); }
constexpr uint32_t TID_NONE = 0xFFFFFu;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t win_byte(uint4 w, uint32_t o) {
    const uint32_t d = (o & 8u) ? ((o & 4u) ? w.w : w.z) : ((o & 4u) ? w.y : w.x);
    return (d >> ((o & 3u) * 8u)) & 0xFFu;
}

__device__ __forceinline__ uint4 load_win(const uint8_t* __restrict__ in, uint64_t n, uint64_t ab) {
    if (ab + 16 <= n) return *reinterpret_cast<const uint4*>(in + ab);
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;   // the last partial block: byte loads inside [0, n)
    for (uint32_t j = 0; j < 16 && ab + j < n; ++j) {
        const uint32_t v = (uint32_t)in[ab + j] << ((j & 3) * 8);
        if (j < 4) w0 |= v; else if (j < 8) w1 |= v; else if (j < 12) w2 |= v; else w3 |= v;
    }
    return make_uint4(w0, w1, w2, w3);
}

// 64-byte input window (one cache line per refill): 4 x 16 bytes in registers
struct Win64 {
    uint4 q0, q1, q2, q3;
};
__device__ __forceinline__ Win64 load_win64(const uint8_t* __restrict__ in, uint64_t n, uint64_t ab) {
    Win64 w;
    if (ab + 64 <= n) {
        const uint4* p = reinterpret_cast<const uint4*>(in + ab);
        w.q0 = p[0];
        w.q1 = p[1];
        w.q2 = p[2];
        w.q3 = p[3];
    } else {
        w.q0 = load_win(in, n, ab);
        w.q1 = load_win(in, n, ab + 16);
        w.q2 = load_win(in, n, ab + 32);
        w.q3 = load_win(in, n, ab + 48);
    }
    return w;
}
__device__ __forceinline__ uint32_t win64_byte(const Win64& w, uint32_t o) {
    const uint4 q = (o & 32u) ? ((o & 16u) ? w.q3 : w.q2) : ((o & 16u) ? w.q1 : w.q0);
    return win_byte(q, o & 15u);
}

// token vector: slot j of a 16-byte register vector (8 x u16 or 4 x u32), stored whole
template <typename T>
__device__ __forceinline__ void vec_put(uint4& a, uint32_t j, uint32_t tok) {
    if (sizeof(T) == 2) {
        const uint32_t sh = (j & 1u) * 16u, q = (j >> 1) & 3u;
        const uint32_t v = (tok & 0xFFFFu) << sh;
        a.x |= q == 0 ? v : 0u;
        a.y |= q == 1 ? v : 0u;
        a.z |= q == 2 ? v : 0u;
        a.w |= q == 3 ? v : 0u;
    } else {
        const uint32_t q = j & 3u;
        a.x = q == 0 ? tok : a.x;
        a.y = q == 1 ? tok : a.y;
        a.z = q == 2 ? tok : a.z;
        a.w = q == 3 ? tok : a.w;
    }
}

// Production walk.  One lane per chunk (as tokenize.wgsl:88) over the packed
// 8-byte double-array records, as a one-byte-per-trip state machine: every loop
// trip a lane consumes exactly one byte — a token start resolved from the root
// transitions cached in LDS, or one trie transition (the trip's single L2 load);
// a start that leads into a multi-byte path does its first transition in the same
// trip, and a walk that enters a leaf (base == 0) ends its token without the
// probe that would only find the mismatch.  No lane waits on another lane's run
// of raw / one-byte tokens (an inner start loop made the wave's walking lanes
// wait: 4.84 vs 4.29 ms on C3).  Input arrives a 64-byte line per refill: with
// ~65K lanes per XCD walking, 16-byte refills were evicted from the 4 MB L2
// between uses (5.33 vs 4.84 ms).
constexpr uint32_t WALK_QV = 4;   // token vectors per scratch store burst

template <typename T>
__global__ __launch_bounds__(WALK_TPB) void k_trie_walk_v5(const uint8_t* __restrict__ in, uint64_t n, uint32_t cs,
                                                           const uint2* __restrict__ rec, uint32_t nrec,
                                                           uint32_t root_base, T* __restrict__ scratch,
                                                           uint32_t* __restrict__ counts, uint64_t nchunks) {
    constexpr uint32_t PER = 16 / sizeof(T);
    __shared__ uint2 lut[256];
    {
        const uint32_t t = root_base + threadIdx.x;
        lut[threadIdx.x] = t < nrec ? rec[t] : make_uint2(0x3FFFFFu, 0u);
    }
    __syncthreads();
    const uint64_t chunk = (uint64_t)blockIdx.x * WALK_TPB + threadIdx.x;
    if (chunk >= nchunks) return;
    const uint64_t c0 = chunk * cs;
    const uint32_t ce = (uint32_t)(min(c0 + cs, n) - c0);
    T* out = scratch + c0;
    uint32_t cb = ~0u;
    Win64 w64{};
    uint4 acc = make_uint4(0, 0, 0, 0);
    auto byte_at = [&](uint32_t p) -> uint32_t {
        const uint32_t b = p & ~63u;
        if (b != cb) {
            cb = b;
            w64 = load_win64(in, n, c0 + b);
        }
        return win64_byte(w64, p & 63u);
    };
    // Completed vectors wait in registers and leave WALK_QV at a time, 64
    // contiguous bytes per lane: 3.85 ms against 4.06 for one 16-byte store per
    // vector on C3 (tokens equal).  Wave-wide bursts (every lane stores
    // when one lane's queue is full) measured the same, and at a 2-vector queue
    // slower (4.09 ms).
    uint32_t cnt = 0, nq = 0;
    uint4 q[WALK_QV > 1 ? WALK_QV - 1 : 1];   // q[WALK_QV-1-nq ..]: the nq waiting vectors, oldest first
    auto emit = [&](uint32_t tok) {
        vec_put<T>(acc, cnt % PER, tok);
        if (++cnt % PER == 0) {
            if (nq == WALK_QV - 1) {
                uint4* o = reinterpret_cast<uint4*>(out + cnt) - WALK_QV;
#pragma unroll
                for (uint32_t i = 0; i + 1 < WALK_QV; ++i) o[i] = q[i];
                o[WALK_QV - 1] = acc;
                nq = 0;
            } else {
                if constexpr (WALK_QV > 1) {
#pragma unroll
                    for (uint32_t i = 0; i + 2 < WALK_QV; ++i) q[i] = q[i + 1];
                    q[WALK_QV - 2] = acc;
                }
                ++nq;
            }
            acc = make_uint4(0, 0, 0, 0);
        }
    };
    auto flush = [&]() {   // the waiting vectors end where the partial vector starts
        if constexpr (WALK_QV > 1) {
            uint4* o = reinterpret_cast<uint4*>(out + (cnt / PER) * PER);
#pragma unroll
            for (uint32_t i = 0; i + 1 < WALK_QV; ++i)
                if (i + nq >= WALK_QV - 1) o[(int)i - (int)WALK_QV + 1] = q[i];
            nq = 0;
        }
    };
    uint32_t pos = 0, wp = 0, lmp = 0, st = 0, base = 0, lmt = TID_NONE, first = 0;
    bool walking = false;
    while (pos < ce) {
        if (!walking) {   // a token start: LDS only
            first = byte_at(pos);
            const uint2 e = lut[first];
            const uint32_t tid = rec_tid(e);
            if (rec_check(e) != 0u || rec_base(e) == 0u || pos + 1 >= ce) {
                // no token starts with this byte (emit it raw, tokenize.wgsl:169-171), a
                // one-byte leaf, or the chunk's last byte
                emit(rec_check(e) == 0u && tid != TID_NONE ? tid : first);
                ++pos;
                continue;
            }
            st = root_base + first;
            base = rec_base(e);
            lmt = tid;
            lmp = pos + 1;
            wp = pos + 1;
            walking = true;
        }
        // one trie transition: the trip's L2 load
        const uint32_t t = base + byte_at(wp);
        const uint2 r = t < nrec ? rec[t] : make_uint2(0x3FFFFFu, 0u);
        bool end = true;
        if (rec_check(r) == st) {
            st = t;
            base = rec_base(r);
            ++wp;
            const uint32_t tid = rec_tid(r);
            if (tid != TID_NONE) {
                lmt = tid;
                lmp = wp;
            }
            end = base == 0u || wp >= ce;
        }
        if (end) {   // the longest match ends: emit it (or the raw first byte), restart after it
            const bool hit = lmt != TID_NONE;
            emit(hit ? lmt : first);
            pos = hit ? lmp : pos + 1;
            walking = false;
        }
    }
    flush();
    if (cnt % PER) *reinterpret_cast<uint4*>(out + (cnt / PER) * PER) = acc;
    counts[chunk] = cnt;
}

// Chunk tokens → final positions.  A wave moves CPW chunks at once (every
// scratch load of the CPW chunks is issued before the first store: one chunk's
// ~cs/4 tokens alone leave too few bytes in flight to cover the HBM latency);
// token j + 64k of a chunk pass goes to lane j, so every u32 store instruction
// writes 256 contiguous bytes.  Chunks of more than 256 tokens take more passes.
constexpr int CPW = 4;   // chunks per wave
template <typename T>
__global__ __launch_bounds__(256) void k_chunk_compact4(const T* __restrict__ scratch, const uint32_t* __restrict__ counts,
                                                        const uint32_t* __restrict__ local,
                                                        const uint64_t* __restrict__ blocksum, uint64_t nchunks,
                                                        uint32_t cs, uint32_t* __restrict__ out, uint64_t out_cap) {
    __shared__ uint64_t s_off[4 * CPW];
    __shared__ uint32_t s_cnt[4 * CPW];
    const uint64_t c0 = (uint64_t)blockIdx.x * (4 * CPW);
    if (threadIdx.x < 4 * CPW) {
        const uint64_t c = c0 + threadIdx.x;
        s_cnt[threadIdx.x] = c < nchunks ? counts[c] : 0u;
        s_off[threadIdx.x] = c < nchunks ? blocksum[c / SCAN_BLK] + local[c] : 0ull;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t most = 0;
#pragma unroll
    for (int q = 0; q < CPW; ++q) most = max(most, s_cnt[wid * CPW + q]);
    for (uint32_t b0 = 0; b0 < most; b0 += 256) {
        uint32_t v[CPW][4];
#pragma unroll
        for (int q = 0; q < CPW; ++q) {
            const uint32_t cnt = s_cnt[wid * CPW + q];
            const T* src = scratch + (c0 + wid * CPW + q) * (uint64_t)cs;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t j = b0 + lane + 64u * k;
                v[q][k] = j < cnt ? (uint32_t)src[j] : 0u;
            }
        }
#pragma unroll
        for (int q = 0; q < CPW; ++q) {
            const uint32_t cnt = s_cnt[wid * CPW + q];
            const uint64_t off = s_off[wid * CPW + q];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t j = b0 + lane + 64u * k;
                if (j < cnt && off + j < out_cap) out[off + j] = v[q][k];
            }
        }
    }
}

// ── batched documents (gbpe_encode_batch): many documents laid end to end, each
// chunked from its own first byte ("Batched documents") ──────────
//
// Per-document table: document d has nch[d] = ceil(len / cs) chunks and a
// scratch slot of round_up(len, 8) token elements (a chunk's last partial
// 16-byte token vector stays inside its document's slot, and slot starts keep
// the vector stores aligned); the exclusive scans of both give chunk_base /
// scr_base.  The scratch is then O(n + n_docs) elements, not nchunks * cs.
constexpr int DOC_TPB = 1024;   // documents per table block (one lane each)

struct DocTotals {   // read back once per call (the grid and the scratch are sized from it)
    uint64_t nchunks, scr_elems, invalid;
};

// wave-then-block exclusive scan of one u64 per thread (DOC_TPB threads); returns
// the thread's exclusive prefix, *total = the block's sum
__device__ __forceinline__ uint64_t doc_block_scan(uint64_t v, uint64_t* wsum, uint64_t* total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint64_t incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    uint64_t run = incl - v, all = 0;
    for (int w = 0; w < DOC_TPB / 64; ++w) {
        if (w < wid) run += wsum[w];
        all += wsum[w];
    }
    __syncthreads();   // wsum is reused by the next scan
    *total = all;
    return run;
}

// one lane per document: validate its offsets, its chunk count and slot size,
// block-local exclusive prefixes of both + the block totals
__global__ __launch_bounds__(DOC_TPB) void k_doc_table(const uint64_t* __restrict__ doc_off, uint64_t n_docs, uint64_t n,
                                                       uint32_t cs, uint64_t* __restrict__ chunk_base,
                                                       uint64_t* __restrict__ scr_base, uint64_t* __restrict__ blk_ch,
                                                       uint64_t* __restrict__ blk_scr, uint32_t* __restrict__ invalid) {
    __shared__ uint64_t wsum[DOC_TPB / 64];
    const uint64_t d = (uint64_t)blockIdx.x * DOC_TPB + threadIdx.x;
    uint64_t nch = 0, slot = 0;
    if (d < n_docs) {
        const uint64_t a = doc_off[d], b = doc_off[d + 1];
        uint32_t bad = 0;
        if (b < a || b > n) bad |= GBPE_DOC_BAD_ORDER;   // (b > n: a later entry decreases or the last is not n)
        if (d == 0 && a != 0) bad |= GBPE_DOC_BAD_FIRST;
        if (d == n_docs - 1 && b != n) bad |= GBPE_DOC_BAD_LAST;
        if (bad) {
            atomicOr(invalid, bad);
        } else {
            const uint64_t len = b - a;
            nch = (len + cs - 1) / cs;
            slot = (len + 7) & ~7ull;
        }
    }
    uint64_t tot_ch, tot_scr;
    const uint64_t pc = doc_block_scan(nch, wsum, &tot_ch);
    const uint64_t ps = doc_block_scan(slot, wsum, &tot_scr);
    if (d < n_docs) {
        chunk_base[d] = pc;
        scr_base[d] = ps;
    }
    if (threadIdx.x == 0) {
        blk_ch[blockIdx.x] = tot_ch;
        blk_scr[blockIdx.x] = tot_scr;
    }
}

// exclusive scan of the table blocks' totals (one workgroup); writes the grand totals
__global__ __launch_bounds__(DOC_TPB) void k_doc_scan2(uint64_t* __restrict__ blk_ch, uint64_t* __restrict__ blk_scr,
                                                       uint64_t nblk, const uint32_t* __restrict__ invalid,
                                                       DocTotals* __restrict__ totals) {
    __shared__ uint64_t wsum[DOC_TPB / 64];
    const uint64_t per = (nblk + DOC_TPB - 1) / DOC_TPB;
    const uint64_t lo = min((uint64_t)threadIdx.x * per, nblk), hi = min(lo + per, nblk);
    uint64_t sc = 0, ss = 0;
    for (uint64_t i = lo; i < hi; ++i) {
        sc += blk_ch[i];
        ss += blk_scr[i];
    }
    uint64_t tot_ch, tot_scr;
    uint64_t rc = doc_block_scan(sc, wsum, &tot_ch);
    uint64_t rs = doc_block_scan(ss, wsum, &tot_scr);
    for (uint64_t i = lo; i < hi; ++i) {
        const uint64_t vc = blk_ch[i], vs = blk_scr[i];
        blk_ch[i] = rc;
        blk_scr[i] = rs;
        rc += vc;
        rs += vs;
    }
    if (threadIdx.x == 0) {
        totals->nchunks = tot_ch;
        totals->scr_elems = tot_scr;
        totals->invalid = *invalid;
    }
}

// block-local prefixes → global chunk_base / scr_base (entry n_docs = the totals)
__global__ __launch_bounds__(DOC_TPB) void k_doc_base(uint64_t* __restrict__ chunk_base, uint64_t* __restrict__ scr_base,
                                                      const uint64_t* __restrict__ blk_ch,
                                                      const uint64_t* __restrict__ blk_scr, uint64_t n_docs,
                                                      const DocTotals* __restrict__ totals) {
    const uint64_t d = (uint64_t)blockIdx.x * DOC_TPB + threadIdx.x;
    if (d < n_docs) {
        chunk_base[d] += blk_ch[blockIdx.x];
        scr_base[d] += blk_scr[blockIdx.x];
    } else if (d == n_docs) {
        chunk_base[d] = totals->nchunks;
        scr_base[d] = totals->scr_elems;
    }
}

// Per-chunk descriptor: where the chunk's bytes start, how many there are, and
// where its tokens go in the scratch.
struct __attribute__((aligned(16))) ChunkDesc {
    uint64_t c0;    // first byte (absolute in the batch buffer)
    uint64_t scr;   // first scratch element
    uint32_t len;   // min(cs, document end - c0)
    uint32_t pad[3];
};
static_assert(sizeof(ChunkDesc) == 32, "two 16-byte loads per descriptor");

// one lane per chunk: its document is the last d with chunk_base[d] <= chunk (an
// empty document repeats its successor's chunk_base and is stepped over)
__global__ __launch_bounds__(256) void k_chunk_desc(const uint64_t* __restrict__ doc_off,
                                                    const uint64_t* __restrict__ chunk_base,
                                                    const uint64_t* __restrict__ scr_base, uint64_t n_docs, uint32_t cs,
                                                    uint64_t nchunks, ChunkDesc* __restrict__ desc) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= nchunks) return;
    uint64_t lo = 0, hi = n_docs;   // chunk_base[lo] <= c < chunk_base[hi] (chunk_base[n_docs] = nchunks)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (chunk_base[mid] <= c) lo = mid;
        else hi = mid;
    }
    const uint64_t k = c - chunk_base[lo];
    const uint64_t start = doc_off[lo] + k * cs;
    ChunkDesc e;
    e.c0 = start;
    e.scr = scr_base[lo] + k * cs;
    e.len = (uint32_t)min((uint64_t)cs, doc_off[lo + 1] - start);
    e.pad[0] = e.pad[1] = e.pad[2] = 0;
    desc[c] = e;
}

// k_trie_walk with the chunk taken from its descriptor; input words are read
// aligned to the buffer and the last partial word byte by byte (inside [0, n))
template <typename T>
__global__ __launch_bounds__(WALK_TPB) void k_trie_walk_batch(const uint8_t* __restrict__ in, uint64_t n,
                                                              const ChunkDesc* __restrict__ desc,
                                                              const uint4* __restrict__ rec, uint32_t nrec,
                                                              const uint4* __restrict__ root, T* __restrict__ scratch,
                                                              uint32_t* __restrict__ counts, uint64_t nchunks) {
    __shared__ uint4 lut[256];   // byte -> {state, base, tokenId, present}
    lut[threadIdx.x] = root[threadIdx.x];
    __syncthreads();
    const uint64_t chunk = (uint64_t)blockIdx.x * WALK_TPB + threadIdx.x;
    if (chunk >= nchunks) return;
    const ChunkDesc dsc = desc[chunk];
    const uint64_t c0 = dsc.c0;
    const uint64_t ce = c0 + dsc.len;
    T* out = scratch + dsc.scr;
    const uint32_t* in32 = reinterpret_cast<const uint32_t*>(in);
    uint64_t widx = ~0ull;
    uint32_t word = 0;
    auto byte_at = [&](uint64_t p) -> uint32_t {
        const uint64_t wi = p >> 2;
        if (wi != widx) {
            if (wi * 4 + 4 <= n) {
                word = in32[wi];
            } else {
                word = 0;
                for (uint64_t j = wi * 4; j < n; ++j) word |= (uint32_t)in[j] << ((j & 3u) * 8u);
            }
            widx = wi;
        }
        return (word >> ((p & 3u) * 8u)) & 0xFFu;
    };
    uint32_t cnt = 0;
    uint64_t pos = c0;
    while (pos < ce) {
        const uint32_t c = byte_at(pos);
        const uint4 e = lut[c];
        uint32_t lmt = INV;
        uint64_t lmp = pos;
        if (e.w) {
            uint32_t s = e.x, base = e.y;
            if (e.z != INV) {
                lmt = e.z;
                lmp = pos + 1;
            }
            uint64_t wp = pos + 1;
            while (wp < ce) {
                const uint32_t t = base + byte_at(wp);
                if (t >= nrec) break;
                const uint4 r = rec[t];
                if (r.x != s) break;
                s = t;
                base = r.y;
                ++wp;
                if (r.z != INV) {
                    lmt = r.z;
                    lmp = wp;
                }
            }
        }
        if (lmt != INV) {
            out[cnt++] = (T)lmt;
            pos = lmp;
        } else {   // no token starts here: emit the raw byte value (tokenize.wgsl:169-171)
            out[cnt++] = (T)c;
            ++pos;
        }
    }
    counts[chunk] = cnt;
}

// k_trie_walk_v5 with the chunk taken from its descriptor.  A chunk starts on any
// byte, so the 64-byte windows are aligned to the BUFFER (the window base is the
// chunk start rounded down to 64; the chunk's first byte sits at offset c0 & 63 of
// its first window): every refill is still one whole cache line and one aligned
// 4 x 16-byte load.  A window may hold bytes of the neighbouring documents; the
// walk only ever asks for bytes below its own `ce`.  Token vectors go to the
// document's slot (scr_base and cs are multiples of 8: 16-byte aligned stores).
template <typename T>
__global__ __launch_bounds__(WALK_TPB) void k_trie_walk_v5_batch(const uint8_t* __restrict__ in, uint64_t n,
                                                                 const ChunkDesc* __restrict__ desc,
                                                                 const uint2* __restrict__ rec, uint32_t nrec,
                                                                 uint32_t root_base, T* __restrict__ scratch,
                                                                 uint32_t* __restrict__ counts, uint64_t nchunks) {
    constexpr uint32_t PER = 16 / sizeof(T);
    __shared__ uint2 lut[256];
    {
        const uint32_t t = root_base + threadIdx.x;
        lut[threadIdx.x] = t < nrec ? rec[t] : make_uint2(0x3FFFFFu, 0u);
    }
    __syncthreads();
    const uint64_t chunk = (uint64_t)blockIdx.x * WALK_TPB + threadIdx.x;
    if (chunk >= nchunks) return;
    const ChunkDesc dsc = desc[chunk];
    const uint64_t a0 = dsc.c0 & ~63ull;            // the first window's base, aligned to the buffer
    const uint32_t sh = (uint32_t)(dsc.c0 & 63u);   // the chunk's first byte inside it
    const uint32_t ce = dsc.len;
    T* out = scratch + dsc.scr;
    uint32_t cb = ~0u;
    Win64 w64{};
    uint4 acc = make_uint4(0, 0, 0, 0);
    auto byte_at = [&](uint32_t p) -> uint32_t {
        const uint32_t q = p + sh;   // (cs <= 2^31: no wrap)
        const uint32_t b = q & ~63u;
        if (b != cb) {
            cb = b;
            w64 = load_win64(in, n, a0 + b);
        }
        return win64_byte(w64, q & 63u);
    };
    uint32_t cnt = 0, nq = 0;
    uint4 q[WALK_QV > 1 ? WALK_QV - 1 : 1];   // q[WALK_QV-1-nq ..]: the nq waiting vectors, oldest first
    auto emit = [&](uint32_t tok) {
        vec_put<T>(acc, cnt % PER, tok);
        if (++cnt % PER == 0) {
            if (nq == WALK_QV - 1) {
                uint4* o = reinterpret_cast<uint4*>(out + cnt) - WALK_QV;
#pragma unroll
                for (uint32_t i = 0; i + 1 < WALK_QV; ++i) o[i] = q[i];
                o[WALK_QV - 1] = acc;
                nq = 0;
            } else {
                if constexpr (WALK_QV > 1) {
#pragma unroll
                    for (uint32_t i = 0; i + 2 < WALK_QV; ++i) q[i] = q[i + 1];
                    q[WALK_QV - 2] = acc;
                }
                ++nq;
            }
            acc = make_uint4(0, 0, 0, 0);
        }
    };
    auto flush = [&]() {   // the waiting vectors end where the partial vector starts
        if constexpr (WALK_QV > 1) {
            uint4* o = reinterpret_cast<uint4*>(out + (cnt / PER) * PER);
#pragma unroll
            for (uint32_t i = 0; i + 1 < WALK_QV; ++i)
                if (i + nq >= WALK_QV - 1) o[(int)i - (int)WALK_QV + 1] = q[i];
            nq = 0;
        }
    };
    uint32_t pos = 0, wp = 0, lmp = 0, st = 0, base = 0, lmt = TID_NONE, first = 0;
    bool walking = false;
    while (pos < ce) {
        if (!walking) {   // a token start: LDS only
            first = byte_at(pos);
            const uint2 e = lut[first];
            const uint32_t tid = rec_tid(e);
            if (rec_check(e) != 0u || rec_base(e) == 0u || pos + 1 >= ce) {
                emit(rec_check(e) == 0u && tid != TID_NONE ? tid : first);
                ++pos;
                continue;
            }
            st = root_base + first;
            base = rec_base(e);
            lmt = tid;
            lmp = pos + 1;
            wp = pos + 1;
            walking = true;
        }
        // one trie transition: the trip's L2 load
        const uint32_t t = base + byte_at(wp);
        const uint2 r = t < nrec ? rec[t] : make_uint2(0x3FFFFFu, 0u);
        bool end = true;
        if (rec_check(r) == st) {
            st = t;
            base = rec_base(r);
            ++wp;
            const uint32_t tid = rec_tid(r);
            if (tid != TID_NONE) {
                lmt = tid;
                lmp = wp;
            }
            end = base == 0u || wp >= ce;
        }
        if (end) {   // the longest match ends: emit it (or the raw first byte), restart after it
            const bool hit = lmt != TID_NONE;
            emit(hit ? lmt : first);
            pos = hit ? lmp : pos + 1;
            walking = false;
        }
    }
    flush();
    // (at most PER - 1 elements past the count: inside the document's rounded slot)
    if (cnt % PER) *reinterpret_cast<uint4*>(out + (cnt / PER) * PER) = acc;
    counts[chunk] = cnt;
}

// k_chunk_compact4 with each chunk's source taken from its descriptor
template <typename T>
__global__ __launch_bounds__(256) void k_chunk_compact4_batch(const T* __restrict__ scratch,
                                                              const ChunkDesc* __restrict__ desc,
                                                              const uint32_t* __restrict__ counts,
                                                              const uint32_t* __restrict__ local,
                                                              const uint64_t* __restrict__ blocksum, uint64_t nchunks,
                                                              uint32_t* __restrict__ out, uint64_t out_cap) {
    __shared__ uint64_t s_off[4 * CPW];
    __shared__ uint64_t s_src[4 * CPW];
    __shared__ uint32_t s_cnt[4 * CPW];
    const uint64_t c0 = (uint64_t)blockIdx.x * (4 * CPW);
    if (threadIdx.x < 4 * CPW) {
        const uint64_t c = c0 + threadIdx.x;
        s_cnt[threadIdx.x] = c < nchunks ? counts[c] : 0u;
        s_off[threadIdx.x] = c < nchunks ? blocksum[c / SCAN_BLK] + local[c] : 0ull;
        s_src[threadIdx.x] = c < nchunks ? desc[c].scr : 0ull;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t most = 0;
#pragma unroll
    for (int q = 0; q < CPW; ++q) most = max(most, s_cnt[wid * CPW + q]);
    for (uint32_t b0 = 0; b0 < most; b0 += 256) {
        uint32_t v[CPW][4];
#pragma unroll
        for (int q = 0; q < CPW; ++q) {
            const uint32_t cnt = s_cnt[wid * CPW + q];
            const T* src = scratch + s_src[wid * CPW + q];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t j = b0 + lane + 64u * k;
                v[q][k] = j < cnt ? (uint32_t)src[j] : 0u;
            }
        }
#pragma unroll
        for (int q = 0; q < CPW; ++q) {
            const uint32_t cnt = s_cnt[wid * CPW + q];
            const uint64_t off = s_off[wid * CPW + q];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t j = b0 + lane + 64u * k;
                if (j < cnt && off + j < out_cap) out[off + j] = v[q][k];
            }
        }
    }
}

// one lane per document (+ the closing entry): its first token's position — the
// scanned offset of its first chunk; a document without chunks starts where the
// next one with chunks does, or at the total
__global__ __launch_bounds__(256) void k_doc_tok_off(const uint64_t* __restrict__ chunk_base,
                                                     const uint32_t* __restrict__ local,
                                                     const uint64_t* __restrict__ blocksum,
                                                     const uint64_t* __restrict__ total, uint64_t n_docs,
                                                     uint64_t nchunks, uint64_t* __restrict__ tok_off) {
    const uint64_t d = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (d > n_docs) return;
    const uint64_t c = d < n_docs ? chunk_base[d] : nchunks;
    tok_off[d] = c < nchunks ? blocksum[c / SCAN_BLK] + local[c] : *total;
}

}  // namespace

struct gbpe_trie {
    gbpe_ctx* ctx = nullptr;
    uint4* rec = nullptr;      // double-array records {check, base, tokenId, 0}
    uint2* rec2 = nullptr;     // packed 8-byte records (pack_rec); null when ids / states do not fit
    uint32_t root_base = 0;    // base of the root state
    uint32_t nrec = 0;
    uint4* root = nullptr;     // 256 root transitions {state, base, tokenId, present}
    uint32_t max_token_len = 0;
    uint32_t max_token_id = 0;
    uint32_t n_nodes = 0, n_edges = 0;
};

extern "C" int gbpe_trie_upload(gbpe_ctx* ctx, const uint32_t* nodes, uint32_t n_nodes, const uint32_t* edges,
                                uint32_t n_edges, gbpe_trie** out) {
    if (!ctx || !out || !nodes || n_nodes == 0 || (!edges && n_edges))
        return gbpe_set_error(ctx, GBPE_E_INVALID, "trie upload: bad arguments");
    *out = nullptr;
    // ── compile the BFS trie into a double array ──
    // state ids: root = 0 (never a transition target); every other node gets
    // slot base(parent) + byte.
    std::vector<uint32_t> state(n_nodes, INV), depth(n_nodes, 0);
    std::vector<uint4> rec(1, make_uint4(INV, 0, INV, 0));  // slot 0 reserved for the root
    std::vector<uint8_t> used(1, 1);
    uint32_t first_free = 1;
    std::vector<uint32_t> queue;
    queue.reserve(n_nodes);
    queue.push_back(0);
    state[0] = 0;
    uint32_t max_len = 0, max_tid = 0, root_base = 0;
    auto ensure = [&](uint64_t sz) {
        if (sz > rec.size()) {
            rec.resize(sz, make_uint4(INV, 0, INV, 0));
            used.resize(sz, 0);
        }
    };
    std::vector<uint4> root(256, make_uint4(0, 0, INV, 0));
    for (size_t qi = 0; qi < queue.size(); ++qi) {
        const uint32_t u = queue[qi];
        const uint32_t fc = nodes[3 * (uint64_t)u], nc = nodes[3 * (uint64_t)u + 1] & 0xFFFFu;
        if (nc && (uint64_t)fc + nc > n_edges)
            return gbpe_set_error(ctx, GBPE_E_INVALID, "trie upload: node %u edges out of range", u);
        uint32_t prev = 0;
        for (uint32_t k = 0; k < nc; ++k) {
            uint32_t c = edges[2 * ((uint64_t)fc + k)] & 0xFFu;
            if (k && c <= prev)
                return gbpe_set_error(ctx, GBPE_E_INVALID, "trie upload: children of node %u not sorted/unique", u);
            prev = c;
        }
        if (nc == 0) continue;
        const uint32_t cmin = edges[2 * (uint64_t)fc] & 0xFFu;
        // first-fit base search
        uint32_t b = first_free > cmin ? first_free - cmin : 1;
        if (b < 1) b = 1;
        for (;; ++b) {
            ensure((uint64_t)b + 256);
            bool ok = true;
            for (uint32_t k = 0; k < nc && ok; ++k) ok = !used[b + (edges[2 * ((uint64_t)fc + k)] & 0xFFu)];
            if (ok) break;
        }
        const uint32_t su = state[u];
        if (u != 0) rec[su].y = b;
        else root_base = b;
        for (uint32_t k = 0; k < nc; ++k) {
            const uint32_t c = edges[2 * ((uint64_t)fc + k)] & 0xFFu;
            const uint32_t v = edges[2 * ((uint64_t)fc + k) + 1];
            if (v >= n_nodes || v == 0) return gbpe_set_error(ctx, GBPE_E_INVALID, "trie upload: bad edge target %u", v);
            if (state[v] != INV) return gbpe_set_error(ctx, GBPE_E_INVALID, "trie upload: node %u reached twice (not a tree)", v);
            const uint32_t t = b + c;
            used[t] = 1;
            state[v] = t;
            depth[v] = depth[u] + 1;
            const uint32_t tid = nodes[3 * (uint64_t)v + 2];
            rec[t] = make_uint4(su, 0, tid, 0);
            if (tid != INV) {
                max_len = std::max(max_len, depth[v]);
                max_tid = std::max(max_tid, tid);
            }
            queue.push_back(v);
            if (u == 0) root[c] = make_uint4(t, 0, tid, 1);
        }
        while (first_free < used.size() && used[first_free]) ++first_free;
    }
    // root LUT entries need their child's base (filled after the BFS)
    for (int c = 0; c < 256; ++c)
        if (root[c].w) root[c].y = rec[root[c].x].y;
    auto* tr = new (std::nothrow) gbpe_trie();
    if (!tr) return gbpe_set_error(ctx, GBPE_E_OOM, "host allocation failed");
    tr->ctx = ctx;
    tr->nrec = (uint32_t)rec.size();
    tr->max_token_len = max_len;
    tr->max_token_id = max_tid;
    tr->n_nodes = n_nodes;
    tr->n_edges = n_edges;
    tr->root_base = root_base;
    hipError_t e = dev_malloc(ctx, &tr->rec, rec.size() * sizeof(uint4));
    if (e == hipSuccess) e = dev_malloc(ctx, &tr->root, 256 * sizeof(uint4));
    if (e == hipSuccess) e = hipMemcpy(tr->rec, rec.data(), rec.size() * sizeof(uint4), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(tr->root, root.data(), 256 * sizeof(uint4), hipMemcpyHostToDevice);
    // packed records: check (22 bits) | tid low 10 << 22, base (22 bits) | tid high 10 << 22
    const bool packable = rec.size() + 256 < 0x3FFFFFu && max_tid < 0xFFFFFu;
    if (e == hipSuccess && packable) {
        std::vector<uint2> r2(rec.size() + 256);
        for (size_t i = 0; i < r2.size(); ++i) {
            const uint4 q = i < rec.size() ? rec[i] : make_uint4(INV, 0, INV, 0);
            const uint32_t chk = q.x == INV ? 0x3FFFFFu : q.x;
            const uint32_t tid = q.z == INV ? 0xFFFFFu : q.z;
            r2[i] = make_uint2(chk | ((tid & 0x3FFu) << 22), (q.y & 0x3FFFFFu) | ((tid >> 10) << 22));
        }
        e = dev_malloc(ctx, &tr->rec2, r2.size() * sizeof(uint2));
        if (e == hipSuccess) e = hipMemcpy(tr->rec2, r2.data(), r2.size() * sizeof(uint2), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        gbpe_trie_free(tr);
        return gbpe_set_error(ctx, GBPE_E_DEVICE, "trie upload failed: %s", hipGetErrorString(e));
    }
    *out = tr;
    return GBPE_OK;
}

extern "C" int gbpe_trie_info(const gbpe_trie* tr, uint32_t* n_records, uint32_t* max_token_len, uint32_t* max_token_id) {
    if (!tr) return GBPE_E_INVALID;
    if (n_records) *n_records = tr->nrec;
    if (max_token_len) *max_token_len = tr->max_token_len;
    if (max_token_id) *max_token_id = tr->max_token_id;
    return GBPE_OK;
}

extern "C" void gbpe_trie_free(gbpe_trie* tr) {
    if (!tr) return;
    hipFree(tr->rec);
    hipFree(tr->rec2);
    hipFree(tr->root);
    delete tr;
}

namespace {

uint32_t effective_cs(const gbpe_trie* tr, uint32_t cs) {
    if (cs) return cs;
    // tokenizer.js:67-68 adaptive chunk
    const uint32_t a = tr->max_token_len * 8u;
    return std::max<uint32_t>(512u, std::min<uint32_t>(2048u, a));
}

// runs the three encode kernels on device buffers; *total_dev receives the count
int encode_device_impl(gbpe_ctx* ctx, gbpe_trie* tr, const uint8_t* d_in, uint64_t n, uint32_t cs, uint32_t* d_out,
                       uint64_t out_cap, uint64_t* n_out) {
    hipStream_t s = ctx->stream;
    const uint64_t nchunks = gbpe_div_up(n, cs);
    const bool narrow = tr->max_token_id < 65536u;   // raw-byte fallbacks are < 256
    const uint64_t esz = narrow ? 2 : 4;
    const uint64_t nblk = gbpe_div_up(nchunks, SCAN_BLK);
    GBPE_HIP(ctx, ctx->enc_scratch.reserve(ctx, nchunks * cs * esz + 16));
    GBPE_HIP(ctx, ctx->enc_counts.reserve(ctx, nchunks * 8 + nblk * 8 + 64));
    uint32_t* counts = (uint32_t*)ctx->enc_counts.p;
    uint32_t* local = counts + nchunks;
    uint64_t* blocksum = (uint64_t*)(((uintptr_t)(local + nchunks) + 15) & ~(uintptr_t)15);
    uint64_t* d_total = blocksum + nblk + 1;
    const uint32_t gw = (uint32_t)gbpe_div_up(nchunks, WALK_TPB);
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[0], s));
    // the packed-record state-machine walk when the trie packs and chunks are whole
    // 16-byte token vectors (cs % 8 == 0: every adaptive chunk size); otherwise the
    // plain per-token walk over 16-byte records
    const bool packed = (cs % 8u) == 0u && tr->rec2;
    const uint32_t nrec2 = tr->nrec + 256;
    if (packed && narrow)
        hipLaunchKernelGGL(k_trie_walk_v5<uint16_t>, dim3(gw), dim3(WALK_TPB), 0, s, d_in, n, cs, tr->rec2, nrec2,
                           tr->root_base, (uint16_t*)ctx->enc_scratch.p, counts, nchunks);
    else if (packed)
        hipLaunchKernelGGL(k_trie_walk_v5<uint32_t>, dim3(gw), dim3(WALK_TPB), 0, s, d_in, n, cs, tr->rec2, nrec2,
                           tr->root_base, (uint32_t*)ctx->enc_scratch.p, counts, nchunks);
    else if (narrow)
        hipLaunchKernelGGL(k_trie_walk<uint16_t>, dim3(gw), dim3(WALK_TPB), 0, s, d_in, n, cs, tr->rec, tr->nrec,
                           tr->root, (uint16_t*)ctx->enc_scratch.p, counts, nchunks);
    else
        hipLaunchKernelGGL(k_trie_walk<uint32_t>, dim3(gw), dim3(WALK_TPB), 0, s, d_in, n, cs, tr->rec, tr->nrec,
                           tr->root, (uint32_t*)ctx->enc_scratch.p, counts, nchunks);
    GBPE_LAUNCH_CHECK(ctx);
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[1], s));
    hipLaunchKernelGGL(k_chunk_scan1, dim3((uint32_t)nblk), dim3(SCAN_TPB), 0, s, (const uint32_t*)counts, nchunks, local,
                       blocksum);
    hipLaunchKernelGGL(k_chunk_scan2, dim3(1), dim3(SCAN_TPB), 0, s, blocksum, nblk, d_total);
    GBPE_LAUNCH_CHECK(ctx);
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[2], s));
    const uint32_t gc4 = (uint32_t)gbpe_div_up(nchunks, 4 * CPW);
    if (narrow)
        hipLaunchKernelGGL(k_chunk_compact4<uint16_t>, dim3(gc4), dim3(256), 0, s, (const uint16_t*)ctx->enc_scratch.p,
                           (const uint32_t*)counts, (const uint32_t*)local, (const uint64_t*)blocksum, nchunks, cs, d_out,
                           out_cap);
    else
        hipLaunchKernelGGL(k_chunk_compact4<uint32_t>, dim3(gc4), dim3(256), 0, s, (const uint32_t*)ctx->enc_scratch.p,
                           (const uint32_t*)counts, (const uint32_t*)local, (const uint64_t*)blocksum, nchunks, cs, d_out,
                           out_cap);
    GBPE_LAUNCH_CHECK(ctx);
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[3], s));
    GBPE_HIP(ctx, hipMemcpyAsync(ctx->enc_host_total, d_total, 8, hipMemcpyDeviceToHost, s));
    GBPE_HIP(ctx, hipStreamSynchronize(s));
    float a = 0, b = 0, c = 0;
    hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[1]);
    hipEventElapsedTime(&b, ctx->ev[1], ctx->ev[2]);
    hipEventElapsedTime(&c, ctx->ev[2], ctx->ev[3]);
    ctx->enc_ms[0] = a;
    ctx->enc_ms[1] = b;
    ctx->enc_ms[2] = c;
    uint64_t total;
    memcpy(&total, ctx->enc_host_total, 8);
    *n_out = total;
    if (total > out_cap) return gbpe_set_error(ctx, GBPE_E_CAPACITY, "encode: output needs %llu tokens", (unsigned long long)total);
    return GBPE_OK;
}

// bytes of ctx->enc_docs the batch encode's per-document table takes for n_docs
// documents: chunk_base + scr_base (n_docs + 1 each), the table blocks' totals
// (two arrays), the grand totals and the invalid flag
uint64_t doc_table_bytes(uint64_t n_docs) {
    const uint64_t ndblk = gbpe_div_up(n_docs, DOC_TPB);
    return 2 * (n_docs + 1) * 8 + 2 * (ndblk + 1) * 8 + sizeof(DocTotals) + 8 + 64;
}

// The batch pipeline on device buffers (n, n_docs > 0): table + scans (one
// readback: the chunk count sizes the grid, the slot total the scratch),
// descriptors, walk, count scan, compact, document token offsets.
int encode_batch_device_impl(gbpe_ctx* ctx, gbpe_trie* tr, const uint8_t* d_in, uint64_t n, const uint64_t* d_doc_off,
                             uint64_t n_docs, uint32_t cs, uint32_t* d_out, uint64_t out_cap, uint64_t* d_tok_off,
                             uint64_t* n_out) {
    hipStream_t s = ctx->stream;
    const bool narrow = tr->max_token_id < 65536u;   // raw-byte fallbacks are < 256
    const uint64_t esz = narrow ? 2 : 4;
    const uint64_t ndblk = gbpe_div_up(n_docs, DOC_TPB);
    GBPE_HIP(ctx, ctx->enc_docs.reserve(ctx, doc_table_bytes(n_docs)));
    uint64_t* chunk_base = (uint64_t*)ctx->enc_docs.p;
    uint64_t* scr_base = chunk_base + n_docs + 1;
    uint64_t* blk_ch = scr_base + n_docs + 1;
    uint64_t* blk_scr = blk_ch + ndblk + 1;
    DocTotals* d_totals = (DocTotals*)(blk_scr + ndblk + 1);
    uint32_t* d_invalid = (uint32_t*)(d_totals + 1);
    GBPE_HIP(ctx, hipMemsetAsync(d_invalid, 0, 4, s));
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[4], s));
    hipLaunchKernelGGL(k_doc_table, dim3((uint32_t)ndblk), dim3(DOC_TPB), 0, s, d_doc_off, n_docs, n, cs, chunk_base,
                       scr_base, blk_ch, blk_scr, d_invalid);
    hipLaunchKernelGGL(k_doc_scan2, dim3(1), dim3(DOC_TPB), 0, s, blk_ch, blk_scr, ndblk, (const uint32_t*)d_invalid,
                       d_totals);
    hipLaunchKernelGGL(k_doc_base, dim3((uint32_t)gbpe_div_up(n_docs + 1, DOC_TPB)), dim3(DOC_TPB), 0, s, chunk_base,
                       scr_base, (const uint64_t*)blk_ch, (const uint64_t*)blk_scr, n_docs, (const DocTotals*)d_totals);
    GBPE_LAUNCH_CHECK(ctx);
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[5], s));
    GBPE_HIP(ctx, hipMemcpyAsync(ctx->enc_host_total, d_totals, sizeof(DocTotals), hipMemcpyDeviceToHost, s));
    GBPE_HIP(ctx, hipStreamSynchronize(s));
    DocTotals tot;
    memcpy(&tot, ctx->enc_host_total, sizeof(tot));
    if (tot.invalid) return gbpe_doc_offsets_error(ctx, "encode batch", (uint32_t)tot.invalid);   // nothing else was launched
    const uint64_t nchunks = tot.nchunks;
    if (nchunks == 0) return gbpe_set_error(ctx, GBPE_E_INTERNAL, "encode batch: no chunks for %llu bytes", (unsigned long long)n);
    const uint64_t nblk = gbpe_div_up(nchunks, SCAN_BLK);
    // scratch: one rounded slot per document, O(n + n_docs) elements
    GBPE_HIP(ctx, ctx->enc_scratch.reserve(ctx, tot.scr_elems * esz + 16));
    GBPE_HIP(ctx, ctx->enc_counts.reserve(ctx, nchunks * 8 + nblk * 8 + 64 + 16 + nchunks * sizeof(ChunkDesc)));
    uint32_t* counts = (uint32_t*)ctx->enc_counts.p;
    uint32_t* local = counts + nchunks;
    uint64_t* blocksum = (uint64_t*)(((uintptr_t)(local + nchunks) + 15) & ~(uintptr_t)15);
    uint64_t* d_total = blocksum + nblk + 1;
    ChunkDesc* desc = (ChunkDesc*)(((uintptr_t)(d_total + 1) + 15) & ~(uintptr_t)15);
    const uint32_t gw = (uint32_t)gbpe_div_up(nchunks, WALK_TPB);
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[6], s));
    hipLaunchKernelGGL(k_chunk_desc, dim3((uint32_t)gbpe_div_up(nchunks, 256)), dim3(256), 0, s, d_doc_off,
                       (const uint64_t*)chunk_base, (const uint64_t*)scr_base, n_docs, cs, nchunks, desc);
    GBPE_LAUNCH_CHECK(ctx);
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[0], s));
    // path selection as in encode_device_impl
    const bool packed = (cs % 8u) == 0u && tr->rec2;
    const uint32_t nrec2 = tr->nrec + 256;
    if (packed && narrow)
        hipLaunchKernelGGL(k_trie_walk_v5_batch<uint16_t>, dim3(gw), dim3(WALK_TPB), 0, s, d_in, n, (const ChunkDesc*)desc,
                           tr->rec2, nrec2, tr->root_base, (uint16_t*)ctx->enc_scratch.p, counts, nchunks);
    else if (packed)
        hipLaunchKernelGGL(k_trie_walk_v5_batch<uint32_t>, dim3(gw), dim3(WALK_TPB), 0, s, d_in, n, (const ChunkDesc*)desc,
                           tr->rec2, nrec2, tr->root_base, (uint32_t*)ctx->enc_scratch.p, counts, nchunks);
    else if (narrow)
        hipLaunchKernelGGL(k_trie_walk_batch<uint16_t>, dim3(gw), dim3(WALK_TPB), 0, s, d_in, n, (const ChunkDesc*)desc,
                           tr->rec, tr->nrec, tr->root, (uint16_t*)ctx->enc_scratch.p, counts, nchunks);
    else
        hipLaunchKernelGGL(k_trie_walk_batch<uint32_t>, dim3(gw), dim3(WALK_TPB), 0, s, d_in, n, (const ChunkDesc*)desc,
                           tr->rec, tr->nrec, tr->root, (uint32_t*)ctx->enc_scratch.p, counts, nchunks);
    GBPE_LAUNCH_CHECK(ctx);
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[1], s));
    hipLaunchKernelGGL(k_chunk_scan1, dim3((uint32_t)nblk), dim3(SCAN_TPB), 0, s, (const uint32_t*)counts, nchunks, local,
                       blocksum);
    hipLaunchKernelGGL(k_chunk_scan2, dim3(1), dim3(SCAN_TPB), 0, s, blocksum, nblk, d_total);
    GBPE_LAUNCH_CHECK(ctx);
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[2], s));
    const uint32_t gc4 = (uint32_t)gbpe_div_up(nchunks, 4 * CPW);
    if (narrow)
        hipLaunchKernelGGL(k_chunk_compact4_batch<uint16_t>, dim3(gc4), dim3(256), 0, s,
                           (const uint16_t*)ctx->enc_scratch.p, (const ChunkDesc*)desc, (const uint32_t*)counts,
                           (const uint32_t*)local, (const uint64_t*)blocksum, nchunks, d_out, out_cap);
    else
        hipLaunchKernelGGL(k_chunk_compact4_batch<uint32_t>, dim3(gc4), dim3(256), 0, s,
                           (const uint32_t*)ctx->enc_scratch.p, (const ChunkDesc*)desc, (const uint32_t*)counts,
                           (const uint32_t*)local, (const uint64_t*)blocksum, nchunks, d_out, out_cap);
    // (runs whether or not the tokens fit: tok_off is complete on GBPE_E_CAPACITY)
    hipLaunchKernelGGL(k_doc_tok_off, dim3((uint32_t)gbpe_div_up(n_docs + 1, 256)), dim3(256), 0, s,
                       (const uint64_t*)chunk_base, (const uint32_t*)local, (const uint64_t*)blocksum,
                       (const uint64_t*)d_total, n_docs, nchunks, d_tok_off);
    GBPE_LAUNCH_CHECK(ctx);
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[3], s));
    GBPE_HIP(ctx, hipMemcpyAsync(ctx->enc_host_total, d_total, 8, hipMemcpyDeviceToHost, s));
    GBPE_HIP(ctx, hipStreamSynchronize(s));
    float a = 0, b = 0, c = 0, t0 = 0, t1 = 0;
    hipEventElapsedTime(&t0, ctx->ev[4], ctx->ev[5]);
    hipEventElapsedTime(&t1, ctx->ev[6], ctx->ev[0]);
    hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[1]);
    hipEventElapsedTime(&b, ctx->ev[1], ctx->ev[2]);
    hipEventElapsedTime(&c, ctx->ev[2], ctx->ev[3]);
    ctx->enc_ms[0] = a;
    ctx->enc_ms[1] = (double)t0 + t1 + b;   // every scan and table kernel
    ctx->enc_ms[2] = c;
    uint64_t total;
    memcpy(&total, ctx->enc_host_total, 8);
    *n_out = total;
    if (total > out_cap)
        return gbpe_set_error(ctx, GBPE_E_CAPACITY, "encode batch: output needs %llu tokens", (unsigned long long)total);
    return GBPE_OK;
}

constexpr uint32_t kBatchMaxChunk = 1u << 31;   // the batch walk's in-chunk positions are 32-bit

}  // namespace

extern "C" int gbpe_encode_batch_device(gbpe_ctx* ctx, gbpe_trie* tr, const void* d_bytes, uint64_t n,
                                        const void* d_doc_off, uint64_t n_docs, uint32_t chunk_size, void* d_out,
                                        uint64_t out_cap, void* d_tok_off, uint64_t* n_out) {
    if (!ctx || !tr || !n_out || !d_tok_off || (n_docs && !d_doc_off) || (n && n_docs && (!d_bytes || (!d_out && out_cap))))
        return gbpe_set_error(ctx, GBPE_E_INVALID, "null argument");
    if ((uintptr_t)d_bytes & 15u) return gbpe_set_error(ctx, GBPE_E_INVALID, "d_bytes must be 16-byte aligned");
    if (((uintptr_t)d_doc_off | (uintptr_t)d_tok_off) & 7u)
        return gbpe_set_error(ctx, GBPE_E_INVALID, "d_doc_off and d_tok_off must be 8-byte aligned");
    const uint32_t cs = effective_cs(tr, chunk_size);
    if (cs > kBatchMaxChunk) return gbpe_set_error(ctx, GBPE_E_INVALID, "encode batch: chunk size above 2^31");
    *n_out = 0;
    if (n_docs == 0 || n == 0) {
        GBPE_HIP(ctx, hipMemsetAsync(d_tok_off, 0, (n_docs + 1) * 8, ctx->stream));
        GBPE_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return GBPE_OK;
    }
    return encode_batch_device_impl(ctx, tr, (const uint8_t*)d_bytes, n, (const uint64_t*)d_doc_off, n_docs, cs,
                                    (uint32_t*)d_out, out_cap, (uint64_t*)d_tok_off, n_out);
}

// Host buffers in and out.  The offsets are checked here, before anything is
// launched.  Inputs above the encode slice run as groups of whole documents (a
// document above the slice is its own group), one group after the other through the
// device pipeline: a group's bytes, its offsets rebased to its first byte, and back
// its tokens and token offsets, which the running total shifts.
extern "C" int gbpe_encode_batch(gbpe_ctx* ctx, gbpe_trie* tr, const uint8_t* bytes, uint64_t n, const uint64_t* doc_off,
                                 uint64_t n_docs, uint32_t chunk_size, uint32_t* out, uint64_t out_cap,
                                 uint64_t* tok_off, uint64_t* n_out) {
    if (!ctx || !tr || !n_out || !tok_off || (n_docs && !doc_off) || (n && !bytes) || (out_cap && !out))
        return gbpe_set_error(ctx, GBPE_E_INVALID, "null argument");
    *n_out = 0;
    if (n_docs == 0) {
        tok_off[0] = 0;
        return GBPE_OK;
    }
    int rc = gbpe_doc_offsets_check(ctx, "encode batch", doc_off, n_docs, n);
    if (rc != GBPE_OK) return rc;
    const uint32_t cs = effective_cs(tr, chunk_size);
    if (cs > kBatchMaxChunk) return gbpe_set_error(ctx, GBPE_E_INVALID, "encode batch: chunk size above 2^31");
    if (n == 0) {
        for (uint64_t d = 0; d <= n_docs; ++d) tok_off[d] = 0;
        return GBPE_OK;
    }
    const uint64_t slice = (uint64_t)std::max<long>(1, gbpe_debug_knob("encode_slice", (long)kEncSlice));
    // the groups: [g0, g1) with at most `slice` bytes, or one document
    auto group_end = [&](uint64_t g0) {
        uint64_t g1 = g0 + 1;
        while (g1 < n_docs && doc_off[g1 + 1] - doc_off[g0] <= slice) ++g1;
        return g1;
    };
    uint64_t max_bytes = 0, max_docs = 0;
    for (uint64_t g0 = 0; g0 < n_docs;) {
        const uint64_t g1 = group_end(g0);
        max_bytes = std::max(max_bytes, doc_off[g1] - doc_off[g0]);
        max_docs = std::max(max_docs, g1 - g0);
        g0 = g1;
    }
    const uint64_t table = (doc_table_bytes(max_docs) + 15) & ~15ull;
    GBPE_HIP(ctx, ctx->enc_in.reserve(ctx, max_bytes + 64));
    GBPE_HIP(ctx, ctx->enc_out.reserve(ctx, max_bytes * 4 + 16));   // <= 1 token per byte
    GBPE_HIP(ctx, ctx->enc_docs.reserve(ctx, table + 2 * (max_docs + 1) * 8));
    uint8_t* d_in = (uint8_t*)ctx->enc_in.p;
    uint32_t* d_out = (uint32_t*)ctx->enc_out.p;
    uint64_t* d_doc_off = (uint64_t*)((uint8_t*)ctx->enc_docs.p + table);   // (behind the impl's table)
    uint64_t* d_tok_off = d_doc_off + max_docs + 1;
    std::vector<uint64_t> rel;
    uint64_t total = 0;
    for (uint64_t g0 = 0; g0 < n_docs;) {
        const uint64_t g1 = group_end(g0), nd = g1 - g0;
        const uint64_t b0 = doc_off[g0], len = doc_off[g1] - b0;
        if (len == 0) {   // empty documents only
            for (uint64_t d = g0; d <= g1; ++d) tok_off[d] = total;
            g0 = g1;
            continue;
        }
        rel.resize(nd + 1);
        for (uint64_t d = 0; d <= nd; ++d) rel[d] = doc_off[g0 + d] - b0;
        GBPE_HIP(ctx, hipMemcpyAsync(d_in, bytes + b0, len, hipMemcpyHostToDevice, ctx->stream));
        GBPE_HIP(ctx, hipMemcpyAsync(d_doc_off, rel.data(), (nd + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        GBPE_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (rel is reused by the next group)
        uint64_t t = 0;
        rc = encode_batch_device_impl(ctx, tr, d_in, len, d_doc_off, nd, cs, d_out, len, d_tok_off, &t);
        if (rc != GBPE_OK) return rc;
        GBPE_HIP(ctx, hipMemcpyAsync(tok_off + g0, d_tok_off, (nd + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        const uint64_t fit = total < out_cap ? std::min(t, out_cap - total) : 0;   // never at or beyond out[out_cap]
        if (fit) GBPE_HIP(ctx, hipMemcpyAsync(out + total, d_out, fit * 4, hipMemcpyDeviceToHost, ctx->stream));
        GBPE_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (uint64_t d = g0; d <= g1; ++d) tok_off[d] += total;
        total += t;
        g0 = g1;
    }
    *n_out = total;
    if (total > out_cap)
        return gbpe_set_error(ctx, GBPE_E_CAPACITY, "encode batch: output needs %llu tokens", (unsigned long long)total);
    return GBPE_OK;
}

extern "C" int gbpe_encode_device(gbpe_ctx* ctx, gbpe_trie* tr, const void* d_bytes, uint64_t n, uint32_t chunk_size,
                                  void* d_out, uint64_t out_cap, uint64_t* n_out) {
    if (!ctx || !tr || !n_out || (n && (!d_bytes || !d_out))) return gbpe_set_error(ctx, GBPE_E_INVALID, "null argument");
    *n_out = 0;
    if ((uintptr_t)d_bytes & 3u) return gbpe_set_error(ctx, GBPE_E_INVALID, "d_bytes must be 4-byte aligned");
    if (n == 0) return GBPE_OK;
    return encode_device_impl(ctx, tr, (const uint8_t*)d_bytes, n, effective_cs(tr, chunk_size), (uint32_t*)d_out,
                              out_cap, n_out);
}

// Host buffers in and out (tokenizer.js:213-335 incl. the readback).  Inputs
// larger than one slice run as a pipeline of chunk-aligned slices: while the
// device encodes slice i+1 (after its upload), a second host thread copies slice
// i's tokens back, so uploads, kernels and downloads overlap.  Slices start at
// multiples of 64 * chunk size, so every chunk — and every token — is the one a
// single pass produces.
extern "C" int gbpe_encode(gbpe_ctx* ctx, gbpe_trie* tr, const uint8_t* bytes, uint64_t n, uint32_t chunk_size,
                           uint32_t* out, uint64_t out_cap, uint64_t* n_out) {
    if (!ctx || !tr || !n_out || (n && !bytes)) return gbpe_set_error(ctx, GBPE_E_INVALID, "null argument");
    *n_out = 0;
    if (n == 0) return GBPE_OK;   // tokenizer.js:175
    const uint32_t cs = effective_cs(tr, chunk_size);
    GBPE_HIP(ctx, ctx->enc_in.reserve(ctx, gbpe_div_up(n, 4) * 4 + 16));
    GBPE_HIP(ctx, ctx->enc_out.reserve(ctx, n * 4 + 16));   // <= 1 token per byte
    const uint64_t unit = (uint64_t)cs * 64;
    // (test override: many slices on small inputs)
    const uint64_t want = (uint64_t)std::max<long>(1, gbpe_debug_knob("encode_slice", (long)kEncSlice));
    const uint64_t slice = std::max<uint64_t>(unit, (want / unit) * unit);
    uint8_t* d_in = (uint8_t*)ctx->enc_in.p;
    uint32_t* d_out = (uint32_t*)ctx->enc_out.p;
    int rc = GBPE_OK;
    if (n <= slice) {
        GBPE_HIP(ctx, hipMemcpyAsync(d_in, bytes, n, hipMemcpyHostToDevice, ctx->stream));
        uint64_t total = 0;
        rc = encode_device_impl(ctx, tr, d_in, n, cs, d_out, n, &total);
        *n_out = total;
        if (rc != GBPE_OK) return rc;
        if (total > out_cap)
            return gbpe_set_error(ctx, GBPE_E_CAPACITY, "encode: output needs %llu tokens", (unsigned long long)total);
        if (total) {
            GBPE_HIP(ctx, hipMemcpyAsync(out, d_out, total * 4, hipMemcpyDeviceToHost, ctx->stream));
            GBPE_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        return GBPE_OK;
    }
    if (!ctx->copy_stream) GBPE_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    struct Part {
        uint64_t off, cnt;
    };
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Part> q;
    bool finished = false;
    hipError_t copy_err = hipSuccess;
    hipStream_t so = ctx->copy_stream;
    const int dev = ctx->device;
    std::thread drain([&]() {
        hipSetDevice(dev);
        for (;;) {
            Part p;
            {
                std::unique_lock<std::mutex> g(mu);
                cv.wait(g, [&] { return finished || !q.empty(); });
                if (q.empty()) return;
                p = q.front();
                q.pop_front();
            }
            if (copy_err != hipSuccess) continue;
            hipError_t e = hipMemcpyAsync(out + p.off, d_out + p.off, p.cnt * 4, hipMemcpyDeviceToHost, so);
            if (e == hipSuccess) e = hipStreamSynchronize(so);
            if (e != hipSuccess) copy_err = e;
        }
    });
    uint64_t total = 0;
    for (uint64_t s0 = 0; s0 < n && rc == GBPE_OK; s0 += slice) {
        const uint64_t len = std::min(slice, n - s0);
        hipError_t e = hipMemcpyAsync(d_in + s0, bytes + s0, len, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            rc = gbpe_set_error(ctx, GBPE_E_DEVICE, "encode upload failed: %s", hipGetErrorString(e));
            break;
        }
        uint64_t t = 0;
        rc = encode_device_impl(ctx, tr, d_in + s0, len, cs, d_out + total, n - total, &t);   // (synchronises)
        if (rc != GBPE_OK) break;
        if (t && total + t <= out_cap) {
            std::lock_guard<std::mutex> g(mu);
            q.push_back(Part{total, t});
            cv.notify_one();
        }
        total += t;
    }
    {
        std::lock_guard<std::mutex> g(mu);
        finished = true;
        cv.notify_one();
    }
    drain.join();
    *n_out = total;
    if (rc != GBPE_OK) return rc;
    if (copy_err != hipSuccess) return gbpe_set_error(ctx, GBPE_E_DEVICE, "encode readback failed: %s", hipGetErrorString(copy_err));
    if (total > out_cap) return gbpe_set_error(ctx, GBPE_E_CAPACITY, "encode: output needs %llu tokens", (unsigned long long)total);
    return GBPE_OK;
}

extern "C" int gbpe_encode_last_timing(gbpe_ctx* ctx, double* ms_walk, double* ms_scan, double* ms_compact) {
    if (!ctx) return GBPE_E_INVALID;
    if (ms_walk) *ms_walk = ctx->enc_ms[0];
    if (ms_scan) *ms_scan = ctx->enc_ms[1];
    if (ms_compact) *ms_compact = ctx->enc_ms[2];
    return GBPE_OK;
}
