// cl100k_base word-start kernels.  Included by pretok.hip inside its unnamed namespace, after the
// GPT-4 rule kernels whose staging, decoding and scan helpers these use.
#pragma once

// ── cl100k_base word starts (gbpe_pretokenize_cl100k*) ───────────
//
// The split pattern of cl100k_base over the five classes of unicode_classes_cl100k.h.
// Every rule reads at most four codepoints back and one ahead, apart from three
// segmented scans, each with a two- or three-valued state:
//   d      digits since the run began, mod 3                     (forward)
//   eaten  O sets, CR/LF keeps, anything else clears: the newlines
//          that a run of "other" takes with it                   (forward)
//   later  CR/LF sets, other whitespace keeps, the rest clears: a
//          newline follows in the same whitespace run            (backward)
//   k_ptc_scan1   per 4096-byte block: the forward and the backward aggregate
//   k_ptc_scan2   one workgroup: the forward ones scanned left to right, the backward ones right to left
//   k_ptc_mark    per byte: the rules on the scanned states → word-start byte
// <DOCS>: k_doc_flags' array staged next to the bytes; a flagged byte is byte 0 of its
// text to every look-back, the end of the text before it to every look-ahead and
// decode, and all three scans reset there.
// Each kernel first turns its window of bytes into one code per byte in LDS, and the
// rules read nothing else: bits 0-2 the class of the codepoint that starts here, bits
// 3-6 what the contraction and the space rules compare (K_ID_*), CL_CONT on a
// continuation byte and past the end.
enum : uint32_t { K_L = 0, K_N, K_W, K_R, K_O };
enum : uint32_t { K_ID_S = 1, K_ID_D, K_ID_M, K_ID_T, K_ID_L, K_ID_V, K_ID_E, K_ID_R, K_ID_APOS, K_ID_SPACE };
constexpr uint32_t CL_CONT = 0xFFu;

// (?i:[sdmt]|ll|ve|re) under simple case folding: ASCII either case, and U+017F for s
__device__ __forceinline__ uint32_t cl_id(uint32_t cp) {
    if (cp == 0x17Fu) return K_ID_S;
    if (cp >= 0x80u) return 0u;
    if (cp == 0x27u) return K_ID_APOS;
    if (cp == 0x20u) return K_ID_SPACE;
    switch (cp | 0x20u) {
        case 's': return K_ID_S;
        case 'd': return K_ID_D;
        case 'm': return K_ID_M;
        case 't': return K_ID_T;
        case 'l': return K_ID_L;
        case 'v': return K_ID_V;
        case 'e': return K_ID_E;
        case 'r': return K_ID_R;
    }
    return 0u;
}
__device__ __forceinline__ bool cl_sdmt(uint32_t id) { return id >= K_ID_S && id <= K_ID_T; }
__device__ __forceinline__ bool cl_pair(uint32_t a, uint32_t b) {
    return (a == K_ID_L && b == K_ID_L) || ((a == K_ID_V || a == K_ID_R) && b == K_ID_E);
}

// scan element: bits 0-2 seg_combine's digit run, bits 3-4 a "last one wins" state
// (0 keep, 1 set, 2 clear).  The forward scans use both, the backward scan the state.
constexpr uint32_t CL_SET = 1u << 3, CL_CLEAR = 2u << 3;
__device__ __forceinline__ uint32_t cl_combine(uint32_t a, uint32_t b) {
    return seg_combine(a & 7u, b & 7u) | ((b & 0x18u) ? (b & 0x18u) : (a & 0x18u));
}

// the code of window byte i (global offset base + i, inside [0, n)); W holds 0 past n, and a
// sequence cut by the end of the bytes or (DOCS) by the next document start decodes with 0s
template <bool DOCS>
__device__ __forceinline__ uint32_t cl_code(const uint8_t* W, const uint8_t* F, const uint8_t* ac, int i,
                                            const uint16_t* __restrict__ idx, const uint8_t* __restrict__ cls) {
    const uint32_t b = W[i];
    if (!is_lead(b)) return CL_CONT;
    if (b < 0x80u) return ac[b] | (cl_id(b) << 3);
    const int sz = (b & 0xE0u) == 0xC0u ? 2 : (b & 0xF0u) == 0xE0u ? 3 : 4;
    uint32_t cp = sz == 2 ? (b & 0x1Fu) : sz == 3 ? (b & 0x0Fu) : (b & 0x07u);
    bool open = true;
    for (int j = 1; j < sz; ++j) {
        open = open && i + j < PT_WIN && !(DOCS && F[i + j]);
        cp = (cp << 6) | (open ? (W[i + j] & 0x3Fu) : 0u);
    }
    const uint32_t k = cp >= 0x110000u ? (uint32_t)K_O
                                       : cls[((uint32_t)idx[cp >> kCl100kBlockShift] << kCl100kBlockShift) | (cp & 0xFFu)];
    return k | (cl_id(cp) << 3);
}

// the codes of the block's bytes (16 per thread) and, STAGE_HALO, of the halo; ends with a barrier
template <bool DOCS, bool STAGE_HALO>
__device__ __forceinline__ void cl_codes(const uint8_t* W, const uint8_t* F, const uint8_t* ac, uint8_t* C, int64_t base,
                                         uint64_t n, const uint16_t* __restrict__ idx, const uint8_t* __restrict__ cls) {
    for (int k = 0; k < PT_ITEMS; ++k) {
        const int i = PT_HALO + threadIdx.x * PT_ITEMS + k;
        C[i] = (uint64_t)(base + i) < n ? (uint8_t)cl_code<DOCS>(W, F, ac, i, idx, cls) : (uint8_t)CL_CONT;
    }
    if (STAGE_HALO && threadIdx.x < 2 * PT_HALO) {
        const int i = threadIdx.x < PT_HALO ? threadIdx.x : PT_BLK + threadIdx.x;
        const int64_t g = base + i;
        C[i] = g >= 0 && (uint64_t)g < n ? (uint8_t)cl_code<DOCS>(W, F, ac, i, idx, cls) : (uint8_t)CL_CONT;
    }
    __syncthreads();
}

template <bool DOCS>
struct ClWin {
    const uint8_t* c;   // LDS: the codes of bytes [base, base + PT_WIN)
    const uint8_t* f;   // LDS: the document-start flags of the same window (DOCS)
    int64_t base;
    uint64_t n;
    __device__ __forceinline__ uint32_t code(uint64_t o) const { return c[(int64_t)o - base]; }
    // o is byte 0 of its text
    __device__ __forceinline__ bool first(uint64_t o) const { return o == 0 || (DOCS && f[(int64_t)o - base] != 0); }
    // the lead byte of the codepoint before the one at o; o is not first
    __device__ __forceinline__ uint64_t prev(uint64_t o) const {
        uint64_t p = o - 1;
        while (!first(p) && code(p) == CL_CONT && o - p < 4) --p;
        return p;
    }
    // the code of the codepoint after the one at o, CL_CONT where the text ends first
    __device__ __forceinline__ uint32_t next_code(uint64_t o) const {
        uint64_t q = o + 1;
        while (q < o + 4 && q < n && !first(q) && code(q) == CL_CONT) ++q;
        return q < n && !first(q) ? code(q) : CL_CONT;
    }
    // forward element of byte o: the digit run and `eaten`; a text's first codepoint resets both
    __device__ __forceinline__ uint32_t fwd(uint64_t o) const {
        const uint32_t c0 = code(o);
        if (c0 == CL_CONT) return 0u;
        const uint32_t k = c0 & 7u;
        uint32_t e = (k == K_N ? 1u : 4u) | (k == K_O ? CL_SET : k == K_R ? 0u : CL_CLEAR);
        if (first(o)) e |= 4u | (k == K_R ? CL_CLEAR : 0u);
        return e;
    }
    // backward element of byte o: `later`; nothing after a text's first byte reaches the text before it
    __device__ __forceinline__ uint32_t bwd(uint64_t o) const {
        const uint32_t c0 = code(o);
        if (c0 == CL_CONT) return 0u;
        const uint32_t k = c0 & 7u;
        return first(o) ? CL_CLEAR : k == K_R ? CL_SET : k == K_W ? 0u : CL_CLEAR;
    }
    // an "other" codepoint whose previous codepoint is at p starts a match: not inside a run of
    // them, and not glued to the single U+0020 the pattern lets such a run begin with
    __device__ __forceinline__ bool o_start_after(uint64_t p) const {
        const uint32_t pc = code(p);
        return (pc & 7u) == K_O ? false : (pc & 7u) == K_W ? (pc >> 3) != K_ID_SPACE : true;
    }
    __device__ __forceinline__ bool o_start(uint64_t o) const { return first(o) || o_start_after(prev(o)); }
    __device__ __forceinline__ bool apos_start(uint64_t o) const { return (code(o) >> 3) == K_ID_APOS && o_start(o); }
};

// block_seg_scan over cl_combine; REV: exclusive from the right (thread 255 first)
template <bool REV>
__device__ __forceinline__ uint32_t cl_block_scan(uint32_t v, uint32_t* sh, uint32_t* total) {
    constexpr int NW = PT_TPB / 64;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = REV ? __shfl_down(incl, o) : __shfl_up(incl, o);
        if (REV ? lane + o < 64 : lane >= o) incl = cl_combine(u, incl);
    }
    if (lane == (REV ? 0 : 63)) sh[wid] = incl;
    __syncthreads();
    uint32_t carry = 0;   // identity
    if (REV) {
        for (int w = NW - 1; w > wid; --w) carry = cl_combine(carry, sh[w]);
    } else {
        for (int w = 0; w < wid; ++w) carry = cl_combine(carry, sh[w]);
    }
    const uint32_t nb = REV ? __shfl_down(incl, 1) : __shfl_up(incl, 1);
    const uint32_t excl = cl_combine(carry, lane != (REV ? 63 : 0) ? nb : 0u);
    if (total) {
        uint32_t t = 0;
        for (int w = 0; w < NW; ++w) t = cl_combine(t, sh[REV ? NW - 1 - w : w]);
        *total = t;
    }
    __syncthreads();
    return excl;
}

#define CL_STAGE(HALO)                                                    \
    __shared__ uint32_t sh[PT_TPB / 64];                                  \
    __shared__ __attribute__((aligned(16))) uint8_t W[PT_WIN];            \
    __shared__ __attribute__((aligned(16))) uint8_t F[DOCS ? PT_WIN : 16]; \
    __shared__ __attribute__((aligned(16))) uint8_t C[PT_WIN];            \
    __shared__ uint8_t ac[128];                                           \
    const int64_t base = (int64_t)blockIdx.x * PT_BLK - PT_HALO;          \
    if (DOCS) pt_stage_flags(df, n, F, base);                             \
    pt_stage(in, n, idx, cls, W, ac, base);                               \
    cl_codes<DOCS, HALO>(W, F, ac, C, base, n, idx, cls);                 \
    const ClWin<DOCS> w{C, F, base, n};                                   \
    const uint64_t o0 = (uint64_t)blockIdx.x * PT_BLK + (uint64_t)threadIdx.x * PT_ITEMS;

// fagg[b], bagg[b]: block b's forward and backward aggregate
template <bool DOCS>
__global__ __launch_bounds__(PT_TPB) void k_ptc_scan1(const uint8_t* __restrict__ in, uint64_t n,
                                                      const uint8_t* __restrict__ df, const uint16_t* __restrict__ idx,
                                                      const uint8_t* __restrict__ cls, uint32_t* __restrict__ fagg,
                                                      uint32_t* __restrict__ bagg) {
    CL_STAGE(false)
    uint32_t a = 0, bk = 0;
    for (int k = 0; k < PT_ITEMS; ++k)
        if (o0 + k < n) a = cl_combine(a, w.fwd(o0 + k));
    for (int k = PT_ITEMS - 1; k >= 0; --k)
        if (o0 + k < n) bk = cl_combine(bk, w.bwd(o0 + k));
    uint32_t ft, bt;
    cl_block_scan<false>(a, sh, &ft);
    cl_block_scan<true>(bk, sh, &bt);
    if (threadIdx.x == 0) {
        fagg[blockIdx.x] = ft;
        bagg[blockIdx.x] = bt;
    }
}

// exclusive scan of a[0, nblk) in place, REV: from the right (k_pt_scan2's shape)
template <bool REV>
__device__ __forceinline__ void cl_scan_blocks(uint32_t* __restrict__ a, uint64_t nblk, uint32_t* sh) {
    const uint64_t per = (nblk + 1023) / 1024;
    const uint64_t lo = min(threadIdx.x * per, nblk), hi = min(lo + per, nblk);
    uint32_t v = 0;
    for (uint64_t i = lo; i < hi; ++i) v = cl_combine(v, a[REV ? nblk - 1 - i : i]);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(incl, o);
        if (lane >= o) incl = cl_combine(u, incl);
    }
    if (lane == 63) sh[wid] = incl;
    __syncthreads();
    uint32_t run = 0;
    for (int x = 0; x < wid; ++x) run = cl_combine(run, sh[x]);
    const uint32_t el = __shfl_up(incl, 1);
    run = cl_combine(run, lane ? el : 0u);
    for (uint64_t i = lo; i < hi; ++i) {
        const uint64_t j = REV ? nblk - 1 - i : i;
        const uint32_t x = a[j];
        a[j] = run;
        run = cl_combine(run, x);
    }
    __syncthreads();
}

__global__ __launch_bounds__(1024) void k_ptc_scan2(uint32_t* __restrict__ fagg, uint32_t* __restrict__ bagg, uint64_t nblk) {
    __shared__ uint32_t sh[16];
    cl_scan_blocks<false>(fagg, nblk, sh);
    cl_scan_blocks<true>(bagg, nblk, sh);
}

template <bool DOCS>
__global__ __launch_bounds__(PT_TPB) void k_ptc_mark(const uint8_t* __restrict__ in, uint64_t n,
                                                     const uint8_t* __restrict__ df, const uint16_t* __restrict__ idx,
                                                     const uint8_t* __restrict__ cls, const uint32_t* __restrict__ fagg,
                                                     const uint32_t* __restrict__ bagg, uint8_t* __restrict__ ws) {
    CL_STAGE(true)
    uint32_t a = 0, bk = 0;
    for (int k = 0; k < PT_ITEMS; ++k)
        if (o0 + k < n) a = cl_combine(a, w.fwd(o0 + k));
    for (int k = PT_ITEMS - 1; k >= 0; --k)
        if (o0 + k < n) bk = cl_combine(bk, w.bwd(o0 + k));
    uint32_t run = cl_combine(fagg[blockIdx.x], cl_block_scan<false>(a, sh, nullptr));
    uint32_t back = cl_combine(bagg[blockIdx.x], cl_block_scan<true>(bk, sh, nullptr));
    uint32_t later = 0;   // bit k: a CR / LF follows byte k's codepoint in its whitespace run
    for (int k = PT_ITEMS - 1; k >= 0; --k) {
        if (o0 + k >= n) continue;
        if ((back & 0x18u) == CL_SET) later |= 1u << k;
        back = cl_combine(back, w.bwd(o0 + k));
    }
    uint32_t wsv[PT_ITEMS / 4] = {0u, 0u, 0u, 0u};   // this thread's 16 word-start bytes, stored as one vector
    for (int k = 0; k < PT_ITEMS; ++k) {
        const uint64_t o = o0 + k;
        if (o >= n) break;
        const uint32_t c0 = w.code(o);
        uint32_t start = 0;
        if (c0 != CL_CONT) {
            const uint32_t cc = c0 & 7u;
            if (w.first(o)) {
                start = 1;
            } else {
                const uint64_t p1 = w.prev(o);
                const uint32_t c1 = w.code(p1), pc = c1 & 7u;
                const bool pws = pc == K_W || pc == K_R;
                const bool e_prev = (run & 0x18u) == CL_SET;   // the codepoint before is O or an eaten newline
                if (cc == K_W || cc == K_R) {
                    if (cc == K_R && e_prev) start = 0;                        // eaten
                    else if (!pws || (pc == K_R && e_prev)) start = 1;         // after a non-blank or an eaten newline
                    else if (cc == K_R || ((later >> k) & 1u)) start = 0;      // inside \s*[\r\n]
                    else if (pc == K_R) start = 1;
                    else {
                        const uint32_t nk = w.next_code(o);                    // the last blank before a non-blank
                        start = nk != CL_CONT && (nk & 7u) != K_W && (nk & 7u) != K_R;
                    }
                } else if (cc == K_N) {
                    start = (run & 3u) == 0u;
                } else if (cc == K_O) {
                    start = w.o_start_after(p1);
                } else if (pc == K_O) {
                    start = !w.o_start(p1);        // a starting O takes the letters: as a contraction or as the prefix
                } else if (pc == K_N || pc == K_R) {
                    start = 1;
                } else if (pc == K_L && (c1 >> 3) != 0u && !w.first(p1)) {
                    // the letter before is one a contraction can end with: 's|x, 'll|x
                    const uint64_t p2 = w.prev(p1);
                    const uint32_t c2 = w.code(p2);
                    if (w.apos_start(p2)) start = cl_sdmt(c1 >> 3);
                    else if (cl_pair(c2 >> 3, c1 >> 3) && !w.first(p2)) start = w.apos_start(w.prev(p2));
                }
            }
        }
#pragma unroll
        for (int q = 0; q < PT_ITEMS / 4; ++q)
            if (k / 4 == q) wsv[q] |= start << (8 * (k & 3));
        run = cl_combine(run, w.fwd(o));
    }
    if (o0 >= n) return;
    if (o0 + PT_ITEMS <= n && ((uintptr_t)(ws + o0) & 15u) == 0u) {
        *reinterpret_cast<uint4*>(ws + o0) = make_uint4(wsv[0], wsv[1], wsv[2], wsv[3]);
    } else {
        for (int k = 0; k < PT_ITEMS && o0 + k < n; ++k) ws[o0 + k] = (uint8_t)(wsv[k / 4] >> (8 * (k & 3)));
    }
}
#undef CL_STAGE

