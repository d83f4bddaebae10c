// o200k_base word-start kernels.  Included by pretok.hip inside its unnamed namespace, after
// pretok_cl100k.h, whose staging, window (ClWin), ids (cl_id) and code layout these use.
#pragma once

// ── o200k_base word starts (gbpe_pretokenize_o200k*) ─────────────
//
// The split pattern of o200k_base over the eight classes of unicode_classes_o200k.h, as one
// forward automaton of 11 states (which match is running and in which phase) plus two
// backward "last one wins" states:
//   forward   END UP LO PFX C2 C1 D1 D2 P1 P2 WS; a codepoint's element is the map state → state
//             of its kind (class + what one or two codepoints ahead decide), 11 nibbles in a
//             64-bit word; the scan operator is composition of maps
//   later     CR/LF sets, other whitespace keeps, the rest clears (§3g's)              (backward)
//   upper     upper-only keeps, other letters and marks clear, the rest and the end of the
//             text set: every codepoint from here to the end of the letter run is upper-only (backward)
//   k_pto_scan1   per 4096-byte block: the composed map and the backward aggregate
//   k_pto_scan2   one workgroup: the maps scanned left to right, the backward words right to left
//   k_pto_mark    per byte: state before the codepoint + its kind → word-start byte
// No transition depends on a backward state: only two start decisions do (an upper-only
// codepoint after a both-sided one in a word still in its upper phase, and a blank inside a
// whitespace run), so the two scans run side by side as §3g's do.
// <DOCS>: as k_ptc_*<true>: a flagged byte is byte 0 of its text; its element is the constant
// map (the state after it, whatever came before) and the backward states restart there.
// Codes per byte in LDS: bits 0-2 the class, bits 3-6 K_ID_* (and K_ID_SLASH), CL_CONT on a
// continuation byte and past the end.
enum : uint32_t { O2_U = 0, O2_L, O2_B, O2_M, O2_N, O2_W, O2_R, O2_O };
constexpr uint32_t K_ID_SLASH = K_ID_SPACE + 1;
enum : uint32_t { S_END = 0, S_UP, S_LO, S_PFX, S_C2, S_C1, S_D1, S_D2, S_P1, S_P2, S_WS, O2_STATES };
// kinds: the class, and for blanks and "other" what follows.  KW: a blank before a blank or the
// end; KWL: the run's last blank, before something it is no prefix of; KWP: a blank that is the
// prefix of letters or the U+0020 of " ?[^\s\p{L}\p{N}]+".  KO / KS (`/`): nothing it could
// be a prefix of follows; KOP / KSP: a letter or mark follows; KA1 / KA2: U+0027 before a
// contraction suffix of one / two letters.
enum : uint32_t { KU = 0, KL, KB, KM, KN, KR, KW, KWL, KWP, KO, KOP, KS, KSP, KA1, KA2, O2_KINDS };

// the state after a codepoint of kind kd that starts a match
constexpr uint32_t o2_fresh(uint32_t kd) {
    switch (kd) {
        case KU: case KB: case KM: return S_UP;    // a mark at a match start: alone as prefix or as letter, the match is the same
        case KL: return S_LO;
        case KN: return S_D1;
        case KO: case KS: return S_P1;
        case KOP: case KSP: case KA1: case KA2: case KWP: return S_PFX;
        default: return S_WS;
    }
}
constexpr bool o2_is_other(uint32_t kd) { return kd >= KO; }
constexpr bool o2_is_slash(uint32_t kd) { return kd == KS || kd == KSP; }
// cont: the codepoint goes on with the running match (no start); the two decisions that also
// need a backward state (UP + KU, WS + KW) are "start" here and settled in k_pto_mark
constexpr uint32_t o2_delta(uint32_t s, uint32_t kd, bool* cont) {
    *cont = true;
    if (s == S_C2) return S_C1;
    if (s == S_C1) return S_END;
    if (s == S_PFX) return kd == KL ? S_LO : o2_is_other(kd) ? S_P1 : o2_fresh(kd);
    if ((s == S_UP || s == S_LO) && (kd == KA1 || kd == KA2)) return kd == KA1 ? S_C1 : S_C2;
    if (s == S_UP && (kd == KB || kd == KM)) return S_UP;
    if (s == S_UP && kd == KL) return S_LO;
    if (s == S_LO && (kd == KL || kd == KB || kd == KM)) return S_LO;
    if (s == S_D1 && kd == KN) return S_D2;
    if (s == S_D2 && kd == KN) return S_END;
    if (s == S_P1 && (o2_is_other(kd) || kd == KM)) return S_P1;
    if ((s == S_P1 || s == S_P2) && kd == KR) return S_P2;
    if (s == S_P2 && o2_is_slash(kd)) return S_P2;
    if (s == S_WS && kd == KR) return S_WS;
    *cont = false;
    return o2_fresh(kd);
}
// bits 0-43: the map, a nibble per state; bits 48-58: cont per state
constexpr uint64_t o2_table(uint32_t kd) {
    uint64_t t = 0;
    for (uint32_t s = 0; s < O2_STATES; ++s) {
        bool cont = false;
        t |= (uint64_t)o2_delta(s, kd, &cont) << (4 * s);
        if (cont) t |= 1ull << (48 + s);
    }
    return t;
}
__device__ const uint64_t kO2Table[16] = {
    o2_table(KU), o2_table(KL), o2_table(KB), o2_table(KM), o2_table(KN), o2_table(KR), o2_table(KW), o2_table(KWL),
    o2_table(KWP), o2_table(KO), o2_table(KOP), o2_table(KS), o2_table(KSP), o2_table(KA1), o2_table(KA2), 0ull};
constexpr uint64_t O2_MAP = (1ull << (4 * O2_STATES)) - 1;
constexpr uint64_t O2_IDENT = 0xA9876543210ull;

// a then b
struct O2Fwd {
    typedef uint64_t T;
    static constexpr T ident = O2_IDENT;
    __device__ __forceinline__ static T combine(T a, T b) {
        if (b == O2_IDENT) return a;
        T r = 0;
#pragma unroll
        for (uint32_t s = 0; s < O2_STATES; ++s) r |= ((b >> (4u * ((uint32_t)(a >> (4 * s)) & 15u))) & 15ull) << (4 * s);
        return r;
    }
};
// bits 3-4 `later`, bits 5-6 `upper`, each 0 keep / 1 set / 2 clear: the second argument's wins
constexpr uint32_t O2_USET = 1u << 5, O2_UCLEAR = 2u << 5;
struct O2Bwd {
    typedef uint32_t T;
    static constexpr T ident = 0u;
    __device__ __forceinline__ static T combine(T a, T b) {
        return ((b & 0x18u) ? (b & 0x18u) : (a & 0x18u)) | ((b & 0x60u) ? (b & 0x60u) : (a & 0x60u));
    }
};

__device__ __forceinline__ uint32_t o2_id(uint32_t cp) { return cp == 0x2Fu ? K_ID_SLASH : cl_id(cp); }

// cl_code over the o200k table and ids
template <bool DOCS>
__device__ __forceinline__ uint32_t o2_code(const uint8_t* W, const uint8_t* F, const uint8_t* ac, int i,
                                            const uint16_t* __restrict__ idx, const uint8_t* __restrict__ cls) {
    const uint32_t b = W[i];
    if (!is_lead(b)) return CL_CONT;
    if (b < 0x80u) return ac[b] | (o2_id(b) << 3);
    const int sz = (b & 0xE0u) == 0xC0u ? 2 : (b & 0xF0u) == 0xE0u ? 3 : 4;
    uint32_t cp = sz == 2 ? (b & 0x1Fu) : sz == 3 ? (b & 0x0Fu) : (b & 0x07u);
    bool open = true;
    for (int j = 1; j < sz; ++j) {
        open = open && i + j < PT_WIN && !(DOCS && F[i + j]);
        cp = (cp << 6) | (open ? (W[i + j] & 0x3Fu) : 0u);
    }
    const uint32_t k = cp >= 0x110000u ? (uint32_t)O2_O
                                       : cls[((uint32_t)idx[cp >> kO200kBlockShift] << kO200kBlockShift) | (cp & 0xFFu)];
    return k | (o2_id(cp) << 3);
}

// the codes of the window (block and halo: every kind looks ahead); ends with a barrier
template <bool DOCS>
__device__ __forceinline__ void o2_codes(const uint8_t* W, const uint8_t* F, const uint8_t* ac, uint8_t* C, int64_t base,
                                         uint64_t n, const uint16_t* __restrict__ idx, const uint8_t* __restrict__ cls) {
    for (int i = threadIdx.x; i < PT_WIN; i += PT_TPB) {
        const int64_t g = base + i;
        C[i] = g >= 0 && (uint64_t)g < n ? (uint8_t)o2_code<DOCS>(W, F, ac, i, idx, cls) : (uint8_t)CL_CONT;
    }
    __syncthreads();
}

template <bool DOCS>
struct O2Win : ClWin<DOCS> {
    const uint64_t* tab;   // LDS: kO2Table
    using ClWin<DOCS>::code;
    using ClWin<DOCS>::first;
    using ClWin<DOCS>::n;
    // the lead byte of the codepoint after the one at o, ~0 where the text ends first
    __device__ __forceinline__ uint64_t nextp(uint64_t o) const {
        uint64_t q = o + 1;
        while (q < o + 4 && q < n && !first(q) && code(q) == CL_CONT) ++q;
        return q < n && !first(q) && code(q) != CL_CONT ? q : ~0ull;
    }
    // the kind of the codepoint at o (a lead byte)
    __device__ __forceinline__ uint32_t kind(uint64_t o) const {
        const uint32_t c0 = code(o), k = c0 & 7u, id = c0 >> 3;
        if (k < O2_W) return k;               // KU KL KB KM KN are the classes' numbers
        if (k == O2_R) return KR;
        const uint64_t q = nextp(o);
        const uint32_t nc = q != ~0ull ? code(q) : (uint32_t)CL_CONT;
        const bool some = nc != CL_CONT, letter = some && (nc & 7u) <= O2_M;
        if (k == O2_W) {
            if (letter || (id == K_ID_SPACE && some && (nc & 7u) == O2_O)) return KWP;
            return some && (nc & 7u) != O2_W && (nc & 7u) != O2_R ? KWL : KW;
        }
        if (id == K_ID_APOS && letter && (nc >> 3) != 0u) {
            if (cl_sdmt(nc >> 3)) return KA1;
            const uint64_t q2 = nextp(q);
            if (q2 != ~0ull && cl_pair(nc >> 3, code(q2) >> 3)) return KA2;
        }
        return id == K_ID_SLASH ? (letter ? KSP : KS) : (letter ? KOP : KO);
    }
    // forward element of byte o; a text's first codepoint: the state after it, whatever came before
    __device__ __forceinline__ uint64_t fwd(uint64_t o) const {
        if (code(o) == CL_CONT) return O2_IDENT;
        const uint64_t t = tab[kind(o)] & O2_MAP;
        return first(o) ? (t & 15ull) * 0x11111111111ull : t;
    }
    // backward element of byte o; nothing after a text's first byte reaches the text before it
    __device__ __forceinline__ uint32_t bwd(uint64_t o) const {
        const uint32_t c0 = code(o);
        if (c0 == CL_CONT) return 0u;
        if (first(o)) return CL_CLEAR | O2_USET;
        const uint32_t k = c0 & 7u;
        return (k == O2_R ? CL_SET : k == O2_W ? 0u : CL_CLEAR) | (k == O2_U ? 0u : k <= O2_M ? O2_UCLEAR : O2_USET);
    }
};

// block-wide exclusive scan over Op (one element per thread); REV: from the right (thread 255 first)
template <class Op, bool REV>
__device__ __forceinline__ typename Op::T o2_block_scan(typename Op::T v, typename Op::T* sh, typename Op::T* total) {
    typedef typename Op::T T;
    constexpr int NW = PT_TPB / 64;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    T incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const T u = REV ? __shfl_down(incl, o) : __shfl_up(incl, o);
        if (REV ? lane + o < 64 : lane >= o) incl = Op::combine(u, incl);
    }
    if (lane == (REV ? 0 : 63)) sh[wid] = incl;
    __syncthreads();
    T carry = Op::ident;
    if (REV) {
        for (int w = NW - 1; w > wid; --w) carry = Op::combine(carry, sh[w]);
    } else {
        for (int w = 0; w < wid; ++w) carry = Op::combine(carry, sh[w]);
    }
    const T nb = REV ? __shfl_down(incl, 1) : __shfl_up(incl, 1);
    const T excl = Op::combine(carry, lane != (REV ? 63 : 0) ? nb : Op::ident);
    if (total) {
        T t = Op::ident;
        for (int w = 0; w < NW; ++w) t = Op::combine(t, sh[REV ? NW - 1 - w : w]);
        *total = t;
    }
    __syncthreads();
    return excl;
}

#define O2_STAGE                                                          \
    __shared__ uint64_t shf[PT_TPB / 64];                                 \
    __shared__ uint32_t shb[PT_TPB / 64];                                 \
    __shared__ uint64_t T[16];                                            \
    __shared__ __attribute__((aligned(16))) uint8_t W[PT_WIN];            \
    __shared__ __attribute__((aligned(16))) uint8_t F[DOCS ? PT_WIN : 16]; \
    __shared__ __attribute__((aligned(16))) uint8_t C[PT_WIN];            \
    __shared__ uint8_t ac[128];                                           \
    const int64_t base = (int64_t)blockIdx.x * PT_BLK - PT_HALO;          \
    if (threadIdx.x < 16) T[threadIdx.x] = kO2Table[threadIdx.x];         \
    if (DOCS) pt_stage_flags(df, n, F, base);                             \
    pt_stage(in, n, idx, cls, W, ac, base);                               \
    o2_codes<DOCS>(W, F, ac, C, base, n, idx, cls);                       \
    const O2Win<DOCS> w{{C, F, base, n}, T};                              \
    const uint64_t o0 = (uint64_t)blockIdx.x * PT_BLK + (uint64_t)threadIdx.x * PT_ITEMS;

// this thread's 16 bytes: the composed map and the backward aggregate
#define O2_THREAD_AGG                                                     \
    uint64_t a = O2_IDENT;                                                \
    uint32_t bk = 0;                                                      \
    for (int k = 0; k < PT_ITEMS; ++k)                                    \
        if (o0 + k < n) a = O2Fwd::combine(a, w.fwd(o0 + k));             \
    for (int k = PT_ITEMS - 1; k >= 0; --k)                               \
        if (o0 + k < n) bk = O2Bwd::combine(bk, w.bwd(o0 + k));

// fagg[b], bagg[b]: block b's composed map and backward aggregate
template <bool DOCS>
__global__ __launch_bounds__(PT_TPB) void k_pto_scan1(const uint8_t* __restrict__ in, uint64_t n,
                                                      const uint8_t* __restrict__ df, const uint16_t* __restrict__ idx,
                                                      const uint8_t* __restrict__ cls, uint64_t* __restrict__ fagg,
                                                      uint32_t* __restrict__ bagg) {
    O2_STAGE
    O2_THREAD_AGG
    uint64_t ft;
    uint32_t bt;
    o2_block_scan<O2Fwd, false>(a, shf, &ft);
    o2_block_scan<O2Bwd, true>(bk, shb, &bt);
    if (threadIdx.x == 0) {
        fagg[blockIdx.x] = ft;
        bagg[blockIdx.x] = bt;
    }
}

// exclusive scan of a[0, nblk) in place, REV: from the right (cl_scan_blocks' shape)
template <class Op, bool REV>
__device__ __forceinline__ void o2_scan_blocks(typename Op::T* __restrict__ a, uint64_t nblk, typename Op::T* sh) {
    typedef typename Op::T T;
    const uint64_t per = (nblk + 1023) / 1024;
    const uint64_t lo = min(threadIdx.x * per, nblk), hi = min(lo + per, nblk);
    T v = Op::ident;
    for (uint64_t i = lo; i < hi; ++i) v = Op::combine(v, a[REV ? nblk - 1 - i : i]);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    T incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(incl, o);
        if (lane >= o) incl = Op::combine(u, incl);
    }
    if (lane == 63) sh[wid] = incl;
    __syncthreads();
    T run = Op::ident;
    for (int x = 0; x < wid; ++x) run = Op::combine(run, sh[x]);
    const T el = __shfl_up(incl, 1);
    run = Op::combine(run, lane ? el : Op::ident);
    for (uint64_t i = lo; i < hi; ++i) {
        const uint64_t j = REV ? nblk - 1 - i : i;
        const T x = a[j];
        a[j] = run;
        run = Op::combine(run, x);
    }
    __syncthreads();
}

__global__ __launch_bounds__(1024) void k_pto_scan2(uint64_t* __restrict__ fagg, uint32_t* __restrict__ bagg, uint64_t nblk) {
    __shared__ uint64_t shf[16];
    __shared__ uint32_t shb[16];
    o2_scan_blocks<O2Fwd, false>(fagg, nblk, shf);
    o2_scan_blocks<O2Bwd, true>(bagg, nblk, shb);
}

template <bool DOCS>
__global__ __launch_bounds__(PT_TPB) void k_pto_mark(const uint8_t* __restrict__ in, uint64_t n,
                                                     const uint8_t* __restrict__ df, const uint16_t* __restrict__ idx,
                                                     const uint8_t* __restrict__ cls, const uint64_t* __restrict__ fagg,
                                                     const uint32_t* __restrict__ bagg, uint8_t* __restrict__ ws) {
    O2_STAGE
    O2_THREAD_AGG
    // the state before this thread's first byte: the text begins in END
    uint32_t s = (uint32_t)O2Fwd::combine(fagg[blockIdx.x], o2_block_scan<O2Fwd, false>(a, shf, nullptr)) & 15u;
    uint32_t back = O2Bwd::combine(bagg[blockIdx.x], o2_block_scan<O2Bwd, true>(bk, shb, nullptr));
    uint32_t later = 0, upper = 0;   // bit k: `later` / `upper` of what follows byte k's codepoint
    for (int k = PT_ITEMS - 1; k >= 0; --k) {
        if (o0 + k >= n) continue;
        if ((back & 0x18u) == CL_SET) later |= 1u << k;
        if ((back & 0x60u) != O2_UCLEAR) upper |= 1u << k;     // (kept to the end of the text: set)
        back = O2Bwd::combine(back, w.bwd(o0 + k));
    }
    uint32_t wsv[PT_ITEMS / 4] = {0u, 0u, 0u, 0u};   // this thread's 16 word-start bytes, stored as one vector
    for (int k = 0; k < PT_ITEMS; ++k) {
        const uint64_t o = o0 + k;
        if (o >= n) break;
        uint32_t start = 0;
        if (w.code(o) != CL_CONT) {
            const uint32_t kd = w.kind(o);
            const uint64_t t = T[kd];
            if (w.first(o)) {
                start = 1;
                s = (uint32_t)t & 15u;
            } else {
                start = ((uint32_t)(t >> (48 + s)) & 1u) ^ 1u;
                if ((s == S_UP && kd == KU) || (s == S_WS && kd == KW)) {
                    const uint32_t pc = w.code(w.prev(o)) & 7u;
                    // AX|B: every letter from here on is upper-only, so [..Ll..]+ can end on X alone;
                    // a blank after \s*[\r\n]+ has ended, with no newline left in the run
                    start = kd == KU ? (pc == O2_B || pc == O2_M) && ((upper >> k) & 1u)
                                     : pc == O2_R && !((later >> k) & 1u);
                }
                s = (uint32_t)(t >> (4 * s)) & 15u;
            }
        }
#pragma unroll
        for (int q = 0; q < PT_ITEMS / 4; ++q)
            if (k / 4 == q) wsv[q] |= start << (8 * (k & 3));
    }
    if (o0 >= n) return;
    if (o0 + PT_ITEMS <= n && ((uintptr_t)(ws + o0) & 15u) == 0u) {
        *reinterpret_cast<uint4*>(ws + o0) = make_uint4(wsv[0], wsv[1], wsv[2], wsv[3]);
    } else {
        for (int k = 0; k < PT_ITEMS && o0 + k < n; ++k) ws[o0 + k] = (uint8_t)(wsv[k / 4] >> (8 * (k & 3)));
    }
}
#undef O2_STAGE
#undef O2_THREAD_AGG

