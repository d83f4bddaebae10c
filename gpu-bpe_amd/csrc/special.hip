// Special tokens of the merge-rank encoder, matched on the device.
//
// A table of 1 to 254 byte strings (<|endoftext|> and its like); the accepted matches are
// those of the sequential scan: left to right, the longest special at a position, resume
// just past it.  Two kernels give the same set in parallel:
//   k_sp_cand    cand[i] = 1 + index of the longest special that matches at byte i (0: none),
//                whatever lies before i.  256 threads x 16 bytes, the window and a look-ahead
//                halo of 127 bytes in LDS; a 256-bit filter of first bytes rejects nearly every
//                position after one test; the table is ordered by first byte, then length
//                descending, so the first hit at a position is the longest.  In a batch call a
//                match that holds a document start past its first byte is not one.
//   k_sp_accept  every accepted match is a candidate with the candidate's length (the scan
//                takes the longest at the position it stands on).  A candidate that no earlier
//                candidate's span covers is an ANCHOR: no accepted match can cover it, so the
//                scan reaches it and accepts it.  The anchor's lane walks the chain from there:
//                accept, jump to the span's end p, take the first candidate at or after p (the
//                scan has nothing to accept before it), stop when that one is an anchor — its
//                own lane carries on.  A span is at most 128 bytes, so a candidate at or past
//                p + 127 is covered by nothing that starts before p: the look-ahead from p and
//                the look-back of the anchor test are both 127 bytes.  The chains are disjoint
//                and together are the sequential scan: each mark byte has one writer.  A chain
//                is serial and as long as the input makes it ("aa" in "aaaa…").
// mark[i] is 0 on an ordinary byte, 1 + index (the caller's order) on an accepted special's
// first byte and 255 on its other bytes.

#include "common.h"

#include <algorithm>
#include <numeric>

namespace {

constexpr int SP_TPB = 256;
constexpr int SP_ITEMS = 16;
constexpr int SP_BLK = SP_TPB * SP_ITEMS;                // bytes per block
constexpr int SP_HALO = GBPE_SPECIAL_MAX_BYTES - 1;      // look-ahead (cand) and look-back (anchor test)
constexpr int SP_WIN = SP_BLK + 128;                     // LDS window: block + halo, rounded up to 16

struct SpTable {
    const uint8_t* bytes;     // the strings end to end, in match order
    const uint32_t* ent;      // per string in match order: offset | (length - 1) << 16 | caller's index << 24
    const uint16_t* first;    // [257]: the entries whose first byte is b are ent[first[b], first[b + 1])
    const uint32_t* filter;   // [8]: bit b set iff some string begins with byte b
    const uint8_t* len1;      // [256]: length of the string with mark value v = 1 + caller's index (0: none)
};

__global__ __launch_bounds__(SP_TPB) void k_sp_cand(const uint8_t* __restrict__ in, uint64_t n,
                                                    const uint8_t* __restrict__ docf, SpTable t,
                                                    uint8_t* __restrict__ cand) {
    __shared__ __attribute__((aligned(16))) uint8_t W[SP_WIN];
    __shared__ uint32_t flt[8];
    const uint64_t base = (uint64_t)blockIdx.x * SP_BLK;
    for (int i = threadIdx.x; i < SP_WIN / 4; i += SP_TPB) {
        const uint64_t g = base + 4 * (uint64_t)i;
        uint32_t v = 0;
        if (g + 4 <= n && ((uintptr_t)(in + g) & 3u) == 0u) {
            v = *reinterpret_cast<const uint32_t*>(in + g);
        } else {
            for (int k = 0; k < 4; ++k)
                if (g + k < n) v |= (uint32_t)in[g + k] << (8 * k);
        }
        reinterpret_cast<uint32_t*>(W)[i] = v;
    }
    if (threadIdx.x < 8) flt[threadIdx.x] = t.filter[threadIdx.x];
    __syncthreads();
    const int l0 = threadIdx.x * SP_ITEMS;
    const uint64_t o0 = base + l0;
    if (o0 >= n) return;
    uint32_t cv[SP_ITEMS / 4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < SP_ITEMS; ++k) {
        const uint64_t o = o0 + k;
        if (o >= n) break;
        const uint32_t b = W[l0 + k];
        if (((flt[b >> 5] >> (b & 31u)) & 1u) == 0u) continue;
        uint32_t hit = 0;
        for (uint32_t e = t.first[b], e1 = t.first[b + 1]; e < e1 && !hit; ++e) {
            const uint32_t ent = t.ent[e];
            const uint32_t len = ((ent >> 16) & 0x7Fu) + 1u;
            if (o + len > n) continue;
            const uint8_t* s = t.bytes + (ent & 0xFFFFu);
            uint32_t j = 1;
            while (j < len && W[l0 + k + j] == s[j]) ++j;   // (l0 + k + j <= SP_BLK - 1 + 127 < SP_WIN)
            if (j < len) continue;
            if (docf) {   // a special lies wholly inside one document
                for (j = 1; j < len && !docf[o + j]; ++j) {}
                if (j < len) continue;
            }
            hit = (ent >> 24) + 1u;
        }
#pragma unroll
        for (int q = 0; q < SP_ITEMS / 4; ++q)
            if (k / 4 == q) cv[q] |= hit << (8 * (k & 3));
    }
    if (o0 + SP_ITEMS <= n) {   // (cand is a pooled block: 16-byte aligned)
        *reinterpret_cast<uint4*>(cand + o0) = make_uint4(cv[0], cv[1], cv[2], cv[3]);
    } else {
        for (int k = 0; k < SP_ITEMS && o0 + k < n; ++k) cand[o0 + k] = (uint8_t)(cv[k / 4] >> (8 * (k & 3)));
    }
}

// no candidate before i reaches over byte i
__device__ __forceinline__ bool sp_anchor(const uint8_t* __restrict__ cand, const uint8_t* __restrict__ len1, uint64_t i) {
    const uint64_t j0 = i > (uint64_t)SP_HALO ? i - SP_HALO : 0;
    for (uint64_t j = j0; j < i; ++j) {
        const uint32_t c = cand[j];
        if (c && j + len1[c] > i) return false;
    }
    return true;
}

// mark (zeroed by the caller) from the candidates; with `flags`, also the pre-tokeniser's
// piece starts: byte 0, each accepted special's first byte and the byte after its last
__global__ __launch_bounds__(SP_TPB) void k_sp_accept(const uint8_t* __restrict__ cand, uint64_t n,
                                                      const uint8_t* __restrict__ len1, uint8_t* __restrict__ mark,
                                                      uint8_t* __restrict__ flags) {
    const uint64_t o0 = ((uint64_t)blockIdx.x * SP_TPB + threadIdx.x) * SP_ITEMS;
    if (o0 >= n) return;
    if (o0 == 0 && flags) flags[0] = 1;
    uint32_t cv[SP_ITEMS / 4] = {0u, 0u, 0u, 0u};
    if (o0 + SP_ITEMS <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(cand + o0);
        cv[0] = v.x, cv[1] = v.y, cv[2] = v.z, cv[3] = v.w;
    } else {
        for (int k = 0; k < SP_ITEMS && o0 + k < n; ++k) cv[k / 4] |= (uint32_t)cand[o0 + k] << (8 * (k & 3));
    }
    if ((cv[0] | cv[1] | cv[2] | cv[3]) == 0u) return;
    for (int k = 0; k < SP_ITEMS; ++k) {
        uint32_t c = 0;
#pragma unroll
        for (int q = 0; q < SP_ITEMS / 4; ++q)
            if (k / 4 == q) c = (cv[q] >> (8 * (k & 3))) & 0xFFu;
        if (!c) continue;
        uint64_t i = o0 + k;
        if (!sp_anchor(cand, len1, i)) continue;
        for (;;) {   // the chain of this anchor
            const uint64_t p = i + len1[c];   // (<= n: k_sp_cand keeps a match inside the input)
            mark[i] = (uint8_t)c;
            for (uint64_t j = i + 1; j < p; ++j) mark[j] = 255;
            if (flags) {
                flags[i] = 1;
                if (p < n) flags[p] = 1;
            }
            uint64_t q = p;
            const uint64_t q1 = p + SP_HALO < n ? p + SP_HALO : n;
            while (q < q1 && !cand[q]) ++q;
            if (q >= q1 || sp_anchor(cand, len1, q)) break;   // (none this near: the next one is an anchor)
            i = q;
            c = cand[q];
        }
    }
}

}  // namespace

struct gbpe_specials {
    gbpe_ctx* ctx = nullptr;
    uint32_t n = 0;
    uint8_t* dev = nullptr;   // one allocation: ids, ent, first, filter, len1, bytes
    SpTable t{};
    const uint32_t* ids = nullptr;   // [n], the caller's order
};

extern "C" int gbpe_specials_upload(gbpe_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, const uint32_t* ids,
                                    uint32_t n_specials, gbpe_specials** out) {
    if (!ctx || !out) return gbpe_set_error(ctx, GBPE_E_INVALID, "specials upload: null argument");
    *out = nullptr;
    if (!bytes || !offsets || !ids) return gbpe_set_error(ctx, GBPE_E_INVALID, "specials upload: null argument");
    if (n_specials == 0 || n_specials > GBPE_SPECIALS_MAX)
        return gbpe_set_error(ctx, GBPE_E_INVALID, "specials upload: %u entries (1 to %u)", n_specials, GBPE_SPECIALS_MAX);
    for (uint32_t i = 0; i < n_specials; ++i) {
        if (offsets[i + 1] <= offsets[i] || offsets[i + 1] - offsets[i] > GBPE_SPECIAL_MAX_BYTES)
            return gbpe_set_error(ctx, GBPE_E_INVALID, "specials upload: entry %u is empty or above %u bytes", i,
                                  GBPE_SPECIAL_MAX_BYTES);
    }
    auto str = [&](uint32_t i) { return std::string((const char*)bytes + offsets[i], offsets[i + 1] - offsets[i]); };
    // match order: by first byte, then the longest first
    std::vector<uint32_t> ord(n_specials);
    std::iota(ord.begin(), ord.end(), 0u);
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) {
        const std::string sa = str(a), sb = str(b);
        if (sa[0] != sb[0]) return (uint8_t)sa[0] < (uint8_t)sb[0];
        if (sa.size() != sb.size()) return sa.size() > sb.size();
        return sa < sb;
    });
    for (uint32_t k = 0; k + 1 < n_specials; ++k)
        if (str(ord[k]) == str(ord[k + 1]))
            return gbpe_set_error(ctx, GBPE_E_INVALID, "specials upload: entries %u and %u are the same string",
                                  std::min(ord[k], ord[k + 1]), std::max(ord[k], ord[k + 1]));
    std::vector<uint32_t> ent(n_specials), filter(8, 0u);
    std::vector<uint16_t> first(257, 0);
    std::vector<uint8_t> len1(256, 0), packed;
    for (uint32_t k = 0; k < n_specials; ++k) {
        const std::string s = str(ord[k]);
        const uint8_t b = (uint8_t)s[0];
        ent[k] = (uint32_t)packed.size() | ((uint32_t)(s.size() - 1) << 16) | (ord[k] << 24);
        packed.insert(packed.end(), s.begin(), s.end());
        filter[b >> 5] |= 1u << (b & 31u);
        ++first[b + 1];
        len1[ord[k] + 1] = (uint8_t)s.size();
    }
    for (int b = 0; b < 256; ++b) first[b + 1] = (uint16_t)(first[b + 1] + first[b]);
    // one block: u32 ids, u32 ent, u32 filter, u16 first, u8 len1, u8 bytes
    const uint64_t o_ent = 4ull * n_specials, o_flt = o_ent + 4ull * n_specials, o_first = o_flt + 32;
    const uint64_t o_len = o_first + 2 * 257 + 2, o_bytes = o_len + 256, total = o_bytes + packed.size();
    std::vector<uint8_t> host(total, 0);
    memcpy(host.data(), ids, 4ull * n_specials);
    memcpy(host.data() + o_ent, ent.data(), 4ull * n_specials);
    memcpy(host.data() + o_flt, filter.data(), 32);
    memcpy(host.data() + o_first, first.data(), 2 * 257);
    memcpy(host.data() + o_len, len1.data(), 256);
    memcpy(host.data() + o_bytes, packed.data(), packed.size());
    auto* sp = new (std::nothrow) gbpe_specials();
    if (!sp) return gbpe_set_error(ctx, GBPE_E_OOM, "host allocation failed");
    hipError_t e = dev_malloc(ctx, &sp->dev, total);
    if (e == hipSuccess) e = hipMemcpy(sp->dev, host.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(sp->dev);
        delete sp;
        return gbpe_set_error(ctx, e == hipErrorOutOfMemory ? GBPE_E_OOM : GBPE_E_DEVICE, "specials upload failed: %s",
                              hipGetErrorString(e));
    }
    sp->ctx = ctx;
    sp->n = n_specials;
    sp->ids = (const uint32_t*)sp->dev;
    sp->t = SpTable{sp->dev + o_bytes, (const uint32_t*)(sp->dev + o_ent), (const uint16_t*)(sp->dev + o_first),
                    (const uint32_t*)(sp->dev + o_flt), sp->dev + o_len};
    *out = sp;
    return GBPE_OK;
}

extern "C" void gbpe_specials_free(gbpe_specials* sp) {
    if (!sp) return;
    hipFree(sp->dev);
    delete sp;
}

const uint32_t* gbpe_specials_ids(const gbpe_specials* sp) { return sp->ids; }

int gbpe_specials_launch(gbpe_ctx* ctx, const gbpe_specials* sp, const uint8_t* d_bytes, uint64_t n,
                         const uint8_t* d_doc_flags, uint8_t* d_cand, uint8_t* d_mark, uint8_t* d_flags) {
    hipStream_t s = ctx->stream;
    const dim3 grid((uint32_t)gbpe_div_up(n, SP_BLK));
    GBPE_HIP(ctx, hipMemsetAsync(d_mark, 0, n, s));
    hipLaunchKernelGGL(k_sp_cand, grid, dim3(SP_TPB), 0, s, d_bytes, n, d_doc_flags, sp->t, d_cand);
    hipLaunchKernelGGL(k_sp_accept, grid, dim3(SP_TPB), 0, s, (const uint8_t*)d_cand, n, sp->t.len1, d_mark, d_flags);
    GBPE_LAUNCH_CHECK(ctx);
    return GBPE_OK;
}

// ── the matcher alone (gbpe_specials_mark*) ────────────────────────────────

namespace {

inline uint64_t sp_up16(uint64_t x) { return (x + 15) & ~15ull; }
inline uint64_t sp_work_bytes(uint64_t n) { return 2 * sp_up16(n) + 16; }

// d_work: candidates, document flags, the bad-offsets word.  With documents the offsets are
// checked by the first kernel and read back before anything is written to d_mark.
int sp_mark_run(gbpe_ctx* ctx, const gbpe_specials* sp, const uint8_t* d_bytes, uint64_t n, const uint64_t* d_doc_off,
                uint64_t n_docs, uint8_t* d_work, uint8_t* d_mark) {
    hipStream_t s = ctx->stream;
    uint8_t* d_cand = d_work;
    uint8_t* d_docf = nullptr;
    if (d_doc_off) {
        d_docf = d_work + sp_up16(n);
        uint32_t* d_invalid = (uint32_t*)(d_docf + sp_up16(n));
        GBPE_HIP(ctx, hipMemsetAsync(d_docf, 0, sp_up16(n) + 16, s));
        const int rc = gbpe_doc_flags_launch(ctx, d_doc_off, n_docs, n, d_docf, 1u, d_invalid);
        if (rc != GBPE_OK) return rc;
        GBPE_HIP(ctx, hipMemcpyAsync(ctx->enc_host_total, d_invalid, 4, hipMemcpyDeviceToHost, s));
        GBPE_HIP(ctx, hipStreamSynchronize(s));
        uint32_t bad = 0;
        memcpy(&bad, ctx->enc_host_total, 4);
        if (bad) return gbpe_doc_offsets_error(ctx, "specials mark", bad);   // nothing else was launched
    }
    return gbpe_specials_launch(ctx, sp, d_bytes, n, d_docf, d_cand, d_mark, nullptr);
}

}  // namespace

extern "C" int gbpe_specials_mark_device(gbpe_ctx* ctx, gbpe_specials* sp, const void* d_bytes, uint64_t n,
                                         const void* d_doc_off, uint64_t n_docs, void* d_mark_out) {
    if (!ctx || !sp || (n_docs && !d_doc_off) || (n && (!d_bytes || !d_mark_out)))
        return gbpe_set_error(ctx, GBPE_E_INVALID, "null argument");
    if ((uintptr_t)d_doc_off & 7u) return gbpe_set_error(ctx, GBPE_E_INVALID, "d_doc_off must be 8-byte aligned");
    if (n == 0 || (d_doc_off && n_docs == 0)) return GBPE_OK;
    GbpeArray<uint8_t> work;
    GBPE_HIP(ctx, work.reserve(ctx, sp_work_bytes(n)));
    const int rc = sp_mark_run(ctx, sp, (const uint8_t*)d_bytes, n, (const uint64_t*)d_doc_off, n_docs, work.p,
                               (uint8_t*)d_mark_out);
    const hipError_t e = hipStreamSynchronize(ctx->stream);   // (the work block goes back to the pool on return)
    if (rc != GBPE_OK) return rc;
    if (e != hipSuccess) return gbpe_set_error(ctx, GBPE_E_DEVICE, "specials mark failed: %s", hipGetErrorString(e));
    return GBPE_OK;
}

extern "C" int gbpe_specials_mark(gbpe_ctx* ctx, gbpe_specials* sp, const uint8_t* bytes, uint64_t n,
                                  const uint64_t* doc_off, uint64_t n_docs, uint8_t* mark_out) {
    if (!ctx || !sp || (n_docs && !doc_off) || (n && (!bytes || !mark_out)))
        return gbpe_set_error(ctx, GBPE_E_INVALID, "null argument");
    if (n == 0 || (doc_off && n_docs == 0)) return GBPE_OK;
    if (doc_off) {
        const int rc = gbpe_doc_offsets_check(ctx, "specials mark", doc_off, n_docs, n);   // before anything is launched
        if (rc != GBPE_OK) return rc;
    }
    hipStream_t s = ctx->stream;
    // one pooled block: offsets, bytes, mark, work
    const uint64_t o_in = doc_off ? sp_up16(8 * (n_docs + 1)) : 0, o_mark = o_in + sp_up16(n), o_work = o_mark + sp_up16(n);
    GbpeArray<uint8_t> io;
    GBPE_HIP(ctx, io.reserve(ctx, o_work + sp_work_bytes(n)));
    hipError_t e = doc_off ? hipMemcpyAsync(io.p, doc_off, 8 * (n_docs + 1), hipMemcpyHostToDevice, s) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(io.p + o_in, bytes, n, hipMemcpyHostToDevice, s);
    const int rc = e == hipSuccess ? sp_mark_run(ctx, sp, io.p + o_in, n, doc_off ? (const uint64_t*)io.p : nullptr, n_docs,
                                                 io.p + o_work, io.p + o_mark)
                                   : GBPE_OK;
    if (e == hipSuccess && rc == GBPE_OK) e = hipMemcpyAsync(mark_out, io.p + o_mark, n, hipMemcpyDeviceToHost, s);
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess) e = es;
    if (rc != GBPE_OK) return rc;
    if (e != hipSuccess) return gbpe_set_error(ctx, GBPE_E_DEVICE, "specials mark failed: %s", hipGetErrorString(e));
    return GBPE_OK;
}
