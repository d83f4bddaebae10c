// Device decode: token ids back to bytes (replaces the host loop of
// tokenizer.js:344-363 TrieTokenizer.decode).
//
// Decode is a gather with variable-length output: per-token byte lengths
// (k_dec_len, with the block-exclusive scan of scan.h's geometry), the scan of the
// block sums (k_chunk_scan2, unchanged), then a scatter of the vocab bytes
// (k_dec_scatter: output-stationary 16-byte vectors; k_dec_scatter_plain: one lane
// per token, GBPE_DEBUG dec_plain=1).  k_dec_doc_off turns document token offsets
// into document byte offsets and checks them.
//
// The vocab lives on the device as one 8-byte entry {blob offset, length} per id
// plus entry V for U+FFFD (tokenizer.js:18, 350): every lookup is ent[min(id, V)],
// so no id can become an out-of-range load.

#include "common.h"
#include "scan.h"

#include <algorithm>

namespace {

constexpr uint64_t kDecSlice = 32ull << 20;   // tokens per slice of the host forms
constexpr uint32_t kDecMaxEntry = 65535u;     // SCAN_BLK * 65535 < 2^32: a block's local prefix fits u32
constexpr uint32_t DEC_BLOB_PAD = 8u;          // zero bytes behind the blob: k_dec_scatter gathers 8 bytes at a time
constexpr uint32_t DEC_BAD_ORDER = 1u, DEC_BAD_FIRST = 2u, DEC_BAD_LAST = 4u;

// 4 tokens of one thread: one 16-byte load (dword-aligned address) inside [0, n),
// the stream's last partial group token by token; ids past the end read as 0 and
// are never used
__device__ __forceinline__ uint4 dec_load4(const uint32_t* __restrict__ tok, uint64_t n, uint64_t base) {
    if (base + 4 <= n) return *reinterpret_cast<const uint4*>(tok + base);
    uint4 t = make_uint4(0, 0, 0, 0);
    if (base < n) t.x = tok[base];
    if (base + 1 < n) t.y = tok[base + 1];
    if (base + 2 < n) t.z = tok[base + 2];
    return t;
}

// per SCAN_BLK tokens: each token's byte length, the block-exclusive prefix of the
// lengths (local) and the block's byte count (blocksum)
__global__ __launch_bounds__(SCAN_TPB) void k_dec_len(const uint32_t* __restrict__ tok, uint64_t n,
                                                      const uint2* __restrict__ ent, uint32_t nv,
                                                      uint32_t* __restrict__ local, uint64_t* __restrict__ blocksum) {
    __shared__ uint32_t wsum[SCAN_TPB / 64];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_BLK + (uint64_t)threadIdx.x * SCAN_PER;
    const uint4 t = dec_load4(tok, n, base);
    const uint32_t id[SCAN_PER] = {t.x, t.y, t.z, t.w};
    uint32_t v[SCAN_PER], s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER; ++k) {
        v[k] = (base + k < n) ? ent[min(id[k], nv)].y : 0u;
        s += v[k];
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t incl = s;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    uint32_t run = incl - s;
    for (int w = 0; w < wid; ++w) run += wsum[w];
    if (base + 4 <= n) {   // (local is 16-byte aligned and base a multiple of 4)
        *reinterpret_cast<uint4*>(local + base) = make_uint4(run, run + v[0], run + v[0] + v[1], run + v[0] + v[1] + v[2]);
        run += s;
    } else {
#pragma unroll
        for (int k = 0; k < SCAN_PER; ++k) {
            if (base + k < n) local[base + k] = run;
            run += v[k];
        }
    }
    if (threadIdx.x == SCAN_TPB - 1) blocksum[blockIdx.x] = run;
}

// one lane per entry of tok_off (n_ent of them): its byte offset — the scanned
// prefix of token tok_off[e], or the total at n.  An entry above n never indexes
// the prefix arrays.  check != 0: the entries are a call's whole offsets array
// (first 0, non-decreasing, last n); what fails goes into *flag.
__global__ __launch_bounds__(256) void k_dec_doc_off(const uint64_t* __restrict__ tok_off, uint64_t n_ent, uint64_t n,
                                                     const uint32_t* __restrict__ local,
                                                     const uint64_t* __restrict__ blocksum,
                                                     const uint64_t* __restrict__ total, int check,
                                                     uint64_t* __restrict__ byte_off, uint32_t* __restrict__ flag) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_ent) return;
    const uint64_t t = tok_off[e];
    uint32_t bad = 0;
    if (t > n) bad |= DEC_BAD_ORDER;   // (a later entry decreases or the last is not n)
    if (check) {
        if (e == 0 && t != 0) bad |= DEC_BAD_FIRST;
        if (e + 1 < n_ent && tok_off[e + 1] < t) bad |= DEC_BAD_ORDER;
        if (e + 1 == n_ent && t != n) bad |= DEC_BAD_LAST;
    }
    if (bad) atomicOr(flag, bad);
    byte_off[e] = t < n ? blocksum[t / SCAN_BLK] + local[t] : *total;
}

// The scatter, output-stationary: workgroup b owns tokens [b * SCAN_BLK, ...) and
// so the contiguous output range [B, E) = [blocksum[b], blocksum[b + 1]) (entry
// nblk is the total).  It stages the block's prefixes and blob offsets in LDS;
// each lane then produces whole 16-byte vectors of the 16-byte-aligned cover of
// [B, min(E, lim)), lim = min(total, out_cap): a binary search of the prefixes for
// the token holding the vector's first owned byte (the last token whose prefix is
// <= the byte's position: zero-length tokens before it are skipped), a walk
// forward gathering the tokens' bytes from the blob (up to 8 at a time) into four
// registers, one store.  Adjacent
// lanes write adjacent 16 bytes.  A vector shared with a neighbouring workgroup
// (the block's first and last) or cut by lim stores its owned bytes one by one.
__global__ __launch_bounds__(SCAN_TPB) void k_dec_scatter(const uint32_t* __restrict__ tok, uint64_t n,
                                                          const uint2* __restrict__ ent, uint32_t nv,
                                                          const uint8_t* __restrict__ blob,
                                                          const uint32_t* __restrict__ local,
                                                          const uint64_t* __restrict__ blocksum,   // nblk + 1 entries
                                                          uint8_t* __restrict__ out, uint64_t out_cap) {
    __shared__ uint32_t pre[SCAN_BLK + 1];
    __shared__ uint32_t boff[SCAN_BLK];
    const uint64_t B = blocksum[blockIdx.x], E = blocksum[blockIdx.x + 1];
    const uint64_t total = blocksum[gridDim.x];
    const uint64_t lim = min(total, out_cap);
    if (B >= lim || E <= B) return;   // (uniform over the workgroup)
    const uint32_t span = (uint32_t)(E - B);
    {
        const uint64_t base = (uint64_t)blockIdx.x * SCAN_BLK + (uint64_t)threadIdx.x * SCAN_PER;
        const uint4 t = dec_load4(tok, n, base);
        const uint32_t id[SCAN_PER] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int k = 0; k < SCAN_PER; ++k) {
            const bool in = base + k < n;
            pre[threadIdx.x * SCAN_PER + k] = in ? local[base + k] : span;   // (past the stream: never found)
            boff[threadIdx.x * SCAN_PER + k] = in ? ent[min(id[k], nv)].x : 0u;
        }
        if (threadIdx.x == 0) pre[SCAN_BLK] = span;
    }
    __syncthreads();
    const uint64_t end = min(E, lim);
    const uint64_t v0 = B & ~15ull;
    const uint64_t nvec = (((end + 15) & ~15ull) - v0) >> 4;
    for (uint64_t j = threadIdx.x; j < nvec; j += SCAN_TPB) {
        const uint64_t pos = v0 + j * 16;
        const uint32_t k0 = pos < B ? (uint32_t)(B - pos) : 0u;
        const uint32_t k1 = pos + 16 > end ? (uint32_t)(end - pos) : 16u;
        if (k0 >= k1) continue;
        const uint32_t r = (uint32_t)(pos + k0 - B);   // < span
        uint32_t i = 0;
#pragma unroll
        for (uint32_t step = SCAN_BLK / 2; step; step >>= 1)
            if (pre[i + step] <= r) i += step;
        // token i holds byte r (pre[i] <= r < pre[i + 1])
        uint32_t nxt = pre[i + 1];
        uint32_t rem = nxt - r;
        const uint8_t* src = blob + boff[i] + (r - pre[i]);
        uint64_t lo = 0, hi = 0;
        for (uint32_t k = k0; k < k1;) {
            if (rem == 0) {   // the next token (bytes remain, so i + 1 < SCAN_BLK)
                ++i;
                const uint32_t cur = nxt;
                nxt = pre[i + 1];
                rem = nxt - cur;
                src = blob + boff[i];
                continue;
            }
            // up to 8 bytes of the token at once: one unaligned 8-byte load (the blob is padded by
            // DEC_BLOB_PAD, so the bytes past the token's end exist), cut to `take`, shifted into place
            const uint32_t take = min(min(rem, 8u), k1 - k);
            uint64_t v;
            __builtin_memcpy(&v, src, 8);
            if (take < 8) v &= (1ull << (take * 8)) - 1;
            if (k < 8) {
                lo |= v << (k * 8);
                if (k && k + take > 8) hi |= v >> ((8 - k) * 8);
            } else {
                hi |= v << ((k - 8) * 8);
            }
            src += take;
            rem -= take;
            k += take;
        }
        if (k0 == 0 && k1 == 16) {
            *reinterpret_cast<uint4*>(out + pos) =
                make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
        } else {
            for (uint32_t k = k0; k < k1; ++k)
                out[pos + k] = (uint8_t)((k < 8 ? lo >> (k * 8) : hi >> ((k - 8) * 8)) & 0xFFu);
        }
    }
}

// the second path: one lane per token copies its bytes one by one to out + prefix
__global__ __launch_bounds__(256) void k_dec_scatter_plain(const uint32_t* __restrict__ tok, uint64_t n,
                                                           const uint2* __restrict__ ent, uint32_t nv,
                                                           const uint8_t* __restrict__ blob,
                                                           const uint32_t* __restrict__ local,
                                                           const uint64_t* __restrict__ blocksum, uint64_t nblk,
                                                           uint8_t* __restrict__ out, uint64_t out_cap) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t lim = min(blocksum[nblk], out_cap);
    const uint2 e = ent[min(tok[i], nv)];
    const uint64_t p = blocksum[i / SCAN_BLK] + local[i];
    for (uint32_t j = 0; j < e.y && p + j < lim; ++j) out[p + j] = blob[e.x + j];
}

int dec_offsets_error(gbpe_ctx* ctx, uint32_t bad) {
    return gbpe_set_error(ctx, GBPE_E_INVALID, "decode batch: token offsets %s",
                          (bad & DEC_BAD_FIRST)   ? "do not start at 0"
                          : (bad & DEC_BAD_ORDER) ? "decrease (or pass the end of the tokens)"
                                                  : "do not end at the token count");
}

}  // namespace

struct gbpe_vocab {
    gbpe_ctx* ctx = nullptr;
    uint2* ent = nullptr;      // n_tokens + 1 entries {blob offset, length}; the last is U+FFFD
    uint8_t* blob = nullptr;   // the entries' bytes end to end, then EF BF BD, then DEC_BLOB_PAD zero bytes
    uint32_t n_tokens = 0;
};

namespace {

struct DecPlan {   // device arrays of one pass over n tokens, inside ctx->dec_work
    uint64_t nblk;
    uint64_t* blocksum;   // nblk + 1 entries: [nblk] is the total
    uint32_t* flag;       // the offsets check of k_dec_doc_off (read back with the total: 16 bytes from blocksum + nblk)
    uint32_t* local;      // n entries, 16-byte aligned
};

int dec_plan(gbpe_ctx* ctx, uint64_t n, DecPlan* pl) {
    pl->nblk = gbpe_div_up(n, SCAN_BLK);
    const uint64_t head = ((pl->nblk + 2) * 8 + 15) & ~15ull;
    GBPE_HIP(ctx, ctx->dec_work.reserve(ctx, head + n * 4 + 16));
    pl->blocksum = (uint64_t*)ctx->dec_work.p;
    pl->flag = (uint32_t*)(pl->blocksum + pl->nblk + 1);
    pl->local = (uint32_t*)((uint8_t*)ctx->dec_work.p + head);
    return GBPE_OK;
}

// Lengths, scans and (n_ent > 0) the byte offsets of n_ent token offsets on device
// buffers, n > 0; one readback: the total and the offsets' status.  Nothing is
// written to an output buffer here.
int decode_measure(gbpe_ctx* ctx, const gbpe_vocab* v, const uint32_t* d_tok, uint64_t n, const uint64_t* d_tok_off,
                   uint64_t n_ent, int check, uint64_t* d_byte_off, const DecPlan& pl, uint64_t* total) {
    hipStream_t s = ctx->stream;
    GBPE_HIP(ctx, hipMemsetAsync(pl.flag, 0, 8, s));
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[0], s));
    hipLaunchKernelGGL(k_dec_len, dim3((uint32_t)pl.nblk), dim3(SCAN_TPB), 0, s, d_tok, n, (const uint2*)v->ent,
                       v->n_tokens, pl.local, pl.blocksum);
    GBPE_LAUNCH_CHECK(ctx);
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[1], s));
    hipLaunchKernelGGL(k_chunk_scan2, dim3(1), dim3(SCAN_TPB), 0, s, pl.blocksum, pl.nblk, pl.blocksum + pl.nblk);
    if (n_ent)
        hipLaunchKernelGGL(k_dec_doc_off, dim3((uint32_t)gbpe_div_up(n_ent, 256)), dim3(256), 0, s, d_tok_off, n_ent, n,
                           (const uint32_t*)pl.local, (const uint64_t*)pl.blocksum,
                           (const uint64_t*)(pl.blocksum + pl.nblk), check, d_byte_off, pl.flag);
    GBPE_LAUNCH_CHECK(ctx);
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[2], s));
    GBPE_HIP(ctx, hipMemcpyAsync(ctx->enc_host_total, pl.blocksum + pl.nblk, 16, hipMemcpyDeviceToHost, s));
    GBPE_HIP(ctx, hipStreamSynchronize(s));
    float a = 0, b = 0;
    hipEventElapsedTime(&a, ctx->ev[0], ctx->ev[1]);
    hipEventElapsedTime(&b, ctx->ev[1], ctx->ev[2]);
    ctx->dec_ms[0] = a;
    ctx->dec_ms[1] = b;
    ctx->dec_ms[2] = 0;
    uint64_t back[2];
    memcpy(back, ctx->enc_host_total, 16);
    *total = back[0];
    if ((uint32_t)back[1]) return dec_offsets_error(ctx, (uint32_t)back[1]);
    return GBPE_OK;
}

// the scatter of a measured pass: writes d_out[0, min(total, out_cap)) only
int decode_scatter(gbpe_ctx* ctx, const gbpe_vocab* v, const uint32_t* d_tok, uint64_t n, const DecPlan& pl,
                   uint8_t* d_out, uint64_t out_cap) {
    const bool plain = gbpe_debug_knob("dec_plain", 0) != 0;   // (read per call: tests run both paths)
    hipStream_t s = ctx->stream;
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[3], s));
    if (plain)
        hipLaunchKernelGGL(k_dec_scatter_plain, dim3((uint32_t)gbpe_div_up(n, 256)), dim3(256), 0, s, d_tok, n,
                           (const uint2*)v->ent, v->n_tokens, (const uint8_t*)v->blob, (const uint32_t*)pl.local,
                           (const uint64_t*)pl.blocksum, pl.nblk, d_out, out_cap);
    else
        hipLaunchKernelGGL(k_dec_scatter, dim3((uint32_t)pl.nblk), dim3(SCAN_TPB), 0, s, d_tok, n, (const uint2*)v->ent,
                           v->n_tokens, (const uint8_t*)v->blob, (const uint32_t*)pl.local,
                           (const uint64_t*)pl.blocksum, d_out, out_cap);
    GBPE_LAUNCH_CHECK(ctx);
    GBPE_HIP(ctx, hipEventRecord(ctx->ev[4], s));
    GBPE_HIP(ctx, hipStreamSynchronize(s));
    float c = 0;
    hipEventElapsedTime(&c, ctx->ev[3], ctx->ev[4]);
    ctx->dec_ms[2] = c;
    return GBPE_OK;
}

int decode_device_impl(gbpe_ctx* ctx, gbpe_vocab* v, const uint32_t* d_tok, uint64_t n, const uint64_t* d_tok_off,
                       uint64_t n_ent, uint8_t* d_out, uint64_t out_cap, uint64_t* d_byte_off, uint64_t* n_out) {
    if (n > (uint64_t)0xFFFFFFFFu * SCAN_BLK) return gbpe_set_error(ctx, GBPE_E_INVALID, "decode: too many tokens for one call");
    DecPlan pl;
    int rc = dec_plan(ctx, n, &pl);
    if (rc != GBPE_OK) return rc;
    uint64_t total = 0;
    rc = decode_measure(ctx, v, d_tok, n, d_tok_off, n_ent, 1, d_byte_off, pl, &total);
    if (rc != GBPE_OK) return rc;   // bad offsets: the scatter is not launched
    *n_out = total;
    if (total && out_cap) {
        rc = decode_scatter(ctx, v, d_tok, n, pl, d_out, out_cap);
        if (rc != GBPE_OK) return rc;
    }
    if (total > out_cap)
        return gbpe_set_error(ctx, GBPE_E_CAPACITY, "decode: output needs %llu bytes", (unsigned long long)total);
    return GBPE_OK;
}

// Host buffers in and out, slice by slice (n, and n_docs when tok_off is given,
// > 0; the offsets already checked).  A slice starts at any token; a document's
// byte offset comes from the slice that holds its first token (the entries equal
// to n from the last slice's total), shifted by the bytes of the slices before.
int decode_host_impl(gbpe_ctx* ctx, gbpe_vocab* v, const uint32_t* tokens, uint64_t n, const uint64_t* tok_off,
                     uint64_t n_docs, uint8_t* out, uint64_t out_cap, uint64_t* byte_off, uint64_t* n_out) {
    const uint64_t slice = (uint64_t)std::max<long>(1, gbpe_debug_knob("decode_slice", (long)kDecSlice));
    const uint64_t n_ent = tok_off ? n_docs + 1 : 0;
    std::vector<uint64_t> rel;
    uint64_t total = 0, e0 = 0;
    for (uint64_t s0 = 0; s0 < n; s0 += slice) {
        const uint64_t len = std::min(slice, n - s0), s1 = s0 + len;
        uint64_t e1 = e0;   // the entries of this slice: tokens [s0, s1), and n itself in the last
        while (e1 < n_ent && (tok_off[e1] < s1 || s1 == n)) ++e1;
        const uint64_t m = e1 - e0;
        const uint64_t tok_bytes = (len * 4 + 15) & ~15ull;
        DecPlan pl;
        int rc = dec_plan(ctx, len, &pl);
        if (rc != GBPE_OK) return rc;
        GBPE_HIP(ctx, ctx->dec_in.reserve(ctx, tok_bytes + 2 * m * 8 + 16));
        uint32_t* d_tok = (uint32_t*)ctx->dec_in.p;
        uint64_t* d_rel = (uint64_t*)((uint8_t*)ctx->dec_in.p + tok_bytes);
        uint64_t* d_boff = d_rel + m;
        GBPE_HIP(ctx, hipMemcpyAsync(d_tok, tokens + s0, len * 4, hipMemcpyHostToDevice, ctx->stream));
        if (m) {
            rel.resize(m);
            for (uint64_t e = 0; e < m; ++e) rel[e] = tok_off[e0 + e] - s0;
            GBPE_HIP(ctx, hipMemcpyAsync(d_rel, rel.data(), m * 8, hipMemcpyHostToDevice, ctx->stream));
        }
        uint64_t t = 0;
        rc = decode_measure(ctx, v, d_tok, len, d_rel, m, 0, d_boff, pl, &t);   // (synchronises: rel is free again)
        if (rc != GBPE_OK) return rc;
        if (m) GBPE_HIP(ctx, hipMemcpyAsync(byte_off + e0, d_boff, m * 8, hipMemcpyDeviceToHost, ctx->stream));
        const uint64_t fit = total < out_cap ? std::min(t, out_cap - total) : 0;   // never at or beyond out[out_cap]
        if (fit) {
            GBPE_HIP(ctx, ctx->dec_out.reserve(ctx, fit + 16));
            rc = decode_scatter(ctx, v, d_tok, len, pl, (uint8_t*)ctx->dec_out.p, fit);
            if (rc != GBPE_OK) return rc;
            GBPE_HIP(ctx, hipMemcpyAsync(out + total, ctx->dec_out.p, fit, hipMemcpyDeviceToHost, ctx->stream));
        }
        GBPE_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (uint64_t e = e0; e < e1; ++e) byte_off[e] += total;
        total += t;
        e0 = e1;
    }
    *n_out = total;
    if (total > out_cap)
        return gbpe_set_error(ctx, GBPE_E_CAPACITY, "decode: output needs %llu bytes", (unsigned long long)total);
    return GBPE_OK;
}

}  // namespace

extern "C" int gbpe_vocab_upload(gbpe_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, uint32_t n_tokens,
                                 gbpe_vocab** out) {
    if (!ctx || !out || !offsets) return gbpe_set_error(ctx, GBPE_E_INVALID, "vocab upload: null argument");
    *out = nullptr;
    if (n_tokens == 0xFFFFFFFFu) return gbpe_set_error(ctx, GBPE_E_INVALID, "vocab upload: too many entries");
    const uint64_t first = offsets[0];
    for (uint32_t i = 0; i < n_tokens; ++i) {
        if (offsets[i + 1] < offsets[i]) return gbpe_set_error(ctx, GBPE_E_INVALID, "vocab upload: offsets decrease at entry %u", i);
        if (offsets[i + 1] - offsets[i] > kDecMaxEntry)
            return gbpe_set_error(ctx, GBPE_E_INVALID, "vocab upload: entry %u has %llu bytes (at most %u)", i,
                                  (unsigned long long)(offsets[i + 1] - offsets[i]), kDecMaxEntry);
    }
    const uint64_t nb = offsets[n_tokens] - first;
    if (nb && !bytes) return gbpe_set_error(ctx, GBPE_E_INVALID, "vocab upload: null bytes");
    if (nb + 3 > 0xFFFFFFFFull) return gbpe_set_error(ctx, GBPE_E_INVALID, "vocab upload: more than 4 GiB of entry bytes");
    std::vector<uint2> ent((size_t)n_tokens + 1);
    for (uint32_t i = 0; i < n_tokens; ++i)
        ent[i] = make_uint2((uint32_t)(offsets[i] - first), (uint32_t)(offsets[i + 1] - offsets[i]));
    ent[n_tokens] = make_uint2((uint32_t)nb, 3u);
    static const uint8_t kReplacement[3] = {0xEF, 0xBF, 0xBD};   // U+FFFD (tokenizer.js:18)
    auto* v = new (std::nothrow) gbpe_vocab();
    if (!v) return gbpe_set_error(ctx, GBPE_E_OOM, "vocab upload: out of host memory");
    v->ctx = ctx;
    v->n_tokens = n_tokens;
    hipError_t e = dev_malloc(ctx, &v->ent, ent.size() * sizeof(uint2));
    if (e == hipSuccess) e = dev_malloc(ctx, &v->blob, nb + 3 + DEC_BLOB_PAD);
    if (e == hipSuccess) e = hipMemsetAsync(v->blob + nb + 3, 0, DEC_BLOB_PAD, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(v->ent, ent.data(), ent.size() * sizeof(uint2), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && nb) e = hipMemcpyAsync(v->blob, bytes + first, nb, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(v->blob + nb, kReplacement, 3, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (ent is a local)
    if (e != hipSuccess) {
        gbpe_vocab_free(v);
        return gbpe_set_error(ctx, e == hipErrorOutOfMemory ? GBPE_E_OOM : GBPE_E_DEVICE, "vocab upload failed: %s",
                              hipGetErrorString(e));
    }
    *out = v;
    return GBPE_OK;
}

extern "C" void gbpe_vocab_free(gbpe_vocab* v) {
    if (!v) return;
    if (v->ctx) hipStreamSynchronize(v->ctx->stream);
    hipFree(v->ent);
    hipFree(v->blob);
    delete v;
}

extern "C" int gbpe_decode_size(const uint64_t* vocab_offsets, uint32_t n_vocab, const uint32_t* tokens, uint64_t n_tokens,
                                uint64_t* n_bytes) {
    if (!vocab_offsets || !n_bytes || (n_tokens && !tokens)) return GBPE_E_INVALID;
    uint64_t s = 0;
    for (uint64_t i = 0; i < n_tokens; ++i) {
        const uint32_t t = tokens[i];
        s += t < n_vocab ? vocab_offsets[t + 1] - vocab_offsets[t] : 3u;
    }
    *n_bytes = s;
    return GBPE_OK;
}

extern "C" int gbpe_decode_device(gbpe_ctx* ctx, gbpe_vocab* v, const void* d_tokens, uint64_t n_tokens, void* d_out,
                                  uint64_t out_cap, uint64_t* n_out) {
    if (!ctx || !v || !n_out || (n_tokens && (!d_tokens || (!d_out && out_cap))))
        return gbpe_set_error(ctx, GBPE_E_INVALID, "null argument");
    *n_out = 0;
    if ((uintptr_t)d_tokens & 3u) return gbpe_set_error(ctx, GBPE_E_INVALID, "d_tokens must be 4-byte aligned");
    if ((uintptr_t)d_out & 15u) return gbpe_set_error(ctx, GBPE_E_INVALID, "d_out must be 16-byte aligned");
    if (n_tokens == 0) return GBPE_OK;
    return decode_device_impl(ctx, v, (const uint32_t*)d_tokens, n_tokens, nullptr, 0, (uint8_t*)d_out, out_cap, nullptr,
                              n_out);
}

extern "C" int gbpe_decode_batch_device(gbpe_ctx* ctx, gbpe_vocab* v, const void* d_tokens, uint64_t n_tokens,
                                        const void* d_tok_off, uint64_t n_docs, void* d_out, uint64_t out_cap,
                                        void* d_byte_off, uint64_t* n_out) {
    if (!ctx || !v || !n_out || !d_byte_off || (n_docs && !d_tok_off) ||
        (n_tokens && n_docs && (!d_tokens || (!d_out && out_cap))))
        return gbpe_set_error(ctx, GBPE_E_INVALID, "null argument");
    *n_out = 0;
    if ((uintptr_t)d_tokens & 3u) return gbpe_set_error(ctx, GBPE_E_INVALID, "d_tokens must be 4-byte aligned");
    if ((uintptr_t)d_out & 15u) return gbpe_set_error(ctx, GBPE_E_INVALID, "d_out must be 16-byte aligned");
    if (((uintptr_t)d_tok_off | (uintptr_t)d_byte_off) & 7u)
        return gbpe_set_error(ctx, GBPE_E_INVALID, "d_tok_off and d_byte_off must be 8-byte aligned");
    if (n_docs == 0 || n_tokens == 0) {
        GBPE_HIP(ctx, hipMemsetAsync(d_byte_off, 0, (n_docs + 1) * 8, ctx->stream));
        GBPE_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return GBPE_OK;
    }
    return decode_device_impl(ctx, v, (const uint32_t*)d_tokens, n_tokens, (const uint64_t*)d_tok_off, n_docs + 1,
                              (uint8_t*)d_out, out_cap, (uint64_t*)d_byte_off, n_out);
}

extern "C" int gbpe_decode(gbpe_ctx* ctx, gbpe_vocab* v, const uint32_t* tokens, uint64_t n_tokens, uint8_t* out,
                           uint64_t out_cap, uint64_t* n_out) {
    if (!ctx || !v || !n_out || (n_tokens && !tokens) || (out_cap && !out))
        return gbpe_set_error(ctx, GBPE_E_INVALID, "null argument");
    *n_out = 0;
    if (n_tokens == 0) return GBPE_OK;
    return decode_host_impl(ctx, v, tokens, n_tokens, nullptr, 0, out, out_cap, nullptr, n_out);
}

extern "C" int gbpe_decode_batch(gbpe_ctx* ctx, gbpe_vocab* v, const uint32_t* tokens, uint64_t n_tokens,
                                 const uint64_t* tok_off, uint64_t n_docs, uint8_t* out, uint64_t out_cap,
                                 uint64_t* byte_off, uint64_t* n_out) {
    if (!ctx || !v || !n_out || !byte_off || (n_docs && !tok_off) || (n_tokens && !tokens) || (out_cap && !out))
        return gbpe_set_error(ctx, GBPE_E_INVALID, "null argument");
    *n_out = 0;
    if (n_docs == 0) {
        byte_off[0] = 0;
        return GBPE_OK;
    }
    if (tok_off[0] != 0) return dec_offsets_error(ctx, DEC_BAD_FIRST);
    for (uint64_t d = 0; d < n_docs; ++d)
        if (tok_off[d + 1] < tok_off[d]) return dec_offsets_error(ctx, DEC_BAD_ORDER);
    if (tok_off[n_docs] != n_tokens) return dec_offsets_error(ctx, tok_off[n_docs] > n_tokens ? DEC_BAD_ORDER : DEC_BAD_LAST);
    if (n_tokens == 0) {
        for (uint64_t d = 0; d <= n_docs; ++d) byte_off[d] = 0;
        return GBPE_OK;
    }
    return decode_host_impl(ctx, v, tokens, n_tokens, tok_off, n_docs, out, out_cap, byte_off, n_out);
}

extern "C" int gbpe_decode_last_timing(gbpe_ctx* ctx, double* ms_len, double* ms_scan, double* ms_scatter) {
    if (!ctx) return GBPE_E_INVALID;
    if (ms_len) *ms_len = ctx->dec_ms[0];
    if (ms_scan) *ms_scan = ctx->dec_ms[1];
    if (ms_scatter) *ms_scatter = ctx->dec_ms[2];
    return GBPE_OK;
}
