// Internal definitions shared by the gpubpe HIP translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/gpubpe.h"

// Memory pool of a context (the header's "the library owns and pools device
// memory"; the reference pools its GPU buffers, tokenizer.js:30-46, 108-166):
// the buffers a trainer or shard frees go back to the pool and the next one of the
// context takes them (the same stream orders every use), so creating and
// destroying a trainer costs no hipMalloc / hipFree once the pool is warm.  Sizes
// round up to classes of <= 1/8 slack; a miss allocates; an allocation that finds
// no memory frees the idle blocks and tries again (so do the library's allocations
// outside the pool, gbpe_dev_malloc); idle blocks above half the device's memory are
// freed at once, and gbpe_ctx_trim gives every idle block back (for allocators
// outside the library).
struct GbpePool {
    std::multimap<uint64_t, void*> idle;          // class bytes -> block
    std::unordered_map<void*, uint64_t> busy;     // block -> class bytes
    uint64_t idle_bytes = 0, hits = 0, misses = 0;
};

// One work buffer of a context's encode, decode and pre-tokenise calls, outside the
// pool (plain hipMalloc through gbpe_dev_malloc): it grows and never shrinks
// (tokenizer.js:30-46 buffer pool), and its contents do not survive a growth.
struct GbpeGrowBuf {
    void* p = nullptr;
    uint64_t bytes = 0;
    // room for `need` bytes.  Enough already: nothing happens; otherwise the context's
    // stream is synchronised, the old buffer freed and need * 1.5 allocated
    // (amortised growth, tokenizer.js:125-128)
    hipError_t reserve(gbpe_ctx* ctx, uint64_t need);   // (api.hip)
    void free() {
        hipFree(p);
        p = nullptr, bytes = 0;
    }
};

struct gbpe_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;   // created by gbpe_ctx_create; `stream` may be a caller's
    hipStream_t copy_stream = nullptr;  // gbpe_encode's device-to-host copies of finished slices (created on first use)
    uint64_t total_mem = 0;
    int num_cu = 0;
    std::string err;
    // trie encode: chunk tokens; counts + scan state (+ chunk descriptors of a batch); byte / token
    // slice of the host forms; gbpe_encode_batch's per-document table (+ the host form's offsets)
    GbpeGrowBuf enc_scratch, enc_counts, enc_in, enc_out, enc_docs;
    uint32_t* enc_host_total = nullptr;   // pinned, 64 bytes: every call's read-back cell
    // decode: token slice / byte slice of the host forms, prefixes + document offsets
    GbpeGrowBuf dec_in, dec_out, dec_work;
    double dec_ms[3] = {0, 0, 0};
    GbpeGrowBuf pt_agg;   // pre-tokenizer block aggregates
    // (all nine are freed by gbpe_ctx_destroy)
    hipEvent_t ev[8] = {};
    double enc_ms[3] = {0, 0, 0};
    double bpe_ms[3] = {0, 0, 0};   // word-bounded merge-rank encode: word starts, long + walk, scan + compact
    GbpePool dpool, hpool;   // device / pinned host blocks of trainers and shards
    std::mutex pool_mu;
};

// pooled allocations (api.hip); host = pinned host memory (hipHostMalloc)
hipError_t gbpe_pool_alloc(gbpe_ctx* ctx, void** p, uint64_t bytes, bool host = false);
void gbpe_pool_free(gbpe_ctx* ctx, void* p, bool host = false);
void gbpe_pool_trim(gbpe_ctx* ctx);
hipError_t gbpe_dev_malloc(gbpe_ctx* ctx, void** p, uint64_t bytes);   // hipMalloc, trimming the pool on OOM
template <typename T>
inline hipError_t dev_malloc(gbpe_ctx* c, T** p, uint64_t n) { return gbpe_dev_malloc(c, (void**)p, n); }

// One block of the context pool, owned: `cap` elements at `p` (device, or pinned
// host with HOST), given back by the destructor.  Move-only.  An untyped array
// (T = void: the symbol type is chosen at run time) passes its element size to
// reserve / reserve_keep and keeps `cap` in those elements.
template <typename T, bool HOST = false>
struct GbpeArray {
    gbpe_ctx* ctx = nullptr;
    T* p = nullptr;
    uint64_t cap = 0;
    static constexpr uint64_t ESZ = sizeof(typename std::conditional<std::is_void<T>::value, char, T>::type);

    GbpeArray() = default;
    GbpeArray(GbpeArray&& o) noexcept : ctx(o.ctx), p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    GbpeArray& operator=(GbpeArray&& o) noexcept {
        if (this != &o) {
            release();
            ctx = o.ctx, p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~GbpeArray() { release(); }
    T* operator->() const { return p; }

    void release() {
        if (p) gbpe_pool_free(ctx, p, HOST);
        p = nullptr, cap = 0;
    }
    // room for n elements; the old contents are thrown away when the block has to grow
    hipError_t reserve(gbpe_ctx* c, uint64_t n, uint64_t esz = ESZ) {
        if (p && cap >= n) return hipSuccess;
        release();
        ctx = c;
        const hipError_t e = gbpe_pool_alloc(c, (void**)&p, n * esz, HOST);
        if (e == hipSuccess) cap = n;
        return e;
    }
    // room for n elements with the first `keep` kept: copied on the stream, one
    // synchronise, then the old block goes back to the pool
    hipError_t reserve_keep(gbpe_ctx* c, uint64_t n, uint64_t keep, hipStream_t s, uint64_t esz = ESZ) {
        if (p && cap >= n) return hipSuccess;
        GbpeArray nb;
        hipError_t e = nb.reserve(c, n, esz);
        if (e == hipSuccess && p && keep) e = hipMemcpyAsync(nb.p, p, keep * esz, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e == hipSuccess) *this = std::move(nb);
        return e;
    }
};

// ── error helpers ──────────────────────────────────────────────────────────
int gbpe_set_error(gbpe_ctx* ctx, int code, const char* fmt, ...);

#define GBPE_HIP(ctx, call)                                                              \
    do {                                                                                 \
        hipError_t _e = (call);                                                          \
        if (_e != hipSuccess)                                                            \
            return gbpe_set_error((ctx), _e == hipErrorOutOfMemory ? GBPE_E_OOM           \
                                                                   : GBPE_E_DEVICE,      \
                                  "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), \
                                  __FILE__, __LINE__);                                   \
    } while (0)

#define GBPE_LAUNCH_CHECK(ctx) GBPE_HIP(ctx, hipGetLastError())

// ── device helpers ─────────────────────────────────────────────────────────
__device__ __forceinline__ uint32_t gbpe_fmix32(uint32_t x) {
    // Murmur3 finaliser — the reference's pair hash (train.wgsl:62-67)
    x = (x ^ (x >> 16)) * 0x7feb352du;
    x = (x ^ (x >> 15)) * 0x846ca68bu;
    return x ^ (x >> 16);
}

__host__ __device__ static inline uint64_t gbpe_div_up(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// Debug / test overrides: GBPE_DEBUG="key=value,key=value" (DESIGN §6 lists the
// keys); every other tuning value is a compiled default
constexpr const char* kGbpeDebugKeys[] = {
    "lexicon", "lex_check", "rehash", "delta_mt", "zt", "rfl", "rflz", "lxwg", "lxtwo", "pair", "pseg", "prej", "zsmax", "zs32", "poison",
    "encode_slice", "decode_slice", "dec_plain", "me_cs", "htime", "ptrace", "rtime",
};

inline long gbpe_debug_knob(const char* key, long def) {
    const char* e = getenv("GBPE_DEBUG");
    if (!e) return def;
    const size_t kl = strlen(key);
    for (const char* p = e; *p;) {
        if (!strncmp(p, key, kl) && p[kl] == '=') return strtol(p + kl + 1, nullptr, 10);
        const char* c = strchr(p, ',');
        if (!c) break;
        p = c + 1;
    }
    return def;
}

// the key of the first GBPE_DEBUG entry that is not `<key of kGbpeDebugKeys>=value`
// ("" when every entry is; empty entries between commas pass): context and trainer
// creation refuse it, so that a misspelt or retired key cannot pass for the default
inline std::string gbpe_debug_unknown() {
    const char* e = getenv("GBPE_DEBUG");
    for (const char* p = e ? e : ""; *p;) {
        const size_t el = strcspn(p, ","), kl = strcspn(p, ",=");
        bool ok = el == 0;
        for (const char* k : kGbpeDebugKeys) ok = ok || (kl < el && strlen(k) == kl && !strncmp(p, k, kl));
        if (!ok) return std::string(p, kl ? kl : el);   // ("=1": the entry)
        p += el + (p[el] == ',');
    }
    return "";
}

// GPT-4 rule word starts of device bytes on ctx->stream (pretok.hip)
int gbpe_pretok_gpt4_launch(gbpe_ctx* ctx, const uint8_t* d_bytes, uint64_t n, uint8_t* d_ws);
// the same for many documents in one buffer: d_flags[n] (4-byte aligned) is non-zero where a document starts
int gbpe_pretok_gpt4_docs_launch(gbpe_ctx* ctx, const uint8_t* d_bytes, uint64_t n, const uint8_t* d_flags, uint8_t* d_ws);
// cl100k_base word starts of the same, d_flags == nullptr: one text
int gbpe_pretok_cl100k_launch(gbpe_ctx* ctx, const uint8_t* d_bytes, uint64_t n, const uint8_t* d_flags, uint8_t* d_ws);
// o200k_base word starts, the same arguments
int gbpe_pretok_o200k_launch(gbpe_ctx* ctx, const uint8_t* d_bytes, uint64_t n, const uint8_t* d_flags, uint8_t* d_ws);
// Document offsets of the batch calls (doc_off[n_docs + 1], from 0 to n, non-decreasing).
// k_doc_flags (pretok.hip), one lane per document: ORs what is wrong into *d_invalid
// (nullptr: unchecked) and `bit` into d_flags[doc_off[d]] (nullptr: no flags) for doc_off[d] < n.
constexpr uint32_t GBPE_DOC_BAD_ORDER = 1u, GBPE_DOC_BAD_FIRST = 2u, GBPE_DOC_BAD_LAST = 4u;
int gbpe_doc_flags_launch(gbpe_ctx* ctx, const uint64_t* d_doc_off, uint64_t n_docs, uint64_t n, uint8_t* d_flags,
                          uint32_t bit, uint32_t* d_invalid);
int gbpe_doc_offsets_check(gbpe_ctx* ctx, const char* what, const uint64_t* doc_off, uint64_t n_docs, uint64_t n);   // host
int gbpe_doc_offsets_error(gbpe_ctx* ctx, const char* what, uint32_t bad);
// Special tokens (special.hip): d_mark[n] = 0 / 1 + index / 255 (gpubpe.h) of d_bytes[n] on
// ctx->stream.  d_cand is n bytes of work, 16-byte aligned; d_doc_flags (nullptr: one document)
// is non-zero where a document starts; d_flags (nullptr: none) gets 1 at byte 0, at each accepted
// special's first byte and at the byte after its last: the pre-tokeniser's piece starts.
int gbpe_specials_launch(gbpe_ctx* ctx, const gbpe_specials* sp, const uint8_t* d_bytes, uint64_t n,
                         const uint8_t* d_doc_flags, uint8_t* d_cand, uint8_t* d_mark, uint8_t* d_flags);
const uint32_t* gbpe_specials_ids(const gbpe_specials* sp);   // device: the ids in the caller's order
// heuristic (byte-class) word starts of device bytes on ctx->stream (train.hip); any alignment
int gbpe_word_boundary_launch(gbpe_ctx* ctx, const uint8_t* d_bytes, uint64_t n, uint8_t* d_ws);
