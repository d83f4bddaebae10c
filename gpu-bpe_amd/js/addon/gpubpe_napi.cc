// Node.js N-API addon over the gpubpe C-ABI (include/gpubpe.h).
//
// This is the native half of the drop-in for the reference's device layer
// (src/bpe/engine.js + WGSL).  The JS modules beside it (engine.js,
// trainer.js, tokenizer.js) keep the reference's API.  Long-running calls
// (trainer steps, encode) run as napi_async_work off the JS thread and
// resolve Promises, so the event loop never blocks — the role the Web
// Worker + yieldToEventLoop play in the reference (bpe-worker.js,
// trainer.js:39-41, 317).
//
// Exports:
//   createContext(device) -> ctx                 limits(ctx) -> {maxBufferSize}
//   kernelNames() -> string[]                    destroyContext(ctx)
//   trainerCreate(ctx, bytes, wordStarts|null, {targetVocabSize, vocabSize, nextTokenId, batchSize, exact}) -> trainer
//   trainerStep(trainer, maxMerges) -> Promise<{merges: Uint32Array [a,b,id,count]*, earlyStop, symbolCount}>
//   trainerDestroy(trainer)
//   trieUpload(ctx, nodes: Uint32Array, edges: Uint32Array) -> trie      trieFree(trie)
//   encode(ctx, trie, bytes, chunkSize) -> Promise<Uint32Array>
//   encodeBatch(ctx, trie, bytes, offsets: Float64Array, chunkSize) -> Promise<{tokens: Uint32Array, offsets: Float64Array}>
//   bpeEncodeWordsBatch(ctx, bpe, bytes, offsets: Float64Array, wordStarts | null, mode) -> {tokens: Uint32Array, offsets: Float64Array}
//   specialsUpload(ctx, bytes, offsets: Float64Array, ids: Uint32Array) -> external; specialsMark(ctx, specials, bytes, offsets | null) -> Uint8Array
//   bpeEncodeSpecial(ctx, bpe, specials, bytes, wordStarts | null, mode) / bpeEncodeSpecialBatch(ctx, bpe, specials, bytes, offsets, wordStarts | null, mode)
//   pretokenizeGpt4Batch(ctx, bytes, offsets: Float64Array) -> Uint8Array
//   pretokenizeO200k(ctx, bytes) / pretokenizeO200kBatch(ctx, bytes, offsets) -> Uint8Array: the o200k_base split pattern's
//   pretokenizeCl100k(ctx, bytes) / pretokenizeCl100kBatch(ctx, bytes, offsets) -> Uint8Array: the cl100k_base split
//   vocabUpload(ctx, bytes: Uint8Array, offsets: Float64Array) -> vocab   vocabFree(vocab)
//   decode(ctx, vocab, tokens: Uint32Array) -> Promise<Uint8Array>
//   decodeBatch(ctx, vocab, tokens: Uint32Array, offsets: Float64Array) -> Promise<{bytes: Uint8Array, offsets: Float64Array}>
//   wordBoundary(ctx, bytes) -> Uint8Array
//
// Concurrency and lifetimes.  Every call that touches a context's device state
// (its stream, pooled encode buffers, error string) holds that context's mutex,
// so overlapping Promises (Promise.all over encode / trainerStep) run one after
// the other on the device instead of racing (the reference serialises them on
// one WebGPU queue).  Contexts are reference-counted by their trainers, tries,
// BPE tables, device vocabs and in-flight work: destroyContext() closes a context for new
// calls, and the device context is freed when the last of those is gone.
// trainerDestroy() / trieFree() / vocabFree() during a step / encode / decode
// defer the free to its completion.
#include <node_api.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "gpubpe.h"

#define NAPI_CALL(env, call)                                                       \
    do {                                                                           \
        if ((call) != napi_ok) {                                                   \
            napi_throw_error((env), nullptr, "gpubpe addon: N-API call failed");   \
            return nullptr;                                                        \
        }                                                                          \
    } while (0)

namespace {

// All reference counts below change on the JS thread only (calls, finalizers,
// async-work completions); worker threads only take `mu`.
struct Ctx {
    gbpe_ctx* ctx = nullptr;
    std::mutex mu;          // serialises device work on this context
    int refs = 1;           // the JS external + children + in-flight work
    bool closed = false;    // destroyContext() was called
    bool js_ref = true;     // the JS external's reference is still held
};
void ctx_release(Ctx* c) {
    if (c && --c->refs == 0) {
        if (c->ctx) gbpe_ctx_destroy(c->ctx);
        delete c;
    }
}
bool ctx_usable(const Ctx* c) { return c && c->ctx && !c->closed; }

struct Trainer {
    gbpe_trainer* t = nullptr;
    Ctx* owner = nullptr;
    uint32_t batch = 128;
    int inflight = 0;              // queued / running trainerStep works
    bool destroy_pending = false;  // trainerDestroy() while a step ran
};
void trainer_free(Trainer* t) {   // the device trainer and its context reference
    if (t->t) {
        std::lock_guard<std::mutex> g(t->owner->mu);
        gbpe_trainer_destroy(t->t);
        t->t = nullptr;
    }
    if (t->owner) {
        ctx_release(t->owner);
        t->owner = nullptr;
    }
}
struct Trie {
    gbpe_trie* trie = nullptr;
    Ctx* owner = nullptr;
    int inflight = 0;
    bool destroy_pending = false;
};
void trie_free(Trie* t) {
    if (t->trie) {
        std::lock_guard<std::mutex> g(t->owner->mu);
        gbpe_trie_free(t->trie);
        t->trie = nullptr;
    }
    if (t->owner) {
        ctx_release(t->owner);
        t->owner = nullptr;
    }
}

std::string last_error(gbpe_ctx* c, const char* what, int rc) {
    std::string m = what;
    m += ": ";
    const char* e = c ? gbpe_last_error(c) : nullptr;
    m += (e && *e) ? e : "gpubpe error";
    m += " (status " + std::to_string(rc) + ")";
    return m;
}

napi_value throw_status(napi_env env, gbpe_ctx* c, const char* what, int rc) {
    napi_throw_error(env, nullptr, last_error(c, what, rc).c_str());
    return nullptr;
}

template <typename T>
T* unwrap_external(napi_env env, napi_value v) {
    void* p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok) return nullptr;
    return static_cast<T*>(p);
}

bool get_bytes(napi_env env, napi_value v, const uint8_t** data, size_t* len) {
    bool is_ta = false;
    napi_is_typedarray(env, v, &is_ta);
    if (!is_ta) return false;
    napi_typedarray_type type;
    size_t length = 0, offset = 0;
    void* raw = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, v, &type, &length, &raw, &ab, &offset) != napi_ok) return false;
    if (type != napi_uint8_array) return false;
    *data = static_cast<const uint8_t*>(raw);
    *len = length;
    return true;
}

bool get_u32s(napi_env env, napi_value v, const uint32_t** data, size_t* len) {
    bool is_ta = false;
    napi_is_typedarray(env, v, &is_ta);
    if (!is_ta) return false;
    napi_typedarray_type type;
    size_t length = 0, offset = 0;
    void* raw = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, v, &type, &length, &raw, &ab, &offset) != napi_ok) return false;
    if (type != napi_uint32_array) return false;
    *data = static_cast<const uint32_t*>(raw);
    *len = length;
    return true;
}

uint32_t get_u32_prop(napi_env env, napi_value obj, const char* name, uint32_t dflt) {
    bool has = false;
    if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return dflt;
    napi_value v;
    napi_get_named_property(env, obj, name, &v);
    napi_valuetype t;
    napi_typeof(env, v, &t);
    if (t == napi_boolean) {
        bool b = false;
        napi_get_value_bool(env, v, &b);
        return b ? 1u : 0u;
    }
    if (t != napi_number) return dflt;
    uint32_t out = dflt;
    napi_get_value_uint32(env, v, &out);
    return out;
}

napi_value make_u32_array(napi_env env, const uint32_t* src, size_t n) {
    napi_value ab, ta;
    void* dst = nullptr;
    if (napi_create_arraybuffer(env, n * 4, &dst, &ab) != napi_ok) return nullptr;
    if (n) memcpy(dst, src, n * 4);
    if (napi_create_typedarray(env, napi_uint32_array, n, ab, 0, &ta) != napi_ok) return nullptr;
    return ta;
}

// ── context ──────────────────────────────────────────────────────────────

void ctx_finalize(napi_env, void* data, void*) {
    Ctx* c = static_cast<Ctx*>(data);
    if (c->js_ref) {
        c->js_ref = false;
        ctx_release(c);
    }
}

napi_value CreateContext(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    int32_t dev = 0;
    if (argc >= 1) napi_get_value_int32(env, argv[0], &dev);
    auto* c = new Ctx();
    int rc = gbpe_ctx_create(dev, &c->ctx);
    if (rc != GBPE_OK) {
        delete c;
        std::string m = "No usable HIP device " + std::to_string(dev) + ": " + gbpe_last_error(nullptr) +
                        " (gbpe_ctx_create status " + std::to_string(rc) + ")";
        napi_throw_error(env, nullptr, m.c_str());
        return nullptr;
    }
    napi_value ext;
    NAPI_CALL(env, napi_create_external(env, c, ctx_finalize, nullptr, &ext));
    return ext;
}

napi_value DestroyContext(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    if (c && !c->closed) {   // freed once its trainers, tries and in-flight work are gone
        c->closed = true;
        if (c->js_ref) {
            c->js_ref = false;
            ctx_release(c);
        }
    }
    return nullptr;
}

napi_value Limits(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    if (!ctx_usable(c)) {
        napi_throw_type_error(env, nullptr, "limits(ctx): invalid context");
        return nullptr;
    }
    uint64_t mb = 0;
    std::unique_lock<std::mutex> g(c->mu);
    int rc = gbpe_ctx_limits(c->ctx, &mb);
    g.unlock();
    if (rc != GBPE_OK) return throw_status(env, c->ctx, "limits", rc);
    napi_value obj, v;
    NAPI_CALL(env, napi_create_object(env, &obj));
    NAPI_CALL(env, napi_create_double(env, (double)mb, &v));
    NAPI_CALL(env, napi_set_named_property(env, obj, "maxBufferSize", v));
    return obj;
}

napi_value KernelNames(napi_env env, napi_callback_info) {
    napi_value arr;
    const int n = gbpe_kernel_count();
    NAPI_CALL(env, napi_create_array_with_length(env, n, &arr));
    for (int i = 0; i < n; ++i) {
        napi_value s;
        NAPI_CALL(env, napi_create_string_utf8(env, gbpe_kernel_name(i), NAPI_AUTO_LENGTH, &s));
        NAPI_CALL(env, napi_set_element(env, arr, i, s));
    }
    return arr;
}

napi_value WordBoundary(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc >= 1 ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    const uint8_t* data = nullptr;
    size_t len = 0;
    if (!ctx_usable(c) || argc < 2 || !get_bytes(env, argv[1], &data, &len)) {
        napi_throw_type_error(env, nullptr, "wordBoundary(ctx, Uint8Array)");
        return nullptr;
    }
    napi_value ab, ta;
    void* dst = nullptr;
    NAPI_CALL(env, napi_create_arraybuffer(env, len, &dst, &ab));
    std::unique_lock<std::mutex> g(c->mu);
    int rc = gbpe_word_boundary(c->ctx, data, len, static_cast<uint8_t*>(dst));
    g.unlock();
    if (rc != GBPE_OK) return throw_status(env, c->ctx, "wordBoundary", rc);
    NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, len, ab, 0, &ta));
    return ta;
}

// GPT-4 rule word starts (PreTokenizer.preTokenizeBytes, pre_tokenizer.mjs:459-509), or with
// rules 1 those of the cl100k_base split pattern (gbpe_pretokenize_cl100k), 2 of o200k_base's (gbpe_pretokenize_o200k)
static napi_value pretokenize(napi_env env, napi_callback_info info, int rules) {
    static const char* const names[3] = {"pretokenizeGpt4", "pretokenizeCl100k", "pretokenizeO200k"};
    static const char* const usage[3] = {"pretokenizeGpt4(ctx, Uint8Array)", "pretokenizeCl100k(ctx, Uint8Array)",
                                         "pretokenizeO200k(ctx, Uint8Array)"};
    const char* name = names[rules];
    size_t argc = 2;
    napi_value argv[2];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc >= 1 ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    const uint8_t* data = nullptr;
    size_t len = 0;
    if (!ctx_usable(c) || argc < 2 || !get_bytes(env, argv[1], &data, &len)) {
        napi_throw_type_error(env, nullptr, usage[rules]);
        return nullptr;
    }
    napi_value ab, ta;
    void* dst = nullptr;
    NAPI_CALL(env, napi_create_arraybuffer(env, len, &dst, &ab));
    std::unique_lock<std::mutex> g(c->mu);
    int rc = (rules == 2 ? gbpe_pretokenize_o200k : rules == 1 ? gbpe_pretokenize_cl100k : gbpe_pretokenize_gpt4)(
        c->ctx, data, len, static_cast<uint8_t*>(dst));
    g.unlock();
    if (rc != GBPE_OK) return throw_status(env, c->ctx, name, rc);
    NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, len, ab, 0, &ta));
    return ta;
}
napi_value PretokenizeGpt4(napi_env env, napi_callback_info info) { return pretokenize(env, info, 0); }
napi_value PretokenizeCl100k(napi_env env, napi_callback_info info) { return pretokenize(env, info, 1); }
napi_value PretokenizeO200k(napi_env env, napi_callback_info info) { return pretokenize(env, info, 2); }

// ── trainer ──────────────────────────────────────────────────────────────

void trainer_finalize(napi_env, void* data, void*) {
    Trainer* t = static_cast<Trainer*>(data);
    trainer_free(t);   // (in-flight steps hold a reference to the external: none runs now)
    delete t;
}

napi_value TrainerCreate(napi_env env, napi_callback_info info) {
    size_t argc = 4;
    napi_value argv[4];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc >= 1 ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    const uint8_t* data = nullptr;
    size_t len = 0;
    if (!ctx_usable(c) || argc < 4 || !get_bytes(env, argv[1], &data, &len)) {
        napi_throw_type_error(env, nullptr, "trainerCreate(ctx, Uint8Array, wordStarts|null, opts)");
        return nullptr;
    }
    const uint8_t* ws = nullptr;
    size_t wslen = 0;
    napi_valuetype wt;
    napi_typeof(env, argv[2], &wt);
    if (wt != napi_null && wt != napi_undefined) {
        if (!get_bytes(env, argv[2], &ws, &wslen) || wslen != len) {
            napi_throw_type_error(env, nullptr, "wordStarts must be a Uint8Array of the byte length");
            return nullptr;
        }
    }
    gbpe_train_opts o{};
    o.target_vocab_size = get_u32_prop(env, argv[3], "targetVocabSize", 4096);
    o.vocab_size = get_u32_prop(env, argv[3], "vocabSize", 256);
    o.next_token_id = get_u32_prop(env, argv[3], "nextTokenId", 256);
    o.batch_size = get_u32_prop(env, argv[3], "batchSize", GBPE_BATCH_SIZE);
    o.flags = get_u32_prop(env, argv[3], "exact", 0) ? GBPE_TRAIN_EXACT_COMPACTION : 0u;
    auto* t = new Trainer();
    t->batch = o.batch_size ? o.batch_size : GBPE_BATCH_SIZE;
    std::unique_lock<std::mutex> g(c->mu);
    int rc = gbpe_trainer_create(c->ctx, data, len, ws, 0, &o, &t->t);
    g.unlock();
    if (rc == GBPE_OK) {
        t->owner = c;
        ++c->refs;
    } else {
        delete t;
        if (rc == GBPE_E_EMPTY) {
            napi_throw_error(env, nullptr, "No symbols to train on — corpus is empty after pre-processing");
            return nullptr;
        }
        return throw_status(env, c->ctx, "train", rc);
    }
    napi_value ext;
    NAPI_CALL(env, napi_create_external(env, t, trainer_finalize, nullptr, &ext));
    return ext;
}

napi_value TrainerDestroy(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Trainer* t = argc ? unwrap_external<Trainer>(env, argv[0]) : nullptr;
    if (t && t->t) {
        if (t->inflight) t->destroy_pending = true;   // step_complete frees it
        else trainer_free(t);
    }
    return nullptr;
}

struct StepWork {
    napi_async_work work = nullptr;
    napi_deferred deferred = nullptr;
    napi_ref keep = nullptr;   // keeps the trainer external alive while the work runs
    Trainer* tr = nullptr;
    uint32_t max_merges = 0;
    std::vector<uint32_t> merges;
    uint32_t n_done = 0, early = 0;
    uint64_t symbols = 0;
    int rc = GBPE_OK;
    std::string err;
};

void step_execute(napi_env, void* data) {
    auto* w = static_cast<StepWork*>(data);
    w->merges.assign((size_t)w->tr->batch * 4, 0);
    std::lock_guard<std::mutex> g(w->tr->owner->mu);
    w->rc = gbpe_trainer_step(w->tr->t, w->max_merges, w->merges.data(), &w->n_done, &w->early);
    if (w->rc != GBPE_OK) {
        w->err = last_error(w->tr->owner->ctx, "train step", w->rc);
        return;
    }
    gbpe_trainer_stats st;
    if (gbpe_trainer_stats_get(w->tr->t, &st) == GBPE_OK) w->symbols = st.symbol_count;
}

void step_complete(napi_env env, napi_status, void* data) {
    auto* w = static_cast<StepWork*>(data);
    if (w->rc != GBPE_OK) {
        napi_value msg, err;
        napi_create_string_utf8(env, w->err.c_str(), NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, nullptr, msg, &err);
        napi_reject_deferred(env, w->deferred, err);
    } else {
        napi_value obj, v;
        napi_create_object(env, &obj);
        napi_set_named_property(env, obj, "merges", make_u32_array(env, w->merges.data(), (size_t)w->n_done * 4));
        napi_get_boolean(env, w->early != 0, &v);
        napi_set_named_property(env, obj, "earlyStop", v);
        napi_create_double(env, (double)w->symbols, &v);
        napi_set_named_property(env, obj, "symbolCount", v);
        napi_resolve_deferred(env, w->deferred, obj);
    }
    if (--w->tr->inflight == 0 && w->tr->destroy_pending) trainer_free(w->tr);
    napi_delete_reference(env, w->keep);
    napi_delete_async_work(env, w->work);
    delete w;
}

napi_value TrainerStep(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value argv[2];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Trainer* t = argc >= 1 ? unwrap_external<Trainer>(env, argv[0]) : nullptr;
    if (!t || !t->t || t->destroy_pending) {
        napi_throw_type_error(env, nullptr, "trainerStep(trainer, maxMerges): invalid trainer");
        return nullptr;
    }
    auto* w = new StepWork();
    w->tr = t;
    ++t->inflight;   // (the trainer holds its context: it outlives the work)
    if (argc >= 2) napi_get_value_uint32(env, argv[1], &w->max_merges);
    napi_value promise, name;
    NAPI_CALL(env, napi_create_promise(env, &w->deferred, &promise));
    NAPI_CALL(env, napi_create_reference(env, argv[0], 1, &w->keep));
    NAPI_CALL(env, napi_create_string_utf8(env, "gpubpe.trainerStep", NAPI_AUTO_LENGTH, &name));
    NAPI_CALL(env, napi_create_async_work(env, nullptr, name, step_execute, step_complete, w, &w->work));
    NAPI_CALL(env, napi_queue_async_work(env, w->work));
    return promise;
}

// ── trie + encode ────────────────────────────────────────────────────────

void trie_finalize(napi_env, void* data, void*) {
    Trie* t = static_cast<Trie*>(data);
    trie_free(t);
    delete t;
}

napi_value TrieUpload(napi_env env, napi_callback_info info) {
    size_t argc = 3;
    napi_value argv[3];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc >= 1 ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    const uint32_t *nodes = nullptr, *edges = nullptr;
    size_t nn = 0, ne = 0;
    if (!ctx_usable(c) || argc < 3 || !get_u32s(env, argv[1], &nodes, &nn) || !get_u32s(env, argv[2], &edges, &ne)) {
        napi_throw_type_error(env, nullptr, "trieUpload(ctx, nodes: Uint32Array, edges: Uint32Array)");
        return nullptr;
    }
    auto* t = new Trie();
    std::unique_lock<std::mutex> g(c->mu);
    int rc = gbpe_trie_upload(c->ctx, nodes, (uint32_t)(nn / 3), edges, (uint32_t)(ne / 2), &t->trie);
    g.unlock();
    if (rc == GBPE_OK) {
        t->owner = c;
        ++c->refs;
    }
    if (rc != GBPE_OK) {
        delete t;
        return throw_status(env, c->ctx, "trie upload", rc);
    }
    napi_value ext;
    NAPI_CALL(env, napi_create_external(env, t, trie_finalize, nullptr, &ext));
    return ext;
}

napi_value TrieFree(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Trie* t = argc ? unwrap_external<Trie>(env, argv[0]) : nullptr;
    if (t && t->trie) {
        if (t->inflight) t->destroy_pending = true;   // encode_complete frees it
        else trie_free(t);
    }
    return nullptr;
}

// ── merge-rank encoder (TokenizerManager.encode, tokenizer-manager.js:13-61) ──

struct Bpe {
    gbpe_bpe* bpe = nullptr;
    Ctx* owner = nullptr;
};

void bpe_finalize(napi_env, void* data, void*) {
    Bpe* b = static_cast<Bpe*>(data);
    if (b->bpe) {
        std::lock_guard<std::mutex> g(b->owner->mu);
        gbpe_bpe_free(b->bpe);
    }
    ctx_release(b->owner);
    delete b;
}

struct Specials {
    gbpe_specials* sp = nullptr;
    Ctx* owner = nullptr;
};

void specials_finalize(napi_env, void* data, void*) {
    Specials* s = static_cast<Specials*>(data);
    if (s->sp) {
        std::lock_guard<std::mutex> g(s->owner->mu);
        gbpe_specials_free(s->sp);
    }
    ctx_release(s->owner);
    delete s;
}

// bpeUpload (ids up to 0xFFFF) and bpeUploadWide (up to GBPE_BPE_MAX_ID): the same handle
napi_value bpe_upload(napi_env env, napi_callback_info info, bool wide) {
    size_t argc = 2;
    napi_value argv[2];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc >= 1 ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    const uint32_t* m = nullptr;
    size_t nm = 0;
    if (!ctx_usable(c) || argc < 2 || !get_u32s(env, argv[1], &m, &nm)) {
        napi_throw_type_error(env, nullptr, wide ? "bpeUploadWide(ctx, merges: Uint32Array [a,b,id]*)"
                                                 : "bpeUpload(ctx, merges: Uint32Array [a,b,id]*)");
        return nullptr;
    }
    auto* b = new Bpe();
    std::unique_lock<std::mutex> g(c->mu);
    int rc = wide ? gbpe_bpe_upload_wide(c->ctx, m, (uint32_t)(nm / 3), &b->bpe)
                  : gbpe_bpe_upload(c->ctx, m, (uint32_t)(nm / 3), &b->bpe);
    g.unlock();
    if (rc == GBPE_OK) {
        b->owner = c;
        ++c->refs;
    }
    if (rc != GBPE_OK) {
        delete b;
        return throw_status(env, c->ctx, "bpe upload", rc);
    }
    napi_value ext;
    NAPI_CALL(env, napi_create_external(env, b, bpe_finalize, nullptr, &ext));
    return ext;
}

napi_value BpeUpload(napi_env env, napi_callback_info info) { return bpe_upload(env, info, false); }
napi_value BpeUploadWide(napi_env env, napi_callback_info info) { return bpe_upload(env, info, true); }

napi_value BpeEncode(napi_env env, napi_callback_info info) {
    size_t argc = 3;
    napi_value argv[3];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc >= 1 ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    Bpe* b = argc >= 2 ? unwrap_external<Bpe>(env, argv[1]) : nullptr;
    const uint8_t* data = nullptr;
    size_t len = 0;
    if (!ctx_usable(c) || !b || !b->bpe || argc < 3 || !get_bytes(env, argv[2], &data, &len)) {
        napi_throw_type_error(env, nullptr, "bpeEncode(ctx, bpe, Uint8Array)");
        return nullptr;
    }
    std::vector<uint32_t> out(len ? len : 1);
    uint64_t n = 0;
    std::unique_lock<std::mutex> g(c->mu);
    int rc = gbpe_bpe_encode(c->ctx, b->bpe, data, len, out.data(), out.size(), &n);
    g.unlock();
    if (rc != GBPE_OK) return throw_status(env, c->ctx, "bpe encode", rc);
    return make_u32_array(env, out.data(), (size_t)n);
}

// bpeEncodeWords(ctx, bpe, bytes, wordStarts | null, mode): the merges inside each
// word alone (gbpe_bpe_encode_words; mode = GBPE_WORDS_*: 1 takes the mask, 2, 3, 4 and 6
// compute it on the device)
// (`special`: bpeEncodeSpecial, the same with a special table after bpe — gbpe_bpe_encode_special)
napi_value bpe_encode_words(napi_env env, napi_callback_info info, bool special) {
    const size_t o = special ? 1 : 0;
    size_t argc = 6;
    napi_value argv[6];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc >= 1 ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    Bpe* b = argc >= 2 ? unwrap_external<Bpe>(env, argv[1]) : nullptr;
    Specials* sp = special && argc >= 3 ? unwrap_external<Specials>(env, argv[2]) : nullptr;
    const uint8_t *data = nullptr, *ws = nullptr;
    size_t len = 0, ws_len = 0;
    uint32_t mode = 0;
    bool ok = ctx_usable(c) && b && b->bpe && (!special || (sp && sp->sp)) && argc >= 5 + o &&
              get_bytes(env, argv[2 + o], &data, &len) && napi_get_value_uint32(env, argv[4 + o], &mode) == napi_ok;
    bool has_ws = false;
    if (ok) {
        napi_valuetype vt;
        ok = napi_typeof(env, argv[3 + o], &vt) == napi_ok;
        has_ws = ok && vt != napi_null && vt != napi_undefined;
        if (has_ws) ok = get_bytes(env, argv[3 + o], &ws, &ws_len) && ws_len == len;
    }
    if (!ok) {
        napi_throw_type_error(env, nullptr,
                              special ? "bpeEncodeSpecial(ctx, bpe, specials, Uint8Array, wordStarts: Uint8Array of the same "
                                        "length | null, mode)"
                                      : "bpeEncodeWords(ctx, bpe, Uint8Array, wordStarts: Uint8Array of the same length | "
                                        "null, mode)");
        return nullptr;
    }
    static const uint8_t kNoByte = 0;
    if (has_ws && !ws) ws = &kNoByte;   // (an empty mask still goes with mode 1)
    std::vector<uint32_t> out(len ? len : 1);
    uint64_t n = 0;
    std::unique_lock<std::mutex> g(c->mu);
    const uint8_t* m = has_ws ? ws : nullptr;
    int rc = special ? gbpe_bpe_encode_special(c->ctx, b->bpe, sp->sp, data, len, m, mode, out.data(), out.size(), &n)
                     : gbpe_bpe_encode_words(c->ctx, b->bpe, data, len, m, mode, out.data(), out.size(), &n);
    g.unlock();
    if (rc != GBPE_OK) return throw_status(env, c->ctx, special ? "bpe encode (special)" : "bpe encode (words)", rc);
    return make_u32_array(env, out.data(), (size_t)n);
}
napi_value BpeEncodeWords(napi_env env, napi_callback_info info) { return bpe_encode_words(env, info, false); }
napi_value BpeEncodeSpecial(napi_env env, napi_callback_info info) { return bpe_encode_words(env, info, true); }

// document offsets as a Float64Array of non-negative integers (exact below 2^53), D + 1 >= 1 entries
bool get_doc_offsets(napi_env env, napi_value v, std::vector<uint64_t>* out) {
    bool is_ta = false;
    napi_typedarray_type type = napi_uint8_array;
    size_t n = 0, off = 0;
    void* raw = nullptr;
    napi_value ab;
    if (napi_is_typedarray(env, v, &is_ta) != napi_ok || !is_ta ||
        napi_get_typedarray_info(env, v, &type, &n, &raw, &ab, &off) != napi_ok || type != napi_float64_array || n < 1)
        return false;
    const double* d = static_cast<const double*>(raw);
    out->resize(n);
    for (size_t i = 0; i < n; ++i) {
        if (!(d[i] >= 0 && d[i] <= 9007199254740992.0) || d[i] != (double)(uint64_t)d[i]) return false;
        (*out)[i] = (uint64_t)d[i];
    }
    return true;
}

napi_value make_f64_array(napi_env env, const std::vector<uint64_t>& v) {
    napi_value ab, ta;
    void* dst = nullptr;
    NAPI_CALL(env, napi_create_arraybuffer(env, v.size() * 8, &dst, &ab));
    for (size_t i = 0; i < v.size(); ++i) static_cast<double*>(dst)[i] = (double)v[i];
    NAPI_CALL(env, napi_create_typedarray(env, napi_float64_array, v.size(), ab, 0, &ta));
    return ta;
}

// bpeEncodeWordsBatch(ctx, bpe, bytes, offsets, wordStarts | null, mode) -> { tokens, offsets }: many
// documents in one call (gbpe_bpe_encode_words_batch), each encoded as bpeEncodeWords encodes it alone
// (`special`: bpeEncodeSpecialBatch, the same with a special table after bpe — gbpe_bpe_encode_special_batch)
napi_value bpe_encode_words_batch(napi_env env, napi_callback_info info, bool special) {
    const size_t o = special ? 1 : 0;
    size_t argc = 7;
    napi_value argv[7];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc >= 1 ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    Bpe* b = argc >= 2 ? unwrap_external<Bpe>(env, argv[1]) : nullptr;
    Specials* sp = special && argc >= 3 ? unwrap_external<Specials>(env, argv[2]) : nullptr;
    const uint8_t *data = nullptr, *ws = nullptr;
    size_t len = 0, ws_len = 0;
    uint32_t mode = 0;
    std::vector<uint64_t> doc_off;
    bool ok = ctx_usable(c) && b && b->bpe && (!special || (sp && sp->sp)) && argc >= 6 + o &&
              get_bytes(env, argv[2 + o], &data, &len) && get_doc_offsets(env, argv[3 + o], &doc_off) &&
              napi_get_value_uint32(env, argv[5 + o], &mode) == napi_ok;
    bool has_ws = false;
    if (ok) {
        napi_valuetype vt;
        ok = napi_typeof(env, argv[4 + o], &vt) == napi_ok;
        has_ws = ok && vt != napi_null && vt != napi_undefined;
        if (has_ws) ok = get_bytes(env, argv[4 + o], &ws, &ws_len) && ws_len == len;
    }
    if (!ok) {
        napi_throw_type_error(env, nullptr,
                              special ? "bpeEncodeSpecialBatch(ctx, bpe, specials, Uint8Array, offsets: Float64Array of "
                                        "non-negative integers, wordStarts: Uint8Array of the same length | null, mode)"
                                      : "bpeEncodeWordsBatch(ctx, bpe, Uint8Array, offsets: Float64Array of non-negative "
                                        "integers, wordStarts: Uint8Array of the same length | null, mode)");
        return nullptr;
    }
    static const uint8_t kNoByte = 0;
    if (has_ws && !ws) ws = &kNoByte;   // (an empty mask still goes with mode 1)
    std::vector<uint32_t> out(len ? len : 1);
    std::vector<uint64_t> tok_off(doc_off.size(), 0);
    uint64_t n = 0;
    std::unique_lock<std::mutex> g(c->mu);
    const uint8_t* m = has_ws ? ws : nullptr;
    int rc = special ? gbpe_bpe_encode_special_batch(c->ctx, b->bpe, sp->sp, data, len, doc_off.data(), doc_off.size() - 1, m,
                                                     mode, out.data(), out.size(), tok_off.data(), &n)
                     : gbpe_bpe_encode_words_batch(c->ctx, b->bpe, data, len, doc_off.data(), doc_off.size() - 1, m, mode,
                                                   out.data(), out.size(), tok_off.data(), &n);
    g.unlock();
    if (rc != GBPE_OK) return throw_status(env, c->ctx, special ? "bpe encode batch (special)" : "bpe encode batch", rc);
    napi_value obj;
    NAPI_CALL(env, napi_create_object(env, &obj));
    NAPI_CALL(env, napi_set_named_property(env, obj, "tokens", make_u32_array(env, out.data(), (size_t)n)));
    NAPI_CALL(env, napi_set_named_property(env, obj, "offsets", make_f64_array(env, tok_off)));
    return obj;
}
napi_value BpeEncodeWordsBatch(napi_env env, napi_callback_info info) { return bpe_encode_words_batch(env, info, false); }
napi_value BpeEncodeSpecialBatch(napi_env env, napi_callback_info info) { return bpe_encode_words_batch(env, info, true); }

// bpeEncodeSpans(ctx, bpe, specials | null, bytes, offsets | null, wordStarts | null, mode) ->
// { tokens, starts[, offsets] }: gbpe_bpe_encode_spans, the most general encode call with the first byte of
// every token.  starts is a Float64Array of tokens.length + 1 entries, the input's length at the end;
// offsets (the documents' token offsets) is there when offsets were given.
napi_value BpeEncodeSpans(napi_env env, napi_callback_info info) {
    size_t argc = 7;
    napi_value argv[7];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc >= 1 ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    Bpe* b = argc >= 2 ? unwrap_external<Bpe>(env, argv[1]) : nullptr;
    const uint8_t *data = nullptr, *ws = nullptr;
    size_t len = 0, ws_len = 0;
    uint32_t mode = 0;
    std::vector<uint64_t> doc_off;
    Specials* sp = nullptr;
    bool has_sp = false, has_off = false, has_ws = false;
    bool ok = ctx_usable(c) && b && b->bpe && argc >= 7 && get_bytes(env, argv[3], &data, &len) &&
              napi_get_value_uint32(env, argv[6], &mode) == napi_ok;
    auto given = [&](napi_value v, bool* has) {
        napi_valuetype vt;
        if (napi_typeof(env, v, &vt) != napi_ok) return false;
        *has = vt != napi_null && vt != napi_undefined;
        return true;
    };
    if (ok) ok = given(argv[2], &has_sp) && given(argv[4], &has_off) && given(argv[5], &has_ws);
    if (ok && has_sp) {
        sp = unwrap_external<Specials>(env, argv[2]);
        ok = sp && sp->sp;
    }
    if (ok && has_off) ok = get_doc_offsets(env, argv[4], &doc_off);
    if (ok && has_ws) ok = get_bytes(env, argv[5], &ws, &ws_len) && ws_len == len;
    if (!ok) {
        napi_throw_type_error(env, nullptr,
                              "bpeEncodeSpans(ctx, bpe, specials | null, Uint8Array, offsets: Float64Array of non-negative "
                              "integers | null, wordStarts: Uint8Array of the same length | null, mode)");
        return nullptr;
    }
    static const uint8_t kNoByte = 0;
    if (has_ws && !ws) ws = &kNoByte;   // (an empty mask still goes with mode 1)
    std::vector<uint32_t> out(len ? len : 1);
    std::vector<uint64_t> starts(out.size() + 1);
    std::vector<uint64_t> tok_off(doc_off.size(), 0);
    uint64_t n = 0;
    std::unique_lock<std::mutex> g(c->mu);
    int rc = gbpe_bpe_encode_spans(c->ctx, b->bpe, has_sp ? sp->sp : nullptr, data, len, has_off ? doc_off.data() : nullptr,
                                   has_off ? doc_off.size() - 1 : 0, has_ws ? ws : nullptr, mode, out.data(), starts.data(),
                                   out.size(), has_off ? tok_off.data() : nullptr, &n);
    g.unlock();
    if (rc != GBPE_OK) return throw_status(env, c->ctx, "bpe encode (spans)", rc);
    starts.resize((size_t)n + 1);
    starts[(size_t)n] = len;
    napi_value obj;
    NAPI_CALL(env, napi_create_object(env, &obj));
    NAPI_CALL(env, napi_set_named_property(env, obj, "tokens", make_u32_array(env, out.data(), (size_t)n)));
    NAPI_CALL(env, napi_set_named_property(env, obj, "starts", make_f64_array(env, starts)));
    if (has_off) NAPI_CALL(env, napi_set_named_property(env, obj, "offsets", make_f64_array(env, tok_off)));
    return obj;
}

// specialsUpload(ctx, bytes: Uint8Array, offsets: Float64Array, ids: Uint32Array) -> external: special i is
// bytes[offsets[i], offsets[i + 1]) with id ids[i] (gbpe_specials_upload)
napi_value SpecialsUpload(napi_env env, napi_callback_info info) {
    size_t argc = 4;
    napi_value argv[4];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc >= 1 ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    const uint8_t* data = nullptr;
    const uint32_t* ids = nullptr;
    size_t len = 0, n_ids = 0;
    std::vector<uint64_t> offs;
    static const uint8_t kNoByte = 0;
    if (!ctx_usable(c) || argc < 4 || !get_bytes(env, argv[1], &data, &len) || !get_doc_offsets(env, argv[2], &offs) ||
        !get_u32s(env, argv[3], &ids, &n_ids) || n_ids + 1 != offs.size() || offs.back() > len) {
        napi_throw_type_error(env, nullptr, "specialsUpload(ctx, Uint8Array, offsets: Float64Array, ids: Uint32Array)");
        return nullptr;
    }
    for (size_t i = 0; i + 1 < offs.size(); ++i) {
        if (offs[i + 1] < offs[i]) {
            napi_throw_type_error(env, nullptr, "specialsUpload: offsets decrease");
            return nullptr;
        }
    }
    auto* s = new Specials();
    const uint32_t no_id = 0;
    std::unique_lock<std::mutex> g(c->mu);
    int rc = gbpe_specials_upload(c->ctx, data ? data : &kNoByte, offs.data(), ids ? ids : &no_id, (uint32_t)n_ids, &s->sp);
    g.unlock();
    if (rc != GBPE_OK) {
        delete s;
        return throw_status(env, c->ctx, "specials upload", rc);
    }
    s->owner = c;
    ++c->refs;
    napi_value ext;
    NAPI_CALL(env, napi_create_external(env, s, specials_finalize, nullptr, &ext));
    return ext;
}

// specialsMark(ctx, specials, bytes, offsets | null) -> Uint8Array: 0 / 1 + index / 255 per byte (gbpe_specials_mark)
napi_value SpecialsMark(napi_env env, napi_callback_info info) {
    size_t argc = 4;
    napi_value argv[4];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc >= 1 ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    Specials* sp = argc >= 2 ? unwrap_external<Specials>(env, argv[1]) : nullptr;
    const uint8_t* data = nullptr;
    size_t len = 0;
    std::vector<uint64_t> doc_off;
    bool ok = ctx_usable(c) && sp && sp->sp && argc >= 3 && get_bytes(env, argv[2], &data, &len);
    bool has_off = false;
    if (ok && argc >= 4) {
        napi_valuetype vt;
        ok = napi_typeof(env, argv[3], &vt) == napi_ok;
        has_off = ok && vt != napi_null && vt != napi_undefined;
        if (has_off) ok = get_doc_offsets(env, argv[3], &doc_off);
    }
    if (!ok) {
        napi_throw_type_error(env, nullptr,
                              "specialsMark(ctx, specials, Uint8Array, offsets: Float64Array of non-negative integers | null)");
        return nullptr;
    }
    napi_value ab, ta;
    void* dst = nullptr;
    NAPI_CALL(env, napi_create_arraybuffer(env, len, &dst, &ab));
    if (len) memset(dst, 0, len);
    std::unique_lock<std::mutex> g(c->mu);
    int rc = gbpe_specials_mark(c->ctx, sp->sp, data, len, has_off ? doc_off.data() : nullptr,
                                has_off ? doc_off.size() - 1 : 0, static_cast<uint8_t*>(dst));
    g.unlock();
    if (rc != GBPE_OK) return throw_status(env, c->ctx, "specialsMark", rc);
    NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, len, ab, 0, &ta));
    return ta;
}

// pretokenizeGpt4Batch(ctx, bytes, offsets) -> Uint8Array: each document's own GPT-4 word starts
// (gbpe_pretokenize_gpt4_batch); pretokenizeCl100kBatch: its own cl100k_base ones (gbpe_pretokenize_cl100k_batch);
// pretokenizeO200kBatch: its own o200k_base ones (gbpe_pretokenize_o200k_batch)
static napi_value pretokenize_batch(napi_env env, napi_callback_info info, int rules) {
    static const char* const names[3] = {"pretokenizeGpt4Batch", "pretokenizeCl100kBatch", "pretokenizeO200kBatch"};
    static const char* const usage[3] = {
        "pretokenizeGpt4Batch(ctx, Uint8Array, offsets: Float64Array of non-negative integers)",
        "pretokenizeCl100kBatch(ctx, Uint8Array, offsets: Float64Array of non-negative integers)",
        "pretokenizeO200kBatch(ctx, Uint8Array, offsets: Float64Array of non-negative integers)"};
    const char* name = names[rules];
    size_t argc = 3;
    napi_value argv[3];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc >= 1 ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    const uint8_t* data = nullptr;
    size_t len = 0;
    std::vector<uint64_t> doc_off;
    if (!ctx_usable(c) || argc < 3 || !get_bytes(env, argv[1], &data, &len) || !get_doc_offsets(env, argv[2], &doc_off)) {
        napi_throw_type_error(env, nullptr, usage[rules]);
        return nullptr;
    }
    napi_value ab, ta;
    void* dst = nullptr;
    NAPI_CALL(env, napi_create_arraybuffer(env, len, &dst, &ab));
    std::unique_lock<std::mutex> g(c->mu);
    int rc = (rules == 2 ? gbpe_pretokenize_o200k_batch : rules == 1 ? gbpe_pretokenize_cl100k_batch : gbpe_pretokenize_gpt4_batch)(
        c->ctx, data, len, doc_off.data(), doc_off.size() - 1, static_cast<uint8_t*>(dst));
    g.unlock();
    if (rc != GBPE_OK) return throw_status(env, c->ctx, name, rc);
    NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, len, ab, 0, &ta));
    return ta;
}
napi_value PretokenizeGpt4Batch(napi_env env, napi_callback_info info) { return pretokenize_batch(env, info, 0); }
napi_value PretokenizeCl100kBatch(napi_env env, napi_callback_info info) { return pretokenize_batch(env, info, 1); }
napi_value PretokenizeO200kBatch(napi_env env, napi_callback_info info) { return pretokenize_batch(env, info, 2); }

struct EncodeWork {
    napi_async_work work = nullptr;
    napi_deferred deferred = nullptr;
    napi_ref keep_in = nullptr, keep_ctx = nullptr, keep_trie = nullptr;
    Ctx* c = nullptr;
    Trie* trie = nullptr;
    const uint8_t* data = nullptr;
    size_t len = 0;
    uint32_t cs = 0;
    std::vector<uint32_t> out;
    uint64_t n_out = 0;
    int rc = GBPE_OK;
    std::string err;
};

void encode_execute(napi_env, void* data) {
    auto* w = static_cast<EncodeWork*>(data);
    w->out.resize(w->len ? w->len : 1);
    std::lock_guard<std::mutex> g(w->c->mu);
    w->rc = gbpe_encode(w->c->ctx, w->trie->trie, w->data, w->len, w->cs, w->out.data(), w->len, &w->n_out);
    if (w->rc != GBPE_OK) w->err = last_error(w->c->ctx, "encode", w->rc);
}

void encode_complete(napi_env env, napi_status, void* data) {
    auto* w = static_cast<EncodeWork*>(data);
    if (w->rc != GBPE_OK) {
        napi_value msg, err;
        napi_create_string_utf8(env, w->err.c_str(), NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, nullptr, msg, &err);
        napi_reject_deferred(env, w->deferred, err);
    } else {
        napi_resolve_deferred(env, w->deferred, make_u32_array(env, w->out.data(), (size_t)w->n_out));
    }
    if (--w->trie->inflight == 0 && w->trie->destroy_pending) trie_free(w->trie);
    ctx_release(w->c);
    napi_delete_reference(env, w->keep_in);
    napi_delete_reference(env, w->keep_ctx);
    napi_delete_reference(env, w->keep_trie);
    napi_delete_async_work(env, w->work);
    delete w;
}

napi_value Encode(napi_env env, napi_callback_info info) {
    size_t argc = 4;
    napi_value argv[4];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc >= 1 ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    Trie* tr = argc >= 2 ? unwrap_external<Trie>(env, argv[1]) : nullptr;
    const uint8_t* data = nullptr;
    size_t len = 0;
    if (!ctx_usable(c) || !tr || !tr->trie || tr->destroy_pending || argc < 4 || !get_bytes(env, argv[2], &data, &len)) {
        napi_throw_type_error(env, nullptr, "encode(ctx, trie, Uint8Array, chunkSize)");
        return nullptr;
    }
    auto* w = new EncodeWork();
    w->c = c;
    ++c->refs;        // released by encode_complete
    w->trie = tr;
    ++tr->inflight;
    w->data = data;
    w->len = len;
    napi_get_value_uint32(env, argv[3], &w->cs);
    napi_value promise, name;
    NAPI_CALL(env, napi_create_promise(env, &w->deferred, &promise));
    NAPI_CALL(env, napi_create_reference(env, argv[2], 1, &w->keep_in));
    NAPI_CALL(env, napi_create_reference(env, argv[0], 1, &w->keep_ctx));
    NAPI_CALL(env, napi_create_reference(env, argv[1], 1, &w->keep_trie));
    NAPI_CALL(env, napi_create_string_utf8(env, "gpubpe.encode", NAPI_AUTO_LENGTH, &name));
    NAPI_CALL(env, napi_create_async_work(env, nullptr, name, encode_execute, encode_complete, w, &w->work));
    NAPI_CALL(env, napi_queue_async_work(env, w->work));
    return promise;
}

// encodeBatch: many documents in one call (gbpe_encode_batch; an addition to the
// reference's API).  Offsets cross the boundary as Float64Array (exact below 2^53).
struct EncodeBatchWork {
    napi_async_work work = nullptr;
    napi_deferred deferred = nullptr;
    napi_ref keep_in = nullptr, keep_ctx = nullptr, keep_trie = nullptr;
    Ctx* c = nullptr;
    Trie* trie = nullptr;
    const uint8_t* data = nullptr;
    size_t len = 0;
    uint32_t cs = 0;
    std::vector<uint64_t> doc_off, tok_off;   // (the offsets are copied on the JS thread)
    std::vector<uint32_t> out;
    uint64_t n_out = 0;
    int rc = GBPE_OK;
    std::string err;
};

void encode_batch_execute(napi_env, void* data) {
    auto* w = static_cast<EncodeBatchWork*>(data);
    w->out.resize(w->len ? w->len : 1);
    w->tok_off.assign(w->doc_off.size(), 0);
    std::lock_guard<std::mutex> g(w->c->mu);
    w->rc = gbpe_encode_batch(w->c->ctx, w->trie->trie, w->data, w->len, w->doc_off.data(), w->doc_off.size() - 1, w->cs,
                              w->out.data(), w->len, w->tok_off.data(), &w->n_out);
    if (w->rc != GBPE_OK) w->err = last_error(w->c->ctx, "encode batch", w->rc);
}

void encode_batch_complete(napi_env env, napi_status, void* data) {
    auto* w = static_cast<EncodeBatchWork*>(data);
    if (w->rc != GBPE_OK) {
        napi_value msg, err;
        napi_create_string_utf8(env, w->err.c_str(), NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, nullptr, msg, &err);
        napi_reject_deferred(env, w->deferred, err);
    } else {
        napi_value obj, ab, offs;
        void* dst = nullptr;
        napi_create_object(env, &obj);
        napi_set_named_property(env, obj, "tokens", make_u32_array(env, w->out.data(), (size_t)w->n_out));
        const size_t no = w->tok_off.size();
        napi_create_arraybuffer(env, no * 8, &dst, &ab);
        for (size_t i = 0; i < no; ++i) static_cast<double*>(dst)[i] = (double)w->tok_off[i];
        napi_create_typedarray(env, napi_float64_array, no, ab, 0, &offs);
        napi_set_named_property(env, obj, "offsets", offs);
        napi_resolve_deferred(env, w->deferred, obj);
    }
    if (--w->trie->inflight == 0 && w->trie->destroy_pending) trie_free(w->trie);
    ctx_release(w->c);
    napi_delete_reference(env, w->keep_in);
    napi_delete_reference(env, w->keep_ctx);
    napi_delete_reference(env, w->keep_trie);
    napi_delete_async_work(env, w->work);
    delete w;
}

napi_value EncodeBatch(napi_env env, napi_callback_info info) {
    size_t argc = 5;
    napi_value argv[5];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc >= 1 ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    Trie* tr = argc >= 2 ? unwrap_external<Trie>(env, argv[1]) : nullptr;
    const uint8_t* data = nullptr;
    size_t len = 0, noff = 0, ooff = 0;
    bool ok = ctx_usable(c) && tr && tr->trie && !tr->destroy_pending && argc >= 5 && get_bytes(env, argv[2], &data, &len);
    napi_typedarray_type type = napi_uint8_array;
    void* raw = nullptr;
    napi_value oab;
    bool is_ta = false;
    if (ok) napi_is_typedarray(env, argv[3], &is_ta);
    ok = ok && is_ta && napi_get_typedarray_info(env, argv[3], &type, &noff, &raw, &oab, &ooff) == napi_ok &&
         type == napi_float64_array && noff >= 1;
    if (!ok) {
        napi_throw_type_error(env, nullptr, "encodeBatch(ctx, trie, Uint8Array, offsets: Float64Array, chunkSize)");
        return nullptr;
    }
    const double* offs = static_cast<const double*>(raw);
    for (size_t i = 0; i < noff; ++i) {
        if (!(offs[i] >= 0 && offs[i] <= 9007199254740992.0) || offs[i] != (double)(uint64_t)offs[i]) {
            napi_throw_range_error(env, nullptr, "encodeBatch: offsets must be non-negative integers");
            return nullptr;
        }
    }
    auto* w = new EncodeBatchWork();
    w->doc_off.resize(noff);
    for (size_t i = 0; i < noff; ++i) w->doc_off[i] = (uint64_t)offs[i];
    w->c = c;
    ++c->refs;        // released by encode_batch_complete
    w->trie = tr;
    ++tr->inflight;
    w->data = data;
    w->len = len;
    napi_get_value_uint32(env, argv[4], &w->cs);
    napi_value promise, name;
    NAPI_CALL(env, napi_create_promise(env, &w->deferred, &promise));
    NAPI_CALL(env, napi_create_reference(env, argv[2], 1, &w->keep_in));
    NAPI_CALL(env, napi_create_reference(env, argv[0], 1, &w->keep_ctx));
    NAPI_CALL(env, napi_create_reference(env, argv[1], 1, &w->keep_trie));
    NAPI_CALL(env, napi_create_string_utf8(env, "gpubpe.encodeBatch", NAPI_AUTO_LENGTH, &name));
    NAPI_CALL(env, napi_create_async_work(env, nullptr, name, encode_batch_execute, encode_batch_complete, w, &w->work));
    NAPI_CALL(env, napi_queue_async_work(env, w->work));
    return promise;
}

// ── device vocab + decode (gbpe_vocab_upload, gbpe_decode, gbpe_decode_batch; an
//    addition to the reference's API, whose decode is a host loop) ────────────
struct DVocab {
    gbpe_vocab* vocab = nullptr;
    Ctx* owner = nullptr;
    std::vector<uint64_t> offsets;   // host copy: gbpe_decode_size sizes every output exactly
    int inflight = 0;
    bool destroy_pending = false;
};
void dvocab_free(DVocab* v) {
    if (v->vocab) {
        std::lock_guard<std::mutex> g(v->owner->mu);
        gbpe_vocab_free(v->vocab);
        v->vocab = nullptr;
    }
    if (v->owner) {
        ctx_release(v->owner);
        v->owner = nullptr;
    }
}
void dvocab_finalize(napi_env, void* data, void*) {
    DVocab* v = static_cast<DVocab*>(data);
    dvocab_free(v);
    delete v;
}

// offsets cross the boundary as Float64Array (exact below 2^53); false: not one, or not non-negative integers
bool get_offsets(napi_env env, napi_value v, std::vector<uint64_t>* out) {
    bool is_ta = false;
    napi_is_typedarray(env, v, &is_ta);
    if (!is_ta) return false;
    napi_typedarray_type type;
    size_t length = 0, offset = 0;
    void* raw = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, v, &type, &length, &raw, &ab, &offset) != napi_ok) return false;
    if (type != napi_float64_array || length < 1) return false;
    const double* offs = static_cast<const double*>(raw);
    out->resize(length);
    for (size_t i = 0; i < length; ++i) {
        if (!(offs[i] >= 0 && offs[i] <= 9007199254740992.0) || offs[i] != (double)(uint64_t)offs[i]) return false;
        (*out)[i] = (uint64_t)offs[i];
    }
    return true;
}

napi_value VocabUpload(napi_env env, napi_callback_info info) {
    size_t argc = 3;
    napi_value argv[3];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc >= 1 ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    const uint8_t* bytes = nullptr;
    size_t nb = 0;
    auto* v = new DVocab();
    if (!ctx_usable(c) || argc < 3 || !get_bytes(env, argv[1], &bytes, &nb) || !get_offsets(env, argv[2], &v->offsets) ||
        v->offsets.size() - 1 > 0xFFFFFFFEull || v->offsets.back() > nb) {
        delete v;
        napi_throw_type_error(env, nullptr, "vocabUpload(ctx, bytes: Uint8Array, offsets: Float64Array of V + 1 entries within bytes)");
        return nullptr;
    }
    std::unique_lock<std::mutex> g(c->mu);
    const int rc = gbpe_vocab_upload(c->ctx, bytes, v->offsets.data(), (uint32_t)(v->offsets.size() - 1), &v->vocab);
    g.unlock();
    if (rc != GBPE_OK) {
        delete v;
        return throw_status(env, c->ctx, "vocab upload", rc);
    }
    v->owner = c;
    ++c->refs;
    napi_value ext;
    NAPI_CALL(env, napi_create_external(env, v, dvocab_finalize, nullptr, &ext));
    return ext;
}

napi_value VocabFree(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value argv[1];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    DVocab* v = argc ? unwrap_external<DVocab>(env, argv[0]) : nullptr;
    if (v && v->vocab) {
        if (v->inflight) v->destroy_pending = true;   // decode_complete frees it
        else dvocab_free(v);
    }
    return nullptr;
}

struct DecodeWork {   // decode and decodeBatch (batch: tok_off has D + 1 entries)
    napi_async_work work = nullptr;
    napi_deferred deferred = nullptr;
    napi_ref keep_in = nullptr, keep_ctx = nullptr, keep_vocab = nullptr;
    Ctx* c = nullptr;
    DVocab* vocab = nullptr;
    const uint32_t* tokens = nullptr;
    size_t n = 0;
    bool batch = false;
    std::vector<uint64_t> tok_off, byte_off;   // (the offsets are copied on the JS thread)
    std::vector<uint8_t> out;
    uint64_t n_out = 0;
    int rc = GBPE_OK;
    std::string err;
};

void decode_execute(napi_env, void* data) {
    auto* w = static_cast<DecodeWork*>(data);
    uint64_t size = 0;
    w->rc = gbpe_decode_size(w->vocab->offsets.data(), (uint32_t)(w->vocab->offsets.size() - 1), w->tokens, w->n, &size);
    if (w->rc != GBPE_OK) {
        w->err = last_error(nullptr, "decode size", w->rc);
        return;
    }
    w->out.resize(size ? size : 1);
    std::lock_guard<std::mutex> g(w->c->mu);
    if (w->batch) {
        w->byte_off.assign(w->tok_off.size(), 0);
        w->rc = gbpe_decode_batch(w->c->ctx, w->vocab->vocab, w->tokens, w->n, w->tok_off.data(), w->tok_off.size() - 1,
                                  w->out.data(), size, w->byte_off.data(), &w->n_out);
    } else {
        w->rc = gbpe_decode(w->c->ctx, w->vocab->vocab, w->tokens, w->n, w->out.data(), size, &w->n_out);
    }
    if (w->rc != GBPE_OK) w->err = last_error(w->c->ctx, w->batch ? "decode batch" : "decode", w->rc);
}

napi_value make_u8_array(napi_env env, const uint8_t* src, size_t n) {
    napi_value ab, ta;
    void* dst = nullptr;
    if (napi_create_arraybuffer(env, n, &dst, &ab) != napi_ok) return nullptr;
    if (n) memcpy(dst, src, n);
    if (napi_create_typedarray(env, napi_uint8_array, n, ab, 0, &ta) != napi_ok) return nullptr;
    return ta;
}

void decode_complete(napi_env env, napi_status, void* data) {
    auto* w = static_cast<DecodeWork*>(data);
    if (w->rc != GBPE_OK) {
        napi_value msg, err;
        napi_create_string_utf8(env, w->err.c_str(), NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, nullptr, msg, &err);
        napi_reject_deferred(env, w->deferred, err);
    } else if (!w->batch) {
        napi_resolve_deferred(env, w->deferred, make_u8_array(env, w->out.data(), (size_t)w->n_out));
    } else {
        napi_value obj, ab, offs;
        void* dst = nullptr;
        napi_create_object(env, &obj);
        napi_set_named_property(env, obj, "bytes", make_u8_array(env, w->out.data(), (size_t)w->n_out));
        const size_t no = w->byte_off.size();
        napi_create_arraybuffer(env, no * 8, &dst, &ab);
        for (size_t i = 0; i < no; ++i) static_cast<double*>(dst)[i] = (double)w->byte_off[i];
        napi_create_typedarray(env, napi_float64_array, no, ab, 0, &offs);
        napi_set_named_property(env, obj, "offsets", offs);
        napi_resolve_deferred(env, w->deferred, obj);
    }
    if (--w->vocab->inflight == 0 && w->vocab->destroy_pending) dvocab_free(w->vocab);
    ctx_release(w->c);
    napi_delete_reference(env, w->keep_in);
    napi_delete_reference(env, w->keep_ctx);
    napi_delete_reference(env, w->keep_vocab);
    napi_delete_async_work(env, w->work);
    delete w;
}

napi_value decode_queue(napi_env env, napi_callback_info info, bool batch) {
    size_t argc = 4;
    napi_value argv[4];
    NAPI_CALL(env, napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
    Ctx* c = argc >= 1 ? unwrap_external<Ctx>(env, argv[0]) : nullptr;
    DVocab* v = argc >= 2 ? unwrap_external<DVocab>(env, argv[1]) : nullptr;
    const uint32_t* tokens = nullptr;
    size_t n = 0;
    std::vector<uint64_t> tok_off;
    if (!ctx_usable(c) || !v || !v->vocab || v->destroy_pending || argc < (batch ? 4u : 3u) ||
        !get_u32s(env, argv[2], &tokens, &n) || (batch && !get_offsets(env, argv[3], &tok_off))) {
        napi_throw_type_error(env, nullptr, batch ? "decodeBatch(ctx, vocab, Uint32Array, offsets: Float64Array of non-negative integers)"
                                                  : "decode(ctx, vocab, Uint32Array)");
        return nullptr;
    }
    auto* w = new DecodeWork();
    w->c = c;
    ++c->refs;        // released by decode_complete
    w->vocab = v;
    ++v->inflight;
    w->tokens = tokens;
    w->n = n;
    w->batch = batch;
    w->tok_off = std::move(tok_off);
    napi_value promise, name;
    NAPI_CALL(env, napi_create_promise(env, &w->deferred, &promise));
    NAPI_CALL(env, napi_create_reference(env, argv[2], 1, &w->keep_in));
    NAPI_CALL(env, napi_create_reference(env, argv[0], 1, &w->keep_ctx));
    NAPI_CALL(env, napi_create_reference(env, argv[1], 1, &w->keep_vocab));
    NAPI_CALL(env, napi_create_string_utf8(env, batch ? "gpubpe.decodeBatch" : "gpubpe.decode", NAPI_AUTO_LENGTH, &name));
    NAPI_CALL(env, napi_create_async_work(env, nullptr, name, decode_execute, decode_complete, w, &w->work));
    NAPI_CALL(env, napi_queue_async_work(env, w->work));
    return promise;
}

napi_value Decode(napi_env env, napi_callback_info info) { return decode_queue(env, info, false); }
napi_value DecodeBatch(napi_env env, napi_callback_info info) { return decode_queue(env, info, true); }

napi_value Init(napi_env env, napi_value exports) {
    napi_property_descriptor props[] = {
        {"createContext", nullptr, CreateContext, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"destroyContext", nullptr, DestroyContext, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"limits", nullptr, Limits, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"kernelNames", nullptr, KernelNames, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"wordBoundary", nullptr, WordBoundary, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"pretokenizeGpt4", nullptr, PretokenizeGpt4, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"trainerCreate", nullptr, TrainerCreate, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"trainerStep", nullptr, TrainerStep, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"trainerDestroy", nullptr, TrainerDestroy, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"trieUpload", nullptr, TrieUpload, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"bpeUpload", nullptr, BpeUpload, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"bpeUploadWide", nullptr, BpeUploadWide, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"bpeEncode", nullptr, BpeEncode, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"bpeEncodeWords", nullptr, BpeEncodeWords, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"trieFree", nullptr, TrieFree, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"encode", nullptr, Encode, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"encodeBatch", nullptr, EncodeBatch, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"bpeEncodeWordsBatch", nullptr, BpeEncodeWordsBatch, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"specialsUpload", nullptr, SpecialsUpload, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"specialsMark", nullptr, SpecialsMark, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"bpeEncodeSpecial", nullptr, BpeEncodeSpecial, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"bpeEncodeSpecialBatch", nullptr, BpeEncodeSpecialBatch, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"bpeEncodeSpans", nullptr, BpeEncodeSpans, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"pretokenizeGpt4Batch", nullptr, PretokenizeGpt4Batch, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"pretokenizeCl100k", nullptr, PretokenizeCl100k, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"pretokenizeCl100kBatch", nullptr, PretokenizeCl100kBatch, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"pretokenizeO200k", nullptr, PretokenizeO200k, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"pretokenizeO200kBatch", nullptr, PretokenizeO200kBatch, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"vocabUpload", nullptr, VocabUpload, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"vocabFree", nullptr, VocabFree, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"decode", nullptr, Decode, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"decodeBatch", nullptr, DecodeBatch, nullptr, nullptr, nullptr, napi_default, nullptr},
    };
    napi_define_properties(env, exports, sizeof(props) / sizeof(props[0]), props);
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
