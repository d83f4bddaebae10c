/*
 * gpubpe.h — C-ABI of the MI355X-native BPE train + trie-encode engine.
 *
 * This is the drop-in boundary for the reference's WebGPU device layer
 * (toprakdeviren/gpu-bpe: src/bpe/engine.js + the WGSL kernels in
 * src/bpe/train.wgsl and src/bpe/tokenizer/tokenize.wgsl).  A host binding
 * (the Node N-API addon in gpu-bpe_amd/js/, the Python ctypes binding in
 * gpu-bpe_amd/gpubpe/) wraps these entry points and keeps the reference's
 * JavaScript API (BPEEngine / BPETrainer / TrieTokenizer).
 *
 * Conventions
 *  - Plain C types only; no HIP or torch types cross the boundary.
 *  - Every function returns an int status (GBPE_OK = 0, negatives = errors);
 *    gbpe_last_error(ctx) returns a message for the last failure on ctx
 *    (ctx NULL: for the last failed gbpe_ctx_create).
 *  - The caller owns every host buffer; buffers are borrowed for the call
 *    and never retained.  The library owns and pools device memory.
 *  - A context is bound to one HIP device and one stream; it is not
 *    re-entrant (one thread at a time), like the reference's single queue.
 *  - Symbols in and out use the reference layout: u32, bits[15:0] = token
 *    id, bit 16 = word start (train.wgsl:36-37).
 */
#ifndef GPUBPE_H
#define GPUBPE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GBPE_ABI_VERSION 10  /* 10: many documents in one call for the word starts and the word-bounded encode
                                 (gbpe_pretokenize_gpt4_batch*, gbpe_bpe_encode_words_batch*);
                                 9: word-bounded merge-rank encode (gbpe_bpe_encode_words*, gbpe_bpe_encode_last_timing);
                                 8: device decode (gbpe_vocab_upload, gbpe_decode*, gbpe_decode_batch*);
                                 7: gbpe_encode_batch, gbpe_encode_batch_device (many documents in one call);
                                 6: pair_candidates, pair_rejected added at the end of the stats; 5: paired_merges
                                 added to the stats, gbpe_ctx_trim (round 6); 4: the late-loop stats removed,
                                 trainer creation time added (round 5) */

/* status codes */
#define GBPE_OK            0
#define GBPE_E_INVALID    -1   /* bad argument */
#define GBPE_E_OOM        -2   /* device or host allocation failed */
#define GBPE_E_DEVICE     -3   /* HIP runtime / kernel failure */
#define GBPE_E_CAPACITY   -4   /* output buffer too small; required size returned */
#define GBPE_E_CANCELLED  -5   /* progress callback returned non-zero */
#define GBPE_E_EMPTY      -6   /* empty corpus (trainer.js:161-163) */
#define GBPE_E_INTERNAL   -7   /* invariant violated (reported, never silent) */

/* reference constants (engine.js:10-13, training-pipeline.js:13) */
#define GBPE_WORKGROUP_SIZE   256u
#define GBPE_TABLE_SIZE       2097152u
#define GBPE_INVALID_TOKEN    0xFFFFFFFFu
#define GBPE_BATCH_SIZE       128u
#define GBPE_WORD_START_BIT   0x10000u

typedef struct gbpe_ctx gbpe_ctx;
typedef struct gbpe_trainer gbpe_trainer;
typedef struct gbpe_trie gbpe_trie;
typedef struct gbpe_vocab gbpe_vocab;

/* ── context / device (replaces engine.js:143-177 requestGPUDevice and
 *    engine.js:216-238 BPEEngine.init) ─────────────────────────────────── */
int  gbpe_ctx_create(int device_ordinal, gbpe_ctx** out);
void gbpe_ctx_destroy(gbpe_ctx* ctx);
/* Give the context's idle pooled device / pinned blocks back to the runtime (the
   pool keeps freed trainer buffers for the next trainer, tokenizer.js:30-46): for
   callers about to allocate outside the library (no reference counterpart). */
int gbpe_ctx_trim(gbpe_ctx* ctx);
/* engine.js:207-210 `limits.maxBufferSize` (used by tokenizer.js:181 for
 * multi-pass slicing).  This engine has no per-buffer cap below HBM size. */
int  gbpe_ctx_limits(gbpe_ctx* ctx, uint64_t* max_buffer_size);
const char* gbpe_last_error(const gbpe_ctx* ctx);
const char* gbpe_version(void);
/* GBPE_ABI_VERSION the library was built with, and sizeof(gbpe_trainer_stats) there:
 * a caller built against another header checks both before gbpe_trainer_stats_get */
int gbpe_abi_version(void);
uint64_t gbpe_trainer_stats_size(void);
/* number of compiled kernels (engine.js:234 logs Object.keys(pipelines).length) */
int  gbpe_kernel_count(void);
const char* gbpe_kernel_name(int i);

/* ── word boundaries (train.wgsl:144-186 bpe_word_boundary) ──────────────
 * ws_out[i] = 1 if byte i starts a word under the reference byte-class
 * heuristic. */
int gbpe_word_boundary(gbpe_ctx* ctx, const uint8_t* bytes, uint64_t n, uint8_t* ws_out);

/* PreTokenizer.preTokenizeBytes (src/wasm/pre_tokenizer.mjs:459-509) word-start
 * mask for NFC UTF-8 bytes (the reference also NFC-normalises: identity on NFC
 * input).  Classes: Unicode general categories (unicode_classes.h).
 * Domain: well-formed UTF-8 that may be cut short at its end — every byte
 * 0x80-0xBF is owned by the lead byte before it, by that lead's size (a cut
 * sequence decodes with its missing bytes read as 0, as in the reference; a
 * 4-byte sequence that decodes to 0x110000 or above has class Other).  A stray
 * continuation byte is outside the domain: the reference starts a 4-byte
 * codepoint at it, these kernels do not, and the result there is unspecified.
 * The _device form takes device pointers of any alignment, reads only
 * d_bytes[0, n) and writes only d_ws[0, n), on the context's stream. */
int gbpe_pretokenize_gpt4(gbpe_ctx* ctx, const uint8_t* bytes, uint64_t n, uint8_t* ws_out);
int gbpe_pretokenize_gpt4_device(gbpe_ctx* ctx, const void* d_bytes, uint64_t n, void* d_ws);
/* The same mask for many documents laid end to end (gbpe_encode_batch's
 * layout: doc_off has n_docs + 1 non-decreasing entries from 0 to n, empty documents
 * allowed): ws_out[doc_off[d] .. doc_off[d+1]) is exactly what gbpe_pretokenize_gpt4
 * gives for document d alone — the digit runs, the contraction look-arounds and a
 * sequence cut at a document's end never see the neighbouring document.  Each
 * document has that function's domain.  This is the word_starts gbpe_train takes for
 * a corpus of documents.  n == 0 or n_docs == 0: GBPE_OK, nothing launched.  Bad
 * offsets: GBPE_E_INVALID; the host form checks them before anything is launched.
 * The _device form takes d_bytes and d_ws of any alignment and d_doc_off (u64)
 * 8-byte aligned; its first kernel checks the offsets and bad ones return before
 * any other kernel runs, with d_ws untouched.  It returns after the kernels have
 * finished (the single-buffer _device form does not wait). */
int gbpe_pretokenize_gpt4_batch(gbpe_ctx* ctx, const uint8_t* bytes, uint64_t n, const uint64_t* doc_off,
                                uint64_t n_docs, uint8_t* ws_out);
int gbpe_pretokenize_gpt4_batch_device(gbpe_ctx* ctx, const void* d_bytes, uint64_t n, const void* d_doc_off,
                                       uint64_t n_docs, void* d_ws);

/* ── cl100k_base word starts ─────────────────────────────────
 * ws_out[i] = 1 at the first byte of every match of the split pattern that
 * cl100k_base, Llama 3 and their derivatives were trained with (tiktoken's, with
 * Rust-regex meaning), else 0:
 *   '(?i:[sdmt]|ll|ve|re)|[^\r\n\p{L}\p{N}]?+\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]++[\r\n]*|\s*[\r\n]|\s+(?!\S)|\s+
 * \p{L} is L* alone (a mark is not a letter), \p{N} is N*, \s is White_Space
 * (U+001C-U+001F are not), only U+0027 opens a contraction, and its letters fold
 * by simple case folding (U+017F is an s).  No normalisation.  The classes are
 * csrc/unicode_classes_cl100k.h's.  The domain, the arguments, the batch layout
 * and every status are those of the gbpe_pretokenize_gpt4 call of the same
 * suffix; a sequence that decodes to 0x110000 or above is "other". */
int gbpe_pretokenize_cl100k(gbpe_ctx* ctx, const uint8_t* bytes, uint64_t n, uint8_t* ws_out);
int gbpe_pretokenize_cl100k_device(gbpe_ctx* ctx, const void* d_bytes, uint64_t n, void* d_ws);
int gbpe_pretokenize_cl100k_batch(gbpe_ctx* ctx, const uint8_t* bytes, uint64_t n, const uint64_t* doc_off,
                                  uint64_t n_docs, uint8_t* ws_out);
int gbpe_pretokenize_cl100k_batch_device(gbpe_ctx* ctx, const void* d_bytes, uint64_t n, const void* d_doc_off,
                                         uint64_t n_docs, void* d_ws);

/* ── o200k_base word starts ──────────────────────────────────
 * The same for the split pattern that o200k_base and its derivatives were trained
 * with (tiktoken's, with Rust-regex meaning):
 *   [^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]*[\p{Ll}\p{Lm}\p{Lo}\p{M}]+(?i:'s|'t|'re|'ve|'m|'ll|'d)?
 *   |[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]+[\p{Ll}\p{Lm}\p{Lo}\p{M}]*(?i:'s|'t|'re|'ve|'m|'ll|'d)?
 *   |\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n/]*|\s*[\r\n]+|\s+(?!\S)|\s+
 * matched leftmost-first with backtracking (AXB is AX|B).  \s, [\r\n], the case
 * folding, the apostrophe, the domain, the arguments, the batch layout and every
 * status are gbpe_pretokenize_cl100k's; the classes are csrc/unicode_classes_o200k.h's. */
int gbpe_pretokenize_o200k(gbpe_ctx* ctx, const uint8_t* bytes, uint64_t n, uint8_t* ws_out);
int gbpe_pretokenize_o200k_device(gbpe_ctx* ctx, const void* d_bytes, uint64_t n, void* d_ws);
int gbpe_pretokenize_o200k_batch(gbpe_ctx* ctx, const uint8_t* bytes, uint64_t n, const uint64_t* doc_off,
                                 uint64_t n_docs, uint8_t* ws_out);
int gbpe_pretokenize_o200k_batch_device(gbpe_ctx* ctx, const void* d_bytes, uint64_t n, const void* d_doc_off,
                                        uint64_t n_docs, void* d_ws);

/* ── training (replaces trainer.js:149-335 BPETrainer.train over the
 *    train.wgsl kernels, training-pipeline.js:178-222 encodeBatch) ─────── */

/* Reproduce the reference's compaction exactly (default, 0) or use the
 * intended compaction.  The reference bounds bpe_finalize_compact_b with
 * the already-updated symbol count (train.wgsl:605-607, 698, 727) so the
 * last m slots of each compacted stream keep stale ping-pong contents. */
#define GBPE_TRAIN_EXACT_COMPACTION  (1u << 0)
/* record per-kernel device time with HIP events (read via gbpe_trainer_stats) */
#define GBPE_TRAIN_TIMING            (1u << 1)
/* word starts from the GPT-4 rules of the reference's PreTokenizer
 * (src/wasm/pre_tokenizer.mjs:226-292) computed on the device, for NFC UTF-8
 * input; ignored when word_starts is given */
#define GBPE_TRAIN_GPT4_BOUNDARIES   (1u << 2)
/* Sector-sparse merge loop.  Once the merge counts have fallen
 * far below the stream length, the stream is re-laid out as word-aligned
 * sectors with a token-presence bitmap: a merge then touches only the sectors
 * holding both of its tokens, plus a dense zone at the end of the stream that
 * carries the reference's compaction quirk.  On by default (same results as
 * the dense loop); DENSE_ONLY disables it, SPARSE_EARLY enters it at the first
 * step boundary where the zone fits (tests). */
#define GBPE_TRAIN_DENSE_ONLY        (1u << 3)
#define GBPE_TRAIN_SPARSE_EARLY      (1u << 4)

typedef struct gbpe_train_opts {
    uint32_t target_vocab_size;  /* trainer.js:149 targetVocabSize (reference default 4096) */
    uint32_t vocab_size;         /* Vocab.size before training (256 for a fresh Vocab) */
    uint32_t next_token_id;      /* Vocab.nextTokenId (trainer.js:191) */
    uint32_t batch_size;         /* merges per host round trip; 0 = 128 (training-pipeline.js:13) */
    uint32_t flags;              /* GBPE_TRAIN_* */
    uint32_t table_log2;         /* pair-table slots = 2^table_log2; 0 = automatic */
} gbpe_train_opts;

typedef struct gbpe_progress {   /* trainer.js:306-315 onProgress payload */
    uint32_t merge_index;        /* totalMergesDone */
    uint32_t total_merges;       /* mergesNeeded */
    uint32_t best_count;         /* count of the batch's last merge */
    uint32_t symbol_count;       /* current stream length */
    uint32_t batch_merges;       /* merges in this batch */
    uint32_t early_stop;
    double   elapsed_s;          /* since the loop started (trainer.js:230, 291) */
} gbpe_progress;

/* Called once per batch with that batch's merges as [a, b, id, count] x
 * batch_merges.  Return non-zero to cancel (gbpe_train returns
 * GBPE_E_CANCELLED, merges so far are kept). */
typedef int (*gbpe_progress_cb)(const gbpe_progress* p, const uint32_t* batch, void* user);

/* One-shot training from host bytes.  word_starts may be NULL (use the
 * heuristic kernel, trainer.js:177-180) or a byte mask (trainer.js:115-121).
 * merges_out receives [a, b, id, count] x n_merges (capacity merges_cap).
 * Returns GBPE_E_EMPTY for n == 0. */
int gbpe_train(gbpe_ctx* ctx, const uint8_t* bytes, uint64_t n, const uint8_t* word_starts,
               const gbpe_train_opts* opts, gbpe_progress_cb cb, void* user,
               uint32_t* merges_out, uint32_t merges_cap, uint32_t* n_merges, uint32_t* early_stop);

/* Stepwise trainer.  With input_on_device != 0, `bytes` (and `word_starts`)
 * are device pointers already resident in HBM (bench path). */
int gbpe_trainer_create(gbpe_ctx* ctx, const uint8_t* bytes, uint64_t n, const uint8_t* word_starts,
                        int input_on_device, const gbpe_train_opts* opts, gbpe_trainer** out);
/* Run up to max_merges merges (one host sync).  merges_out may be NULL. */
int gbpe_trainer_step(gbpe_trainer* t, uint32_t max_merges, uint32_t* merges_out,
                      uint32_t* n_done, uint32_t* early_stop);

typedef struct gbpe_trainer_stats {
    uint64_t symbol_count;        /* current stream length */
    uint64_t merges_done;         /* total merges so far */
    uint64_t stream_bytes_moved;  /* sum over merges of s*(2*N_i + N_{i+1}), s = bytes/symbol */
    uint64_t tail_dropped;        /* sum of m over merges (reference compaction quirk) */
    uint64_t live_pairs;          /* distinct pairs with count > 0 (last refresh) */
    uint64_t table_slots;
    uint64_t table_used;          /* occupied slots (incl. dead) */
    uint64_t max_live_pairs;      /* max over merges: > ~1.7M means the reference's 2^21
                                     table would likely have dropped counts (train.wgsl:422-429) */
    uint32_t bytes_per_symbol;
    uint32_t early_stop;
    double   ms_merge;            /* GBPE_TRAIN_TIMING: device ms in the two stream kernels (k_delta + k_compact) */
    double   ms_select;           /* k_select: argmax + merge setup */
    double   ms_other;            /* k_refresh: block maxima of touched table blocks */
    uint64_t timed_merges;
    double   ms_delta;            /* k_delta alone (HIP events between the two stream kernels) */
    double   ms_compact;          /* k_compact alone (tiles + stale-tail blocks) */
    uint64_t sparse_merges;       /* merges run by the sector-sparse loop */
    uint32_t sparse_enters;       /* dense -> sparse re-layouts */
    uint32_t sparse_exits;        /* sparse -> dense re-layouts (export, zone too small; a crowded table grows in place) */
    uint64_t sparse_sectors;      /* sectors of the last sparse layout */
    uint64_t sparse_zone;         /* zone length at the last sparse entry */
    uint64_t body_bytes;          /* bytes k_body actually moved: candidate extents + signature words, sector
                                     symbols read and rewritten, the single-workgroup zone pass (pair-table
                                     traffic excluded) */
    uint64_t zone_bytes;          /* bytes of the multi-tile zone passes (zone k_delta + k_compact + window copy) */
    uint64_t dense_bytes;         /* s*(2*N_i + N_{i+1}) summed over the dense merges only */
    double   ms_dense;            /* GBPE_TRAIN_TIMING: merge-pass device ms of the dense merges (k_delta + k_compact) */
    double   ms_sparse;           /* GBPE_TRAIN_TIMING: merge-pass device ms of the sparse merges (k_body + zone passes) */
    double   ms_body;             /* GBPE_TRAIN_TIMING: k_body alone */
    uint32_t lexicon_builds;      /* sparse entries whose body became a word lexicon */
    uint32_t lexicon_fallbacks;   /* ... that kept the in-place sectors (store not much smaller, collision) */
    uint64_t lexicon_words;       /* body word occurrences the lexicon represents (all builds and shrinks) */
    uint64_t lexicon_entries;     /* distinct-word entries of the current lexicon */
    uint64_t lexicon_symbols;     /* symbols of the current lexicon store (separators included) */
    double   ms_create;           /* host wall ms of trainer creation (symbols, word starts, first count):
                                     the part of a run the reference's t_loop excludes (trainer.js:230) */
    uint64_t paired_merges;       /* merges run as the second merge of a paired k_body launch */
    uint64_t pair_candidates;     /* launches whose top two pairs allowed a second merge */
    uint64_t pair_rejected;       /* ... whose second merge the zone workgroup's verdict turned down (reference
                                     compaction only; pair_candidates - pair_rejected == paired_merges) */
} gbpe_trainer_stats;
int gbpe_trainer_stats_get(gbpe_trainer* t, gbpe_trainer_stats* out);
/* Current symbol stream in the reference u32 layout (bit16 = word start). */
int gbpe_trainer_symbols(gbpe_trainer* t, uint32_t* out, uint64_t cap, uint64_t* n);
/* Live pair counts (count > 0): pids[i] = a<<16|b.  For parity tests. */
int gbpe_trainer_pair_counts(gbpe_trainer* t, uint32_t* pids, uint32_t* counts, uint64_t cap, uint64_t* n);
void gbpe_trainer_destroy(gbpe_trainer* t);

/* The library's HIP stream (the lexicon hand-over runs RCCL transfers on it). */
int gbpe_ctx_set_stream(gbpe_ctx* ctx, void* hip_stream);   /* taken literally (NULL = the null stream) */
void* gbpe_ctx_get_stream(gbpe_ctx* ctx);                    /* current stream (save / restore) */
/* ── checkpoint / resume: a run continues on another trainer ─────────────────
 * (The reference keeps no mid-run checkpoint)  The
 * state of a trainer is its current stream and its previous stream (the
 * ping-pong buffer the compaction quirk reads stale symbols from,
 * train.wgsl:605-607 + 698/727), both in the reference u32 layout (bit16 =
 * word start).  cur/prev NULL = lengths only; on_device != 0: cur/prev are
 * device pointers.
 * `prev` is defined only where the next merge's stale window can read it: after
 * the sector-sparse loop, positions below the body length at its last merge hold
 * the body as it was at entry, not the previous stream (the window always lies in
 * the stream's tail, so a resumed run reads the same symbols). */
int gbpe_trainer_export_state(gbpe_trainer* t, uint32_t* cur, uint64_t cap_cur, uint64_t* n_cur,
                              uint32_t* prev, uint64_t cap_prev, uint64_t* n_prev, int on_device);
/* A single-device trainer continuing from an exported state: opts as for
 * gbpe_trainer_create with vocab_size / next_token_id of the run so far (the
 * merges still to do are target_vocab_size - vocab_size); pair counts are
 * recounted from `cur`.  n_prev >= n (n_prev - n is the last merge's count;
 * n_prev == n for a run with no merges yet, whose prev is all zero). */
int gbpe_trainer_create_from_state(gbpe_ctx* ctx, const uint32_t* cur, uint64_t n, const uint32_t* prev,
                                   uint64_t n_prev, int input_on_device, const gbpe_train_opts* opts,
                                   gbpe_trainer** out);

/* ── sharded first pass + lexicon hand-over ─────────
 * The reference trains on one device (training-pipeline.js:178-222) and its merge
 * chain is sequential, so a multi-GPU run parallelises the first pass instead:
 * every rank turns ITS piece of the corpus (cut at a word start of the global
 * stream, the pieces concatenated in rank order are the corpus) into symbols, pair
 * counts and a word lexicon — its distinct words with their multiplicities — and ONE
 * root continues from all of them with the single-device sector-sparse loop
 * (DESIGN §2b/§2c).  The stream's tail — the last zt symbols, cut at a word start;
 * it may span several pieces — stays dense as the zone, where the reference
 * compaction quirk acts (train.wgsl:605-607 + 698/727).  The stream order
 * of the body stays on the ranks (their occurrence lists), so the stream may exceed
 * one device's 32-bit positions (C4: 8.6*10^9 symbols).  Protocol:
 *   rank:  lexshard_create → info_get: top_count, symbols → (sum of top counts: an upper
 *          bound of the first merge's count → zt; this piece's part of the last zt
 *          stream symbols) lexshard_build(part) → copy STORE + MUL + ZONE to the root
 *          → release
 *   root:  trainer_create_from_lexicon(stores in rank order, zones in rank order,
 *          body symbols)
 *          → map (a global word id per store entry, in rank order) → rank slices
 *          → lexshard_remap; gbpe_trainer_step as for any trainer
 *   check: gbpe_trainer_expand(root, every rank's OCC in rank order) = the stream. */
typedef struct gbpe_lexshard gbpe_lexshard;
typedef struct gbpe_lexshard_info {
    uint64_t symbols;        /* the piece's symbols */
    uint64_t body;           /* symbols before its zone (all of them on a rank without a zone) */
    uint64_t zone;           /* zone symbols (the ranks holding the stream's tail) */
    uint64_t store_symbols;  /* distinct words + one 0 separator each */
    uint64_t entries;        /* distinct words (words over 64 symbols: one entry per occurrence) */
    uint64_t words;          /* body words in stream order (the occurrence list) */
    uint32_t top_count;      /* the piece's largest pair count */
    uint32_t bytes_per_symbol;   /* STORE / ZONE layout: 2 = u16 (bit 15 word start), 4 = u32 (bit 16) */
} gbpe_lexshard_info;
#define GBPE_LEXSHARD_STORE 0   /* store_symbols x bytes_per_symbol */
#define GBPE_LEXSHARD_MUL   1   /* store_symbols x u32: each symbol's word multiplicity (0 at separators) */
#define GBPE_LEXSHARD_OCC   2   /* words x u32: word id (local; global after remap) or 0x80000000|symbol */
#define GBPE_LEXSHARD_ZONE  3   /* zone x bytes_per_symbol */
/* opts as for gbpe_trainer_create, identical on every rank and the root */
int  gbpe_lexshard_create(gbpe_ctx* ctx, const uint8_t* bytes, uint64_t n, const uint8_t* word_starts,
                          int input_on_device, const gbpe_train_opts* opts, gbpe_lexshard** out);
int  gbpe_lexshard_build(gbpe_lexshard* ls, uint64_t zone_target /* 0: no zone; >= symbols: all zone */);
int  gbpe_lexshard_info_get(const gbpe_lexshard* ls, gbpe_lexshard_info* out);
int  gbpe_lexshard_copy(gbpe_lexshard* ls, int part, void* dst, uint64_t cap_bytes, int dst_on_device);
int  gbpe_lexshard_release(gbpe_lexshard* ls);   /* frees the piece's stream and counts, keeps the lexicon */
int  gbpe_lexshard_remap(gbpe_lexshard* ls, const uint32_t* map, uint64_t n_map, int map_on_device);
void gbpe_lexshard_destroy(gbpe_lexshard* ls);
/* The root trainer: store / mul = every rank's STORE and MUL concatenated in rank
 * order (store_len symbols), zone = every rank's ZONE in rank order, body_len = the symbols of
 * every piece before the zone (the stream is body_len + zone_len symbols; may exceed
 * 2^32).  map_out (map_cap entries) receives one global word id per store entry.
 * The trainer never returns to one dense stream: gbpe_trainer_symbols /
 * export_state fail, gbpe_trainer_expand rebuilds the stream. */
int  gbpe_trainer_create_from_lexicon(gbpe_ctx* ctx, const void* store, const uint32_t* mul, uint64_t store_len,
                                      const void* zone, uint64_t zone_len, uint64_t body_len, int input_on_device,
                                      const gbpe_train_opts* opts, uint32_t* map_out, uint64_t map_cap,
                                      uint64_t* n_map, int map_on_device, gbpe_trainer** out);
/* The current stream (u32 reference layout) of a trainer in the word-lexicon loop:
 * prefix_occ (every rank's remapped OCC in rank order; none for a single-device
 * trainer) then the trainer's own occurrences, then its zone.  out NULL: length only. */
int  gbpe_trainer_expand(gbpe_trainer* t, const uint32_t* prefix_occ, uint64_t n_prefix, int prefix_on_device,
                         uint32_t* out, uint64_t cap, uint64_t* n_out, int out_on_device);

/* ── trie encode (replaces tokenizer.js:54-335 TrieTokenizer over the
 *    tokenize.wgsl kernels) ─────────────────────────────────────────────── */

/* Upload a parsed trie (trie.js:137-160 parseTrieBuffers output): nodes =
 * u32 x 3 per node {firstChild, numChildren, tokenId}, edges = u32 x 2 per
 * edge {symbol, targetNode}.  Replaces tokenizer.js:59-71. */
/* native compileVocabToTrie (trie.js:39-98 + serializeTrie :167-206): token id i
 * has bytes[offsets[i] .. offsets[i+1]) (empty = skipped); writes the v3 blob.
 * out == NULL: *out_len = the size needed.  Host only (no context). */
int  gbpe_trie_compile(const uint8_t* bytes, const uint64_t* offsets, uint32_t n_tokens, uint8_t* out, uint64_t cap,
                       uint64_t* out_len);
/* DXFT .bin (export-controller.js:221-248): u32 [0x44584654, vocabSize,
 * tokenCount, vocabJsonLen] + tokens + vocab JSON bytes.  out == NULL: size only. */
int  gbpe_dxft_pack(const uint32_t* tokens, uint64_t n_tokens, uint32_t vocab_size, const uint8_t* vocab_json,
                    uint64_t json_len, uint8_t* out, uint64_t cap, uint64_t* out_len);
int  gbpe_trie_upload(gbpe_ctx* ctx, const uint32_t* nodes, uint32_t n_nodes,
                      const uint32_t* edges, uint32_t n_edges, gbpe_trie** out);
void gbpe_trie_free(gbpe_trie* trie);
/* double-array size of the uploaded trie; maxTokenLen (tokenizer.js maxTokenLen getter) and max id */
int  gbpe_trie_info(const gbpe_trie* trie, uint32_t* n_records, uint32_t* max_token_len, uint32_t* max_token_id);

/* tokenizer.js:173-206 encodeBytes: chunked greedy longest match.
 * chunk_size 0 = the reference's adaptive size (tokenizer.js:67-68).
 * On GBPE_E_CAPACITY *n_out holds the required token count and nothing is written
 * at or beyond out[out_cap] (tokens below it may or may not have been written). */
int gbpe_encode(gbpe_ctx* ctx, gbpe_trie* trie, const uint8_t* bytes, uint64_t n, uint32_t chunk_size,
                uint32_t* out, uint64_t out_cap, uint64_t* n_out);
/* Device-resident variant: d_bytes / d_out are device pointers (bench path).
 * d_bytes must be 4-byte aligned (any multiple of 4: the walks load 16 bytes at a
 * time from dword-aligned addresses); otherwise GBPE_E_INVALID with *n_out = 0 and
 * nothing launched.  Only d_bytes[0, n) is read: the last partial 16-byte block and
 * the last partial word are loaded byte by byte.  d_out is 4-byte aligned (u32
 * tokens).  On GBPE_E_CAPACITY *n_out holds the required token count, the first
 * out_cap tokens are in d_out and nothing is written at or beyond d_out[out_cap]. */
int gbpe_encode_device(gbpe_ctx* ctx, gbpe_trie* trie, const void* d_bytes, uint64_t n, uint32_t chunk_size,
                       void* d_out, uint64_t out_cap, uint64_t* n_out);
/* Many documents in one call (no reference counterpart: tokenizer.js encodes one
 * buffer at a time).  The documents lie end to end in `bytes`; doc_off has
 * n_docs + 1 non-decreasing entries, doc_off[0] == 0 and doc_off[n_docs] == n, and
 * document d is bytes[doc_off[d] .. doc_off[d+1]) (empty documents allowed).
 * out receives every document's tokens in order and tok_off (n_docs + 1 entries)
 * their boundaries: out[tok_off[d] .. tok_off[d+1]) is exactly what gbpe_encode
 * returns for document d alone with the same chunk_size (at most 2^31) — chunks
 * start at multiples of the chunk size from the document's first byte and no token
 * crosses a document boundary.  On GBPE_E_CAPACITY *n_out holds the required token
 * count, tok_off is complete and nothing is written at or beyond out[out_cap].
 * n_docs == 0 or n == 0: GBPE_OK, *n_out = 0, every tok_off entry 0.
 * Bad offsets: GBPE_E_INVALID (checked on the host before anything is launched). */
int gbpe_encode_batch(gbpe_ctx* ctx, gbpe_trie* trie, const uint8_t* bytes, uint64_t n, const uint64_t* doc_off,
                      uint64_t n_docs, uint32_t chunk_size, uint32_t* out, uint64_t out_cap, uint64_t* tok_off,
                      uint64_t* n_out);
/* Device-resident variant: d_bytes (16-byte aligned), d_doc_off and d_tok_off (u64,
 * 8-byte aligned) and d_out are device pointers.  The offsets are checked by the
 * first kernel; bad offsets return GBPE_E_INVALID before any other kernel runs. */
int gbpe_encode_batch_device(gbpe_ctx* ctx, gbpe_trie* trie, const void* d_bytes, uint64_t n, const void* d_doc_off,
                             uint64_t n_docs, uint32_t chunk_size, void* d_out, uint64_t out_cap, void* d_tok_off,
                             uint64_t* n_out);
/* ── merge-rank encode: TokenizerManager.encode (tokenizer-manager.js:13-61) ──
 * merges = [a, b, newId] x n in learned order, every id at most 0xFFFF.  Exact for
 * every list whose new ids are fresh: each at least 256 and given by one entry only.
 * On that domain a merge whose operand is only created later never fires, a repeated
 * pair keeps its first rank and the pair (0, 0) merges like any other (all as in the
 * reference); new ids may come in any order, 0xFFFF among them.  Any other list —
 * a new id below 256, or one that an earlier entry of the list gave, whether or not
 * that entry can fire — is GBPE_E_INVALID at upload: *out = NULL, nothing is
 * allocated, and gbpe_last_error names the merge's index.
 * gbpe_bpe_encode is gbpe_bpe_encode_words (below) with GBPE_WORDS_NONE and no
 * mask, and has its contract: on GBPE_E_CAPACITY *n_out holds the required token
 * count and the first out_cap tokens are in place; out == NULL goes with
 * out_cap == 0 only (the size query), else GBPE_E_INVALID.
 * gbpe_bpe_encode_last_timing reports this call too. */
typedef struct gbpe_bpe gbpe_bpe;
int  gbpe_bpe_upload(gbpe_ctx* ctx, const uint32_t* merges, uint32_t n_merges, gbpe_bpe** out);
int  gbpe_bpe_encode(gbpe_ctx* ctx, gbpe_bpe* bpe, const uint8_t* bytes, uint64_t n, uint32_t* out, uint64_t out_cap,
                     uint64_t* n_out);
void gbpe_bpe_free(gbpe_bpe* bpe);
/* The same for models with ids above 0xFFFF: every a, b and new id at
 * most GBPE_BPE_MAX_ID, all else as gbpe_bpe_upload (fresh new ids, the first rank
 * of a repeated pair, operands that do not exist yet, *out = NULL and the merge's
 * index in gbpe_last_error on GBPE_E_INVALID).  The handle is a gbpe_bpe like any
 * other: every gbpe_bpe_encode* call takes it, and gbpe_bpe_free releases it.  The
 * rank table keys a pair by both full operands; a list that fits gbpe_bpe_upload
 * gives the same tokens through either call. */
#define GBPE_BPE_MAX_ID 0xFFFFFFu   /* 2^24 - 1 */
int  gbpe_bpe_upload_wide(gbpe_ctx* ctx, const uint32_t* merges, uint32_t n_merges, gbpe_bpe** out);

/* Merge-rank encode within word boundaries: pre-tokenise, then BPE
 * inside each word — what a model trained with word starts means.  word_starts is
 * a byte mask over the input: byte i starts a word iff word_starts[i] != 0, and
 * byte 0 always does.  The output is the concatenation, over the words in order,
 * of what gbpe_bpe_encode returns for that word's bytes alone; no token spans a
 * word start.  Where the word starts come from: */
#define GBPE_WORDS_NONE       0u   /* no word cuts: gbpe_bpe_encode's result */
#define GBPE_WORDS_MASK       1u   /* the caller's mask */
#define GBPE_WORDS_HEURISTIC  2u   /* gbpe_word_boundary's mask of the same bytes, computed on the device */
#define GBPE_WORDS_GPT4       3u   /* gbpe_pretokenize_gpt4's mask of the same bytes (its domain), on the device */
#define GBPE_WORDS_CL100K     4u   /* gbpe_pretokenize_cl100k's mask of the same bytes (its domain), on the device */
#define GBPE_WORDS_O200K      6u   /* gbpe_pretokenize_o200k's mask of the same bytes (its domain), on the device.
                                    * 5 is no mode and stays GBPE_E_INVALID (callers and tests pass it as their
                                    * unknown mode); adding 6 leaves GBPE_ABI_VERSION as it is. */
/* word_starts is non-NULL exactly when words_mode is GBPE_WORDS_MASK; anything
 * else, and an unknown mode, is GBPE_E_INVALID with nothing launched.  n == 0:
 * GBPE_OK, *n_out = 0, nothing launched.  On GBPE_E_CAPACITY *n_out holds the
 * required token count, the first out_cap tokens are in place and nothing is
 * written at or beyond out[out_cap]; out == NULL with out_cap == 0 asks for the
 * size.  The input limit is gbpe_bpe_encode's (one device allocation). */
int gbpe_bpe_encode_words(gbpe_ctx* ctx, gbpe_bpe* bpe, const uint8_t* bytes, uint64_t n, const uint8_t* word_starts,
                          uint32_t words_mode, uint32_t* out, uint64_t out_cap, uint64_t* n_out);
/* Device-resident variant, on the context's stream: d_bytes and d_word_starts are
 * device pointers of any alignment, d_out (u32) is 4-byte aligned, else
 * GBPE_E_INVALID.  Only d_bytes[0, n) and d_word_starts[0, n) are read and only
 * d_out[0, min(total, out_cap)) is written.  Work buffers come from the context's
 * pool. */
int gbpe_bpe_encode_words_device(gbpe_ctx* ctx, gbpe_bpe* bpe, const void* d_bytes, uint64_t n,
                                 const void* d_word_starts, uint32_t words_mode, void* d_out, uint64_t out_cap,
                                 uint64_t* n_out);
/* Many documents in one call (gbpe_encode_batch's layout of bytes,
 * doc_off, out and tok_off): out[tok_off[d] .. tok_off[d+1]) is exactly what
 * gbpe_bpe_encode_words returns for document d alone in the same mode, and no token
 * crosses a document start.  GBPE_WORDS_NONE: each document gets gbpe_bpe_encode's
 * tokens.  GBPE_WORDS_MASK: word_starts has n entries, one mask over the
 * concatenation; a document's first byte starts a word whatever it says.
 * GBPE_WORDS_HEURISTIC, GBPE_WORDS_GPT4, GBPE_WORDS_CL100K, GBPE_WORDS_O200K: each document's own mask
 * (gbpe_pretokenize_gpt4_batch's for GPT4, gbpe_pretokenize_cl100k_batch's for CL100K, gbpe_pretokenize_o200k_batch's for O200K).  The mode and mask rules are
 * gbpe_bpe_encode_words's.  On GBPE_E_CAPACITY *n_out holds the required token
 * count, tok_off is complete, the first out_cap tokens are in place and nothing is
 * written at or beyond out[out_cap]; out == NULL with out_cap == 0 asks for the
 * size.  n == 0 or n_docs == 0: GBPE_OK, *n_out = 0, every tok_off entry 0.  Bad
 * offsets: GBPE_E_INVALID with nothing written; the host form checks them before
 * anything is launched.  The input limit is gbpe_bpe_encode_words's, one device
 * allocation for the whole batch: larger inputs are not split into groups of whole
 * documents the way gbpe_encode_batch splits them. */
int gbpe_bpe_encode_words_batch(gbpe_ctx* ctx, gbpe_bpe* bpe, const uint8_t* bytes, uint64_t n, const uint64_t* doc_off,
                                uint64_t n_docs, const uint8_t* word_starts, uint32_t words_mode, uint32_t* out,
                                uint64_t out_cap, uint64_t* tok_off, uint64_t* n_out);
/* Device-resident variant, on the context's stream: d_bytes and d_word_starts of any
 * alignment, d_doc_off and d_tok_off (u64) 8-byte aligned, d_out (u32) 4-byte
 * aligned, else GBPE_E_INVALID.  Only [0, n) of the inputs and d_doc_off[0, n_docs]
 * are read; only d_out[0, min(total, out_cap)) and d_tok_off[0, n_docs] are written.
 * The first kernel checks the offsets; its verdict comes back with the call's first
 * read-back, before anything is written to d_out or d_tok_off.  Work buffers come
 * from the context's pool; the call synchronises twice, as the single-buffer one. */
int gbpe_bpe_encode_words_batch_device(gbpe_ctx* ctx, gbpe_bpe* bpe, const void* d_bytes, uint64_t n,
                                       const void* d_doc_off, uint64_t n_docs, const void* d_word_starts,
                                       uint32_t words_mode, void* d_out, uint64_t out_cap, void* d_tok_off,
                                       uint64_t* n_out);
/* device ms of the last word encode's kernels: the word-start kernels (a batch call:
 * with the document flags), k_me_long plus the walk, the count scan plus the
 * compaction (a batch call: with the document token offsets) */
int gbpe_bpe_encode_last_timing(gbpe_ctx* ctx, double* ms_starts, double* ms_walk, double* ms_compact);

/* ── special tokens of the merge-rank encode ──────────────────
 * A special table is 1 to GBPE_SPECIALS_MAX distinct byte strings of 1 to
 * GBPE_SPECIAL_MAX_BYTES bytes, each with an id of the caller's choosing (any
 * u32, not checked against the model).  Matching is on the raw bytes, before any
 * pre-tokenisation: scan left to right; where one or more specials match, take the
 * longest and resume just past it; otherwise advance one byte.  The matches are
 * leftmost, longest at a position, and do not overlap.  In a batch call a special
 * lies wholly inside one document: a string that straddles a document start is not
 * a match (a shorter special at the same position that fits still is). */
#define GBPE_SPECIALS_MAX       254u
#define GBPE_SPECIAL_MAX_BYTES  128u
typedef struct gbpe_specials gbpe_specials;
/* Special i is bytes[offsets[i] .. offsets[i+1]) with id ids[i] (gbpe_vocab_upload's
 * layout).  GBPE_E_INVALID with nothing allocated and *out = NULL: no entry or more
 * than GBPE_SPECIALS_MAX, an empty entry, one above GBPE_SPECIAL_MAX_BYTES bytes,
 * the same string twice. */
int  gbpe_specials_upload(gbpe_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, const uint32_t* ids,
                          uint32_t n_specials, gbpe_specials** out);
void gbpe_specials_free(gbpe_specials* specials);
/* The matcher alone: mark_out[i] is 0 for an ordinary byte, 1 + i's index in the
 * table at the first byte of an accepted special and 255 on its other bytes.
 * doc_off == NULL with n_docs == 0: one document.  Otherwise doc_off has
 * n_docs + 1 entries (gbpe_pretokenize_gpt4_batch's rules): bad offsets are
 * GBPE_E_INVALID with mark_out untouched, n == 0 or n_docs == 0 is GBPE_OK with
 * nothing written. */
int gbpe_specials_mark(gbpe_ctx* ctx, gbpe_specials* specials, const uint8_t* bytes, uint64_t n,
                       const uint64_t* doc_off, uint64_t n_docs, uint8_t* mark_out);
/* Device-resident variant: d_bytes and d_mark_out of any alignment, d_doc_off (u64)
 * 8-byte aligned.  Only [0, n) of each is touched. */
int gbpe_specials_mark_device(gbpe_ctx* ctx, gbpe_specials* specials, const void* d_bytes, uint64_t n,
                              const void* d_doc_off, uint64_t n_docs, void* d_mark_out);
/* gbpe_bpe_encode_words* with a special table.  The accepted specials cut a document
 * into pieces, the maximal runs of bytes outside every accepted special; the output
 * is, in order, what gbpe_bpe_encode_words returns for each piece ALONE in the
 * call's mode, and each special's id as one token.  GBPE_WORDS_GPT4, GBPE_WORDS_CL100K,
 * GBPE_WORDS_O200K and GBPE_WORDS_HEURISTIC: the word starts are those of the piece alone (not the whole
 * buffer's with the specials' edges forced: "it" EOT "'s" has word starts 1 1 in
 * its last piece).  GBPE_WORDS_MASK: the caller's mask restricted to the piece, its
 * first byte forced; the entries under a special's bytes are ignored.
 * GBPE_WORDS_NONE: each piece gets gbpe_bpe_encode's tokens.  With a table that
 * never matches the tokens are those of the call without one.  specials == NULL is
 * GBPE_E_INVALID; everything else — arguments, alignment, GBPE_E_CAPACITY, the size
 * query, tok_off, bad offsets — is the contract of the call of the same name
 * without `_special`.  gbpe_bpe_encode_last_timing reports these calls: matching
 * and the flags count under ms_starts. */
int gbpe_bpe_encode_special(gbpe_ctx* ctx, gbpe_bpe* bpe, gbpe_specials* specials, const uint8_t* bytes, uint64_t n,
                            const uint8_t* word_starts, uint32_t words_mode, uint32_t* out, uint64_t out_cap,
                            uint64_t* n_out);
int gbpe_bpe_encode_special_device(gbpe_ctx* ctx, gbpe_bpe* bpe, gbpe_specials* specials, const void* d_bytes, uint64_t n,
                                   const void* d_word_starts, uint32_t words_mode, void* d_out, uint64_t out_cap,
                                   uint64_t* n_out);
int gbpe_bpe_encode_special_batch(gbpe_ctx* ctx, gbpe_bpe* bpe, gbpe_specials* specials, const uint8_t* bytes, uint64_t n,
                                  const uint64_t* doc_off, uint64_t n_docs, const uint8_t* word_starts,
                                  uint32_t words_mode, uint32_t* out, uint64_t out_cap, uint64_t* tok_off,
                                  uint64_t* n_out);
int gbpe_bpe_encode_special_batch_device(gbpe_ctx* ctx, gbpe_bpe* bpe, gbpe_specials* specials, const void* d_bytes,
                                         uint64_t n, const void* d_doc_off, uint64_t n_docs, const void* d_word_starts,
                                         uint32_t words_mode, void* d_out, uint64_t out_cap, void* d_tok_off,
                                         uint64_t* n_out);

/* ── byte spans of the merge-rank encode's tokens ─────────────
 * The most general encode call, with the first byte of every token beside its id.
 * The call's shape is read off its arguments: specials == NULL applies no special
 * table; doc_off == NULL with n_docs == 0 is one document, and tok_off is NULL
 * exactly when doc_off is (anything else: GBPE_E_INVALID).  out is bit for bit what
 * gbpe_bpe_encode_words, _words_batch, _special or _special_batch gives for the same
 * arguments.  tok_start[i] is the index in bytes of the first byte of token i, counted
 * in the whole concatenation for a batch call; token i covers
 * [tok_start[i], tok_start[i+1]) and the last token ends at n.  The tokens tile the
 * input, so no closing entry is written; an empty document contributes no token; a
 * special's one token covers exactly the special's bytes, whatever its id.
 * On GBPE_E_CAPACITY *n_out holds the required count, the first out_cap entries of
 * both out and tok_start are in place, nothing is written at or beyond index out_cap
 * of either, and tok_off is complete.  out == NULL and tok_start == NULL go with
 * out_cap == 0 only (the size query).  n == 0, bad offsets, the mode and mask rules
 * are those of the calls of the same shape.  n above 2^32 - 1 - 4096 is
 * GBPE_E_INVALID with nothing launched: a token's start is kept relative to its
 * chunk in 32 bits.  gbpe_bpe_encode_last_timing reports these calls too. */
int gbpe_bpe_encode_spans(gbpe_ctx* ctx, gbpe_bpe* bpe, gbpe_specials* specials, const uint8_t* bytes, uint64_t n,
                          const uint64_t* doc_off, uint64_t n_docs, const uint8_t* word_starts, uint32_t words_mode,
                          uint32_t* out, uint64_t* tok_start, uint64_t out_cap, uint64_t* tok_off, uint64_t* n_out);
/* Device-resident variant, on the context's stream: d_tok_start, d_doc_off and
 * d_tok_off (u64) are 8-byte aligned and d_out (u32) 4-byte aligned, else
 * GBPE_E_INVALID with nothing launched; d_bytes and d_word_starts may have any
 * alignment.  Only d_out and d_tok_start[0, min(total, out_cap)) and
 * d_tok_off[0, n_docs] are written. */
int gbpe_bpe_encode_spans_device(gbpe_ctx* ctx, gbpe_bpe* bpe, gbpe_specials* specials, const void* d_bytes, uint64_t n,
                                 const void* d_doc_off, uint64_t n_docs, const void* d_word_starts, uint32_t words_mode,
                                 void* d_out, void* d_tok_start, uint64_t out_cap, void* d_tok_off, uint64_t* n_out);

/* device ms of the last encode's kernels (walk, scan, compact); after a batch call:
 * the walk, every scan and table kernel (document table, descriptors, count scan),
 * the compaction with the document token offsets (the last group's, when the host
 * variant ran several) */
int gbpe_encode_last_timing(gbpe_ctx* ctx, double* ms_walk, double* ms_scan, double* ms_compact);

/* ── device decode (replaces the host loop of tokenizer.js:344-363 decode) ───
 * Token ids back to bytes: per-token lengths, an exclusive scan, a scatter of
 * the vocab bytes.  The output is exactly the reference's decode:
 * each id's vocab bytes in order, and every id >= the vocab's n_tokens —
 * 0xFFFFFFFF included — yields EF BF BD (U+FFFD, tokenizer.js:18, 350).  Such an
 * id is clamped before any table read, so a bad id never becomes an
 * out-of-range load. */

/* Token id i has bytes[offsets[i] .. offsets[i+1]) — the layout gbpe_trie_compile
   takes.  Empty entries are allowed and decode to nothing.  An entry longer than
   65,535 bytes is GBPE_E_INVALID (a 4096-token block's byte prefix then fits 32
   bits), and so are offsets that decrease. */
int  gbpe_vocab_upload(gbpe_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, uint32_t n_tokens,
                       gbpe_vocab** out);
void gbpe_vocab_free(gbpe_vocab* vocab);

/* Host only (no context, no device), like gbpe_trie_compile: the exact decoded
   size.  An id >= n_vocab counts 3 bytes (U+FFFD, tokenizer.js:18, 350).
   tokens may be NULL when n_tokens == 0; any other null argument is GBPE_E_INVALID. */
int  gbpe_decode_size(const uint64_t* vocab_offsets, uint32_t n_vocab, const uint32_t* tokens, uint64_t n_tokens,
                      uint64_t* n_bytes);

/* Host buffers in and out.  n_tokens == 0: GBPE_OK, *n_out = 0, nothing launched.
 * On GBPE_E_CAPACITY *n_out holds the required byte count, the first out_cap
 * bytes are in out and nothing is written at or beyond out[out_cap].  Token
 * streams above the decode slice (32M tokens) run slice by slice through the
 * context's pooled buffers; a slice may start at any token. */
int gbpe_decode(gbpe_ctx* ctx, gbpe_vocab* vocab, const uint32_t* tokens, uint64_t n_tokens, uint8_t* out,
                uint64_t out_cap, uint64_t* n_out);
/* Device-resident variant: d_tokens (u32, 4-byte aligned) and d_out (16-byte
 * aligned) are device pointers; a wrong alignment is GBPE_E_INVALID with
 * *n_out = 0 and nothing launched.  Only d_tokens[0, n_tokens) is read and only
 * d_out[0, min(total, out_cap)) is ever written; on GBPE_E_CAPACITY *n_out holds
 * the required byte count and the first out_cap bytes are in d_out. */
int gbpe_decode_device(gbpe_ctx* ctx, gbpe_vocab* vocab, const void* d_tokens, uint64_t n_tokens, void* d_out,
                       uint64_t out_cap, uint64_t* n_out);
/* Many documents in one call: the documents' tokens lie end to end in `tokens`;
 * tok_off has n_docs + 1 non-decreasing entries, tok_off[0] == 0 and
 * tok_off[n_docs] == n_tokens, and document d is tokens[tok_off[d] .. tok_off[d+1])
 * (empty documents allowed).  out receives every document's bytes in order — the
 * bytes gbpe_decode gives the whole stream — and byte_off (n_docs + 1 entries)
 * their boundaries: out[byte_off[d] .. byte_off[d+1]) is document d.  On
 * GBPE_E_CAPACITY *n_out holds the required byte count, byte_off is complete, the
 * first out_cap bytes are in place and nothing is written at or beyond
 * out[out_cap].  n_docs == 0 or n_tokens == 0: GBPE_OK, *n_out = 0, every byte_off
 * entry 0.  Bad offsets: GBPE_E_INVALID (checked on the host before anything is
 * launched).  Above the decode slice a document may span slices: a byte_off entry
 * comes from the slice that holds token tok_off[d], shifted by the running total. */
int gbpe_decode_batch(gbpe_ctx* ctx, gbpe_vocab* vocab, const uint32_t* tokens, uint64_t n_tokens,
                      const uint64_t* tok_off, uint64_t n_docs, uint8_t* out, uint64_t out_cap, uint64_t* byte_off,
                      uint64_t* n_out);
/* Device-resident variant: d_tokens (4-byte aligned), d_tok_off and d_byte_off
 * (u64, 8-byte aligned) and d_out (16-byte aligned) are device pointers.  The
 * offsets are checked on the device by the kernel that writes d_byte_off, which
 * never indexes the prefix arrays with an entry above n_tokens; the status comes
 * back with the total, and on bad offsets (GBPE_E_INVALID, *n_out = 0) the scatter
 * is not launched, d_out is untouched and d_byte_off is unspecified. */
int gbpe_decode_batch_device(gbpe_ctx* ctx, gbpe_vocab* vocab, const void* d_tokens, uint64_t n_tokens,
                             const void* d_tok_off, uint64_t n_docs, void* d_out, uint64_t out_cap, void* d_byte_off,
                             uint64_t* n_out);
/* device ms of the last decode's kernels: lengths + block scan, the scan of the
 * block sums with the document byte offsets, the scatter (the last slice's, when
 * the host variant ran several) */
int gbpe_decode_last_timing(gbpe_ctx* ctx, double* ms_len, double* ms_scan, double* ms_scatter);

/* ── device memory helpers for device-resident callers ─────────────────── */
int gbpe_device_alloc(gbpe_ctx* ctx, uint64_t bytes, void** dptr);
int gbpe_device_free(gbpe_ctx* ctx, void* dptr);
int gbpe_memcpy_h2d(gbpe_ctx* ctx, void* dst, const void* src, uint64_t bytes);
int gbpe_memcpy_d2h(gbpe_ctx* ctx, void* dst, const void* src, uint64_t bytes);
int gbpe_synchronize(gbpe_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* GPUBPE_H */
