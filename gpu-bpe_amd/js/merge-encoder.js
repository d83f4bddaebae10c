/**
 * MergeEncoder — TokenizerManager.encode (src/bpe/tokenizer/tokenizer-manager.js:13-61)
 * on the MI355X: the learned merges applied in rank order to the whole text, or,
 * with word starts, inside each word alone (pre-tokenise, then BPE per word).
 * encode(text) → { tokens, text, vocab, vocabStrings } as the reference's
 * (model = { vocab, vocabStrings, merges }).  opts = { wordStarts: Uint8Array (one
 * entry per byte, non-zero = word start) } or { words: 'gpt4' | 'heuristic' | 'cl100k' | 'o200k_base' }
 * (the mask computed on the device; 'cl100k' / 'o200k_base' are the exact cl100k_base / o200k_base split patterns);
 * without opts no word is cut.  encodeBatch(docs,
 * opts) encodes many documents in one call.  new MergeEncoder(engine, model,
 * { specialTokens: { '<|endoftext|>': id, ... } | Map of string or Uint8Array to id })
 * matches those strings on the raw bytes: each is one token and the text between
 * them is encoded as if alone; opts.special === false gives the result without the
 * table, findSpecial(bytes, offsets) the matches (0 / 1 + index / 255 per byte).
 * encodeBytesSpans / encodeBatchSpans take the same opts and also return starts, a
 * Float64Array of tokens.length + 1 byte offsets (the input's length at the end): token i
 * covers bytes starts[i] to starts[i + 1], a special's token the special's bytes.
 * Exact for every merge list whose new ids are at least 256 and distinct (any order,
 * repeated pairs, the pair (0, 0) and operands created later or never included); a
 * new id below 256 or given twice makes the constructor throw (GBPE_E_INVALID, the
 * message names the merge).  A list that holds an id above 0xFFFF is uploaded through
 * gbpe_bpe_upload_wide (ids up to 0xFFFFFF); every call is the same.
 * Node 12 syntax.
 */
import { native } from './native.js';

const WORDS_MASK = 1;
const WORDS_MODES = { heuristic: 2, gpt4: 3, cl100k: 4, o200k_base: 6 };

/** { bytes, offsets: Float64Array } of an array of Uint8Array laid end to end, or of one buffer with its offsets. */
export function flattenDocuments(docs, offsets) {
    if (offsets !== undefined && offsets !== null) {
        return { bytes: docs, offsets: offsets instanceof Float64Array ? offsets : Float64Array.from(offsets) };
    }
    const offs = new Float64Array(docs.length + 1);
    for (let d = 0; d < docs.length; d++) offs[d + 1] = offs[d] + docs[d].length;
    const bytes = new Uint8Array(offs[docs.length]);
    for (let d = 0; d < docs.length; d++) bytes.set(docs[d], offs[d]);
    return { bytes: bytes, offsets: offs };
}

/**
 * A special table checked on the host: [{ bytes: Uint8Array, id }] in the given order.
 * 1 to 254 distinct strings of 1 to 128 bytes, ids in [0, 2^32); anything else throws.
 */
export function checkedSpecialTokens(specialTokens) {
    const entries = specialTokens instanceof Map ? Array.from(specialTokens.entries())
        : (specialTokens && typeof specialTokens === 'object' ? Object.keys(specialTokens).map(function (k) {
            return [k, specialTokens[k]];
        }) : null);
    if (entries === null) throw new TypeError('specialTokens: give an object or a Map of string or Uint8Array to id');
    const seen = new Set();
    const table = entries.map(function (e) {
        const raw = typeof e[0] === 'string' ? new Uint8Array(Buffer.from(e[0], 'utf8')) : e[0];
        if (!(raw instanceof Uint8Array)) throw new TypeError('specialTokens: a key must be a string or a Uint8Array');
        if (raw.length < 1 || raw.length > 128) throw new RangeError('specialTokens: an entry has 1 to 128 bytes');
        const key = Buffer.from(raw).toString('hex');
        if (seen.has(key)) throw new RangeError('specialTokens: an entry is given twice');
        seen.add(key);
        if (!Number.isInteger(e[1]) || e[1] < 0 || e[1] > 0xFFFFFFFF) {
            throw new RangeError('specialTokens: an id must be an integer in [0, 2^32)');
        }
        return { bytes: raw, id: e[1] };
    });
    if (table.length < 1 || table.length > 254) throw new RangeError('specialTokens: 1 to 254 entries');
    return table;
}

export class MergeEncoder {
    constructor(engine, model, opts) {
        this._engine = engine;
        this._model = model;
        this._sp = null;
        this.specialTokens = opts && opts.specialTokens ? checkedSpecialTokens(opts.specialTokens) : null;
        const merges = model.merges || [];
        const flat = new Uint32Array(merges.length * 3);
        // ids above 0xFFFF take the wide rank table (gbpe_bpe_upload_wide, up to 0xFFFFFF); what no u32 holds
        // goes in as 0xFFFFFFFF, so that the library rejects it and names the merge
        let wide = false;
        merges.forEach(function (m, i) {
            for (let k = 0; k < 3; k++) {
                const v = Number.isInteger(m[k]) && m[k] >= 0 && m[k] <= 0xFFFFFFFF ? m[k] : 0xFFFFFFFF;
                if (v > 0xFFFF) wide = true;
                flat[3 * i + k] = v;
            }
        });
        this.wide = wide;
        this._h = wide ? native().bpeUploadWide(engine.device, flat) : native().bpeUpload(engine.device, flat);
        if (this.specialTokens !== null) {
            const flatSp = flattenDocuments(this.specialTokens.map(function (e) { return e.bytes; }));
            const ids = Uint32Array.from(this.specialTokens.map(function (e) { return e.id; }));
            this._sp = native().specialsUpload(engine.device, flatSp.bytes, flatSp.offsets, ids);
        }
    }

    /** The table a call uses: the encoder's unless opts.special === false; opts.special === true insists on one. */
    _special(opts) {
        const special = opts && opts.special !== undefined && opts.special !== null ? opts.special : null;
        if (special === false) return null;
        if (special === true && this._sp === null) throw new TypeError('special: true on an encoder without specialTokens');
        return this._sp;
    }

    /** The matches of the special table: Uint8Array, 0 / 1 + index / 255 per byte; offsets: the documents'. */
    findSpecial(bytes, offsets) {
        if (this._sp === null) throw new TypeError('findSpecial: the encoder has no specialTokens');
        const flat = Array.isArray(bytes) || (offsets !== undefined && offsets !== null) ? flattenDocuments(bytes, offsets) : null;
        return flat === null ? native().specialsMark(this._engine.device, this._sp, bytes, null)
            : native().specialsMark(this._engine.device, this._sp, flat.bytes, flat.offsets);
    }

    encodeBytes(bytes, opts) {
        const ws = opts && opts.wordStarts !== undefined && opts.wordStarts !== null ? opts.wordStarts : null;
        const words = opts && opts.words !== undefined && opts.words !== null ? opts.words : null;
        const sp = this._special(opts);
        const dev = this._engine.device;
        const h = this._h;
        const run = function (mask, mode) {
            return sp !== null ? native().bpeEncodeSpecial(dev, h, sp, bytes, mask, mode)
                : native().bpeEncodeWords(dev, h, bytes, mask, mode);
        };
        if (ws === null && words === null) return sp !== null ? run(null, 0) : native().bpeEncode(dev, h, bytes);
        if (ws !== null && words !== null) throw new TypeError('encodeBytes: give wordStarts or words, not both');
        if (ws !== null) {
            if (!(ws instanceof Uint8Array) || ws.length !== bytes.length) {
                throw new TypeError('encodeBytes: wordStarts must be a Uint8Array with one entry per byte');
            }
            return run(ws, WORDS_MASK);
        }
        if (!Object.prototype.hasOwnProperty.call(WORDS_MODES, words)) {
            throw new TypeError("encodeBytes: words must be 'gpt4', 'heuristic', 'cl100k' or 'o200k_base'");
        }
        return run(null, WORDS_MODES[words]);
    }

    /**
     * Many documents in one call: docs is an array of Uint8Array, or one Uint8Array
     * with opts.offsets (D + 1 document offsets from 0 to its length).  Returns
     * { tokens: Uint32Array, offsets: Float64Array }: document d's tokens are
     * tokens.subarray(offsets[d], offsets[d + 1]), exactly encodeBytes of that
     * document alone with the same opts.  opts.wordStarts is one mask over the
     * concatenation; a document's first byte starts a word whatever it says.
     */
    encodeBatch(docs, opts) {
        const flat = flattenDocuments(docs, opts && opts.offsets);
        const ws = opts && opts.wordStarts !== undefined && opts.wordStarts !== null ? opts.wordStarts : null;
        const words = opts && opts.words !== undefined && opts.words !== null ? opts.words : null;
        if (ws !== null && words !== null) throw new TypeError('encodeBatch: give wordStarts or words, not both');
        let mode = 0;
        if (ws !== null) {
            if (!(ws instanceof Uint8Array) || ws.length !== flat.bytes.length) {
                throw new TypeError('encodeBatch: wordStarts must be a Uint8Array with one entry per byte');
            }
            mode = WORDS_MASK;
        } else if (words !== null) {
            if (!Object.prototype.hasOwnProperty.call(WORDS_MODES, words)) {
                throw new TypeError("encodeBatch: words must be 'gpt4', 'heuristic', 'cl100k' or 'o200k_base'");
            }
            mode = WORDS_MODES[words];
        }
        const sp = this._special(opts);
        if (sp !== null) {
            return native().bpeEncodeSpecialBatch(this._engine.device, this._h, sp, flat.bytes, flat.offsets, ws, mode);
        }
        return native().bpeEncodeWordsBatch(this._engine.device, this._h, flat.bytes, flat.offsets, ws, mode);
    }

    /** The mode and mask of opts, checked as encodeBytes / encodeBatch check them; `name` is the caller's. */
    _wordsOf(name, n, opts) {
        const ws = opts && opts.wordStarts !== undefined && opts.wordStarts !== null ? opts.wordStarts : null;
        const words = opts && opts.words !== undefined && opts.words !== null ? opts.words : null;
        if (ws !== null && words !== null) throw new TypeError(name + ': give wordStarts or words, not both');
        if (ws !== null) {
            if (!(ws instanceof Uint8Array) || ws.length !== n) {
                throw new TypeError(name + ': wordStarts must be a Uint8Array with one entry per byte');
            }
            return { mask: ws, mode: WORDS_MASK };
        }
        if (words === null) return { mask: null, mode: 0 };
        if (!Object.prototype.hasOwnProperty.call(WORDS_MODES, words)) {
            throw new TypeError(name + ": words must be 'gpt4', 'heuristic', 'cl100k' or 'o200k_base'");
        }
        return { mask: null, mode: WORDS_MODES[words] };
    }

    /**
     * encodeBytes with the byte span of every token (gbpe_bpe_encode_spans):
     * { tokens: Uint32Array, starts: Float64Array }, starts[i] the first byte of token i
     * and bytes.length at the end.  Options and errors are encodeBytes's.
     */
    encodeBytesSpans(bytes, opts) {
        const w = this._wordsOf('encodeBytes', bytes.length, opts);
        return native().bpeEncodeSpans(this._engine.device, this._h, this._special(opts), bytes, null, w.mask, w.mode);
    }

    /**
     * encodeBatch with the byte span of every token: { tokens, offsets, starts }, starts
     * counted in the concatenation of the documents.  Options and errors are encodeBatch's.
     */
    encodeBatchSpans(docs, opts) {
        const flat = flattenDocuments(docs, opts && opts.offsets);
        const w = this._wordsOf('encodeBatch', flat.bytes.length, opts);
        return native().bpeEncodeSpans(this._engine.device, this._h, this._special(opts), flat.bytes, flat.offsets, w.mask,
            w.mode);
    }

    async encode(text, opts) {
        const bytes = new Uint8Array(Buffer.from(text, 'utf8'));
        const tokens = Array.from(this.encodeBytes(bytes, opts));
        return { tokens: tokens, text: text, vocab: this._model.vocab, vocabStrings: this._model.vocabStrings };
    }
}
