/**
 * MergeEncoder — TokenizerManager.encode (src/bpe/tokenizer/tokenizer-manager.js:13-61)
 * on the MI355X: the learned merges applied in rank order to the whole text, or,
 * with word starts, inside each word alone (pre-tokenise, then BPE per word).
 * encode(text) → { tokens, text, vocab, vocabStrings } as the reference's
 * (model = { vocab, vocabStrings, merges }).  opts = { wordStarts: Uint8Array (one
 * entry per byte, non-zero = word start) } or { words: 'gpt4' | 'heuristic' } (the
 * mask computed on the device); without opts no word is cut.  encodeBatch(docs,
 * opts) encodes many documents in one call.  Node 12 syntax.
 */
import { native } from './native.js';

const WORDS_MASK = 1;
const WORDS_MODES = { heuristic: 2, gpt4: 3 };

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

export class MergeEncoder {
    constructor(engine, model) {
        this._engine = engine;
        this._model = model;
        const merges = model.merges || [];
        const flat = new Uint32Array(merges.length * 3);
        merges.forEach(function (m, i) { flat[3 * i] = m[0]; flat[3 * i + 1] = m[1]; flat[3 * i + 2] = m[2]; });
        this._h = native().bpeUpload(engine.device, flat);
    }

    encodeBytes(bytes, opts) {
        const ws = opts && opts.wordStarts !== undefined && opts.wordStarts !== null ? opts.wordStarts : null;
        const words = opts && opts.words !== undefined && opts.words !== null ? opts.words : null;
        if (ws === null && words === null) return native().bpeEncode(this._engine.device, this._h, bytes);
        if (ws !== null && words !== null) throw new TypeError('encodeBytes: give wordStarts or words, not both');
        if (ws !== null) {
            if (!(ws instanceof Uint8Array) || ws.length !== bytes.length) {
                throw new TypeError('encodeBytes: wordStarts must be a Uint8Array with one entry per byte');
            }
            return native().bpeEncodeWords(this._engine.device, this._h, bytes, ws, WORDS_MASK);
        }
        if (!Object.prototype.hasOwnProperty.call(WORDS_MODES, words)) {
            throw new TypeError("encodeBytes: words must be 'gpt4' or 'heuristic'");
        }
        return native().bpeEncodeWords(this._engine.device, this._h, bytes, null, WORDS_MODES[words]);
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
                throw new TypeError("encodeBatch: words must be 'gpt4' or 'heuristic'");
            }
            mode = WORDS_MODES[words];
        }
        return native().bpeEncodeWordsBatch(this._engine.device, this._h, flat.bytes, flat.offsets, ws, mode);
    }

    async encode(text, opts) {
        const bytes = new Uint8Array(Buffer.from(text, 'utf8'));
        const tokens = Array.from(this.encodeBytes(bytes, opts));
        return { tokens: tokens, text: text, vocab: this._model.vocab, vocabStrings: this._model.vocabStrings };
    }
}
