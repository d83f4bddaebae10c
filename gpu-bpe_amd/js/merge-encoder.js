/**
 * MergeEncoder — TokenizerManager.encode (src/bpe/tokenizer/tokenizer-manager.js:13-61)
 * on the MI355X: the learned merges applied in rank order to the whole text, or,
 * with word starts, inside each word alone (pre-tokenise, then BPE per word).
 * encode(text) → { tokens, text, vocab, vocabStrings } as the reference's
 * (model = { vocab, vocabStrings, merges }).  opts = { wordStarts: Uint8Array (one
 * entry per byte, non-zero = word start) } or { words: 'gpt4' | 'heuristic' } (the
 * mask computed on the device); without opts no word is cut.  Node 12 syntax.
 */
import { native } from './native.js';

const WORDS_MASK = 1;
const WORDS_MODES = { heuristic: 2, gpt4: 3 };

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

    async encode(text, opts) {
        const bytes = new Uint8Array(Buffer.from(text, 'utf8'));
        const tokens = Array.from(this.encodeBytes(bytes, opts));
        return { tokens: tokens, text: text, vocab: this._model.vocab, vocabStrings: this._model.vocabStrings };
    }
}
