/**
 * GpuPreTokenizer — the reference PreTokenizer (src/wasm/pre_tokenizer.mjs:402-509)
 * with its GPT-4 word-boundary rules computed on the MI355X.
 *
 * preTokenizeBytes(bytes) / preTokenize(text) return { bytes, wordStarts } like
 * the reference; BPETrainer.train(input, { preTokenizer }) accepts it the same
 * way (trainer.js:62-99).  Input must already be NFC (the reference
 * NFC-normalises first, which leaves NFC text unchanged).  Every call takes
 * { rules: 'cl100k' } for the word starts of the cl100k_base split pattern instead, or
 * { rules: 'o200k_base' } for those of the o200k_base split pattern (no normalisation
 * belongs to either); the default, 'gpt4', is the rules above.
 * Node 12 syntax.
 */
import { native } from './native.js';
import { flattenDocuments } from './merge-encoder.js';

function rulesOf(opts, what) {
    const rules = opts && opts.rules !== undefined && opts.rules !== null ? opts.rules : 'gpt4';
    if (rules !== 'gpt4' && rules !== 'cl100k' && rules !== 'o200k_base') {
        throw new TypeError(what + ": rules must be 'gpt4', 'cl100k' or 'o200k_base'");
    }
    return rules;
}

export class GpuPreTokenizer {
    constructor(engine) {
        if (!engine) throw new Error('GpuPreTokenizer requires an initialized BPEEngine');
        this._engine = engine;
    }

    preTokenizeBytes(rawBytes, opts) {
        const rules = rulesOf(opts, 'preTokenizeBytes');
        if (!rawBytes || rawBytes.length === 0) return { bytes: new Uint8Array(0), wordStarts: new Uint8Array(0) };
        const bytes = rawBytes instanceof Uint8Array ? rawBytes : new Uint8Array(rawBytes);
        const wordStarts = rules === 'o200k_base' ? native().pretokenizeO200k(this._engine.device, bytes)
            : rules === 'cl100k' ? native().pretokenizeCl100k(this._engine.device, bytes)
            : native().pretokenizeGpt4(this._engine.device, bytes);
        return { bytes, wordStarts };
    }

    /**
     * Word starts of many documents in one call: docs is an array of Uint8Array, or one
     * Uint8Array with its D + 1 offsets.  Returns { bytes, wordStarts, offsets } over the
     * concatenation; each document's part is exactly preTokenizeBytes of it alone.
     */
    preTokenizeBatch(docs, offsets, opts) {
        const rules = rulesOf(opts, 'preTokenizeBatch');
        const flat = flattenDocuments(docs, offsets);
        const wordStarts = rules === 'o200k_base' ? native().pretokenizeO200kBatch(this._engine.device, flat.bytes, flat.offsets)
            : rules === 'cl100k' ? native().pretokenizeCl100kBatch(this._engine.device, flat.bytes, flat.offsets)
            : native().pretokenizeGpt4Batch(this._engine.device, flat.bytes, flat.offsets);
        return { bytes: flat.bytes, wordStarts: wordStarts, offsets: flat.offsets };
    }

    preTokenize(text, opts) {
        if (!text || text.length === 0) return { bytes: new Uint8Array(0), wordStarts: new Uint8Array(0) };
        return this.preTokenizeBytes(new Uint8Array(Buffer.from(text, 'utf8')), opts);
    }
}
