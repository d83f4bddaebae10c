/**
 * TrieTokenizer — drop-in for the reference src/bpe/tokenizer/tokenizer.js
 * over the HIP chunked trie walk.  Chunk size: options.chunkSize, else
 * max(512, min(2048, maxTokenLen * 8)) (tokenizer.js:67-68); tokens never
 * cross a chunk; unmatched bytes map to their byte value.
 */
import { native } from './native.js';
import { compileVocabToTrie, parseHeader, parseTrieBuffers } from './trie.js';

const DEFAULT_CHUNK_SIZE = 512;
const UTF8_REPLACEMENT = [0xEF, 0xBF, 0xBD];

export class TrieTokenizer {
    constructor(engine, trieData, vocab, options) {
        this._engine = engine;
        const byteVocab = [];
        for (let i = 0; i < 256; i++) byteVocab.push([i]);
        this._vocab = vocab || byteVocab;
        const header = parseHeader(trieData);
        const bufs = parseTrieBuffers(trieData, header);
        this.nodeCount = header.nodeCount;
        this.edgeCount = header.edgeCount;
        this.maxTokenLen = header.maxTokenLen;
        const adaptive = Math.max(DEFAULT_CHUNK_SIZE, Math.min(2048, header.maxTokenLen * 8));
        this._chunkSize = options && options.chunkSize !== undefined && options.chunkSize !== null
            ? options.chunkSize : adaptive;
        this._trie = native().trieUpload(engine.device, bufs.nodes, bufs.edges);
        console.log('[ok] TrieTokenizer: ' + this.nodeCount + ' nodes, ' + this.edgeCount + ' edges, chunk=' +
            this._chunkSize);
    }

    static fromVocab(engine, vocab, options) {
        return new TrieTokenizer(engine, compileVocabToTrie(vocab), vocab, options || {});
    }

    get chunkSize() { return this._chunkSize; }

    async encodeBytes(bytes) {
        if (bytes.length === 0) return new Uint32Array(0);
        return native().encode(this._engine.device, this._trie, bytes, this._chunkSize);
    }

    /**
     * Many documents in one device call (an addition to the reference's API):
     * one Uint32Array per document, each what encodeBytes returns for that
     * document alone, all views into one shared buffer.
     */
    async encodeBatch(docs) {
        const offsets = new Float64Array(docs.length + 1);
        for (let d = 0; d < docs.length; d++) offsets[d + 1] = offsets[d] + docs[d].length;
        const total = offsets[docs.length];
        if (docs.length === 0 || total === 0) return docs.map(function () { return new Uint32Array(0); });
        const bytes = new Uint8Array(total);
        for (let d = 0; d < docs.length; d++) bytes.set(docs[d], offsets[d]);
        const r = await native().encodeBatch(this._engine.device, this._trie, bytes, offsets, this._chunkSize);
        const views = [];
        for (let d = 0; d < docs.length; d++) views.push(r.tokens.subarray(r.offsets[d], r.offsets[d + 1]));
        return views;
    }

    decode(tokens) {
        let total = 0;
        const parts = [];
        for (const t of tokens) {
            const idx = Number(t);
            const b = idx < this._vocab.length ? this._vocab[idx] : UTF8_REPLACEMENT;
            parts.push(b);
            total += b.length;
        }
        const out = new Uint8Array(total);
        let off = 0;
        for (const p of parts) { out.set(p, off); off += p.length; }
        return out;
    }

    /** The vocab table on the device, uploaded on first use. */
    _deviceVocab() {
        if (!this._dvocab) {
            const offsets = new Float64Array(this._vocab.length + 1);
            for (let i = 0; i < this._vocab.length; i++) offsets[i + 1] = offsets[i] + this._vocab[i].length;
            const bytes = new Uint8Array(offsets[this._vocab.length]);
            for (let i = 0; i < this._vocab.length; i++) bytes.set(this._vocab[i], offsets[i]);
            this._dvocab = native().vocabUpload(this._engine.device, bytes, offsets);
        }
        return this._dvocab;
    }

    /** decode() on the device (an addition to the reference's API): the same bytes. */
    async decodeBytes(tokens) {
        if (tokens.length === 0) return new Uint8Array(0);
        const t = tokens instanceof Uint32Array ? tokens : Uint32Array.from(tokens);
        return native().decode(this._engine.device, this._deviceVocab(), t);
    }

    /**
     * Many token documents in one device call: one Uint8Array per document,
     * each what decode returns for that document alone, all views into one
     * shared buffer (mirrors encodeBatch).
     */
    async decodeBatch(docs) {
        const offsets = new Float64Array(docs.length + 1);
        for (let d = 0; d < docs.length; d++) offsets[d + 1] = offsets[d] + docs[d].length;
        const total = offsets[docs.length];
        if (docs.length === 0 || total === 0) return docs.map(function () { return new Uint8Array(0); });
        const tokens = new Uint32Array(total);
        for (let d = 0; d < docs.length; d++) tokens.set(docs[d], offsets[d]);
        const r = await native().decodeBatch(this._engine.device, this._deviceVocab(), tokens, offsets);
        const views = [];
        for (let d = 0; d < docs.length; d++) views.push(r.bytes.subarray(r.offsets[d], r.offsets[d + 1]));
        return views;
    }

    destroy() {
        if (this._dvocab) native().vocabFree(this._dvocab);
        this._dvocab = null;
        if (this._trie) native().trieFree(this._trie);
        this._trie = null;
    }
}
