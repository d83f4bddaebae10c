// GPU checks of { words: 'o200k_base' } (MergeEncoder) and { rules: 'o200k_base' } (GpuPreTokenizer)
// through the N-API addon against fixtures the Python side computed (argv[2] JSON:
// {merges, text_b64, mask[], tokens[], docs_b64[], doc_masks[][], doc_tokens[][]}).
import fs from 'fs';
import { BPEEngine, GpuPreTokenizer, MergeEncoder } from '../../gpu-bpe_amd/js/index.js';

const c = JSON.parse(fs.readFileSync(process.argv[2]));
function fail(msg) { console.error('FAIL ' + msg); process.exit(1); }
function same(a, b) { return a.length === b.length && Array.from(a).every(function (v, i) { return v === b[i]; }); }
function b64(s) { return new Uint8Array(Buffer.from(s, 'base64')); }

async function main() {
    const engine = await new BPEEngine().init();
    for (const k of ['k_pretok_o200k', 'k_pretok_o200k_docs']) if (!(k in engine.pipelines)) fail('kernel inventory: ' + k);
    const enc = new MergeEncoder(engine, { merges: c.merges, vocab: [], vocabStrings: [] });
    const pt = new GpuPreTokenizer(engine);
    const bytes = b64(c.text_b64);
    const docs = c.docs_b64.map(b64);
    let checks = 0;
    // the word starts
    if (!same(pt.preTokenizeBytes(bytes, { rules: 'o200k_base' }).wordStarts, c.mask)) fail("preTokenizeBytes rules: 'o200k_base'");
    if (same(pt.preTokenizeBytes(bytes).wordStarts, c.mask)) fail('the default rules must stay the GPT-4 ones');
    if (same(pt.preTokenizeBytes(bytes, { rules: 'cl100k' }).wordStarts, c.mask)) fail("rules: 'cl100k' must stay cl100k_base's");
    if (!same(pt.preTokenizeBytes(bytes, { rules: 'gpt4' }).wordStarts, pt.preTokenizeBytes(bytes).wordStarts)) fail("rules: 'gpt4'");
    const text = Buffer.from(docs[3]).toString('utf8');
    if (!same(pt.preTokenize(text, { rules: 'o200k_base' }).wordStarts, c.doc_masks[3])) fail("preTokenize rules: 'o200k_base'");
    const batch = pt.preTokenizeBatch(docs, null, { rules: 'o200k_base' });
    if (!same(batch.wordStarts, [].concat.apply([], c.doc_masks))) fail("preTokenizeBatch rules: 'o200k_base'");
    if (pt.preTokenizeBytes(new Uint8Array(0), { rules: 'o200k_base' }).wordStarts.length !== 0) fail('empty input');
    checks += 7;
    // the tokens
    if (!same(enc.encodeBytes(bytes, { words: 'o200k_base' }), c.tokens)) fail("encodeBytes words: 'o200k_base'");
    if (same(enc.encodeBytes(bytes, { words: 'cl100k' }), c.tokens)) fail('the case needs an input on which the two split patterns differ');
    const r = await enc.encode(text, { words: 'o200k_base' });
    if (!same(r.tokens, c.doc_tokens[3]) || r.text !== text) fail('encode(text, opts)');
    const eb = enc.encodeBatch(docs, { words: 'o200k_base' });
    if (!same(eb.tokens, [].concat.apply([], c.doc_tokens))) fail("encodeBatch words: 'o200k_base'");
    let at = 0;
    c.doc_tokens.forEach(function (t, d) {
        if (eb.offsets[d] !== at) fail('encodeBatch offsets');
        at += t.length;
    });
    if (eb.offsets[docs.length] !== at) fail('encodeBatch last offset');
    checks += 5;
    // bad names, the short name among them, still throw a TypeError
    for (const call of [function () { enc.encodeBytes(bytes, { words: 'o200k' }); },
                        function () { enc.encodeBatch(docs, { words: 'words' }); },
                        function () { enc.encodeBytes(bytes, { words: 'o200k_base', wordStarts: Uint8Array.from(c.mask) }); },
                        function () { pt.preTokenizeBytes(bytes, { rules: 'o200k' }); },
                        function () { pt.preTokenizeBatch(docs, null, { rules: 'rules' }); }]) {
        let threw = false;
        try { call(); } catch (e) { threw = e instanceof TypeError; }
        if (!threw) fail('a bad name must throw a TypeError');
        checks++;
    }
    engine.destroy();
    console.log('ok ' + checks + ' checks');
}
main().catch(function (e) { fail(e && e.stack || e); });
