// GPU checks of MergeEncoder.encodeBatch and GpuPreTokenizer.preTokenizeBatch through the
// N-API addon: tokens, token offsets and word starts must equal what the per-document
// CPU oracle gave (argv[2] JSON: {merges, text_b64, offsets[], mask[], want: {none, mask,
// heuristic, gpt4: {tokens, offsets}}, ws_gpt4[], pairs: [{docs_b64[], per}]}).
import fs from 'fs';
import { BPEEngine, MergeEncoder, GpuPreTokenizer } from '../../gpu-bpe_amd/js/index.js';

const c = JSON.parse(fs.readFileSync(process.argv[2]));
function fail(msg) { console.error('FAIL ' + msg); process.exit(1); }
function same(a, b) { return a.length === b.length && Array.from(a).every(function (v, i) { return v === b[i]; }); }
function check(r, want, what) {
    if (!(r.tokens instanceof Uint32Array) || !(r.offsets instanceof Float64Array)) fail(what + ': result shape');
    if (!same(r.tokens, want.tokens)) fail(what + ': tokens');
    if (!same(r.offsets, want.offsets)) fail(what + ': offsets');
}

async function main() {
    const engine = await new BPEEngine().init();
    for (const k of ['k_doc_flags', 'k_pretok_docs', 'k_me_walk_docs', 'k_me_tok_off']) {
        if (!(k in engine.pipelines)) fail('kernel inventory: ' + k);
    }
    const enc = new MergeEncoder(engine, { merges: c.merges, vocab: [], vocabStrings: [] });
    const bytes = new Uint8Array(Buffer.from(c.text_b64, 'base64'));
    const mask = Uint8Array.from(c.mask);
    const docs = [];
    for (let d = 0; d + 1 < c.offsets.length; d++) docs.push(bytes.subarray(c.offsets[d], c.offsets[d + 1]));
    let checks = 0;
    // one case per mode, as a list of documents and as one buffer with offsets
    check(enc.encodeBatch(docs), c.want.none, 'no opts');
    check(enc.encodeBatch(docs, { wordStarts: mask }), c.want.mask, 'wordStarts');
    check(enc.encodeBatch(docs, { words: 'heuristic' }), c.want.heuristic, "words: 'heuristic'");
    check(enc.encodeBatch(docs, { words: 'gpt4' }), c.want.gpt4, "words: 'gpt4'");
    check(enc.encodeBatch(bytes, { offsets: c.offsets, words: 'gpt4' }), c.want.gpt4, 'one buffer with offsets');
    checks += 5;
    if (same(enc.encodeBytes(bytes, { words: 'gpt4' }), c.want.gpt4.tokens)) fail('the case needs cuts that change the tokens');
    // a document alone through encodeBytes is its slice of the batch
    const r = enc.encodeBatch(docs, { words: 'gpt4' });
    for (const d of [0, 1, 17, docs.length - 1]) {
        if (!same(enc.encodeBytes(docs[d], { words: 'gpt4' }), r.tokens.subarray(r.offsets[d], r.offsets[d + 1]))) fail('document ' + d);
        checks++;
    }
    // the word starts
    const pt = new GpuPreTokenizer(engine);
    const w = pt.preTokenizeBatch(docs);
    if (!same(w.wordStarts, c.ws_gpt4) || !same(w.offsets, c.offsets) || !same(w.bytes, bytes)) fail('preTokenizeBatch');
    if (!same(pt.preTokenizeBatch(bytes, c.offsets).wordStarts, c.ws_gpt4)) fail('preTokenizeBatch with offsets');
    checks += 2;
    for (const p of c.pairs) {
        const pd = p.docs_b64.map(function (b) { return new Uint8Array(Buffer.from(b, 'base64')); });
        if (Array.from(pt.preTokenizeBatch(pd).wordStarts).join('') !== p.per) fail('hand pair ' + p.per);
        checks++;
    }
    // nothing to encode
    const e = enc.encodeBatch([], { words: 'gpt4' });
    if (e.tokens.length !== 0 || !same(e.offsets, [0])) fail('no documents');
    const e2 = enc.encodeBatch([new Uint8Array(0), new Uint8Array(0)]);
    if (e2.tokens.length !== 0 || !same(e2.offsets, [0, 0, 0])) fail('empty documents');
    checks += 2;
    // bad arguments
    const bad = [{ wordStarts: mask, words: 'gpt4' }, { wordStarts: mask.subarray(1) }, { words: 'words' }];
    for (const opts of bad) {
        let threw = false;
        try { enc.encodeBatch(docs, opts); } catch (err) { threw = err instanceof TypeError; }
        if (!threw) fail('bad opts must throw: ' + JSON.stringify(Object.keys(opts)));
        checks++;
    }
    // offsets the library refuses come back with its status
    let threw = false;
    try { enc.encodeBatch(bytes, { offsets: [0, 50, 40, bytes.length] }); } catch (err) { threw = /status -1/.test(err.message); }
    if (!threw) fail('decreasing offsets must throw with the status');
    threw = false;
    try { pt.preTokenizeBatch(bytes, [0, 50, bytes.length - 1]); } catch (err) { threw = /status -1/.test(err.message); }
    if (!threw) fail('offsets that stop short must throw with the status');
    checks += 2;
    engine.destroy();
    console.log('ok ' + checks + ' checks');
}
main().catch(function (e) { fail(e && e.stack || e); });
