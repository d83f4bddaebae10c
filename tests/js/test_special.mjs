// GPU checks of the special tokens through the N-API addon: MergeEncoder with specialTokens —
// encodeBytes, encodeBatch and findSpecial must equal what the CPU reference gave (argv[2] JSON:
// {merges, text_b64, offsets[], specials_b64[], ids[], single[], batch: {tokens, offsets}, mark[],
// mark_batch[]}).
import fs from 'fs';
import { BPEEngine, MergeEncoder } from '../../gpu-bpe_amd/js/index.js';

const c = JSON.parse(fs.readFileSync(process.argv[2]));
function fail(msg) { console.error('FAIL ' + msg); process.exit(1); }
function same(a, b) { return a.length === b.length && Array.from(a).every(function (v, i) { return v === b[i]; }); }

async function main() {
    const engine = await new BPEEngine().init();
    for (const k of ['k_sp_cand', 'k_sp_accept', 'k_me_sp_mask', 'k_me_walk_special']) {
        if (!(k in engine.pipelines)) fail('kernel inventory: ' + k);
    }
    const model = { merges: c.merges, vocab: [], vocabStrings: [] };
    const table = new Map();
    c.specials_b64.forEach(function (b, i) { table.set(new Uint8Array(Buffer.from(b, 'base64')), c.ids[i]); });
    const enc = new MergeEncoder(engine, model, { specialTokens: table });
    const plain = new MergeEncoder(engine, model);
    const bytes = new Uint8Array(Buffer.from(c.text_b64, 'base64'));
    const docs = [];
    for (let d = 0; d + 1 < c.offsets.length; d++) docs.push(bytes.subarray(c.offsets[d], c.offsets[d + 1]));
    let checks = 0;
    if (!same(enc.encodeBytes(bytes, { words: 'gpt4' }), c.single)) fail('encodeBytes');
    const r = enc.encodeBatch(docs, { words: 'gpt4' });
    if (!(r.tokens instanceof Uint32Array) || !(r.offsets instanceof Float64Array)) fail('encodeBatch: result shape');
    if (!same(r.tokens, c.batch.tokens) || !same(r.offsets, c.batch.offsets)) fail('encodeBatch');
    const r2 = enc.encodeBatch(bytes, { offsets: c.offsets, words: 'gpt4' });
    if (!same(r2.tokens, c.batch.tokens) || !same(r2.offsets, c.batch.offsets)) fail('encodeBatch, one buffer with offsets');
    checks += 3;
    // a table given as an object of strings is the same table
    const obj = {};
    c.specials_b64.forEach(function (b, i) { obj[Buffer.from(b, 'base64').toString('utf8')] = c.ids[i]; });
    const enc2 = new MergeEncoder(engine, model, { specialTokens: obj });
    if (!same(enc2.encodeBytes(bytes, { words: 'gpt4' }), c.single)) fail('specialTokens as an object');
    checks++;
    // findSpecial
    const m = enc.findSpecial(bytes);
    if (!(m instanceof Uint8Array) || !same(m, c.mark)) fail('findSpecial');
    if (!same(enc.findSpecial(docs), c.mark_batch)) fail('findSpecial, documents');
    if (!same(enc.findSpecial(bytes, c.offsets), c.mark_batch)) fail('findSpecial, offsets');
    checks += 3;
    // special: false is the encoder without a table
    if (!same(enc.encodeBytes(bytes, { words: 'gpt4', special: false }), plain.encodeBytes(bytes, { words: 'gpt4' }))) {
        fail('special: false');
    }
    const p = plain.encodeBatch(docs, { words: 'gpt4' });
    const q = enc.encodeBatch(docs, { words: 'gpt4', special: false });
    if (!same(p.tokens, q.tokens) || !same(p.offsets, q.offsets)) fail('special: false, batch');
    if (same(p.tokens, c.batch.tokens)) fail('the case needs specials that change the tokens');
    checks += 2;
    // the whole string with a special in it
    const xy = new MergeEncoder(engine, { merges: [[120, 32, 256], [256, 121, 257]] }, { specialTokens: { '<|e|>': 999 } });
    if (!same(xy.encodeBytes(new Uint8Array(Buffer.from('x y<|e|>x y'))), [257, 999, 257])) fail('x y<|e|>x y');
    if (!same(xy.encodeBytes(new Uint8Array(Buffer.from('x <|e|>y'))), [256, 999, 121])) fail('x <|e|>y');
    if (!same((await xy.encode('x <|e|>y')).tokens, [256, 999, 121])) fail('encode');
    checks += 3;
    // bad tables
    const long = new Uint8Array(129).fill(97);
    const bad = [{}, { '': 1 }, new Map([[long, 1]]), new Map([['a', 1], [new Uint8Array([97]), 2]]), { a: -1 }, { a: 1.5 }];
    for (const t of bad) {
        let threw = false;
        try { new MergeEncoder(engine, model, { specialTokens: t }); } catch (err) { threw = err instanceof RangeError || err instanceof TypeError; }
        if (!threw) fail('a bad table must throw');
        checks++;
    }
    let threw = false;
    try { plain.findSpecial(bytes); } catch (err) { threw = err instanceof TypeError; }
    if (!threw) fail('findSpecial without a table must throw');
    threw = false;
    try { enc.findSpecial(bytes, [0, 50, 40, bytes.length]); } catch (err) { threw = /status -1/.test(err.message); }
    if (!threw) fail('decreasing offsets must throw with the status');
    checks += 2;
    engine.destroy();
    console.log('ok ' + checks + ' checks');
}
main().catch(function (e) { fail(e && e.stack || e); });
