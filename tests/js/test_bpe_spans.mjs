// GPU checks of the tokens' byte spans through the N-API addon: MergeEncoder.encodeBytesSpans and
// encodeBatchSpans must equal what the Python layer gave (argv[2] JSON: {cases: [{merges, specials_b64[],
// ids[], docs_b64[] | text_b64, opts, tokens[], starts[], offsets[] | null}]}).
import fs from 'fs';
import { BPEEngine, MergeEncoder } from '../../gpu-bpe_amd/js/index.js';

const c = JSON.parse(fs.readFileSync(process.argv[2]));
function fail(msg) { console.error('FAIL ' + msg); process.exit(1); }
function same(a, b) { return a.length === b.length && Array.from(a).every(function (v, i) { return v === b[i]; }); }
function bytesOf(b) { return new Uint8Array(Buffer.from(b, 'base64')); }
function throwsType(f) {
    try { f(); } catch (err) { return err instanceof TypeError; }
    return false;
}

async function main() {
    const engine = await new BPEEngine().init();
    for (const k of ['k_me_walk_spans', 'k_me_compact_spans']) {
        if (!(k in engine.pipelines)) fail('kernel inventory: ' + k);
    }
    let checks = 0;
    for (const k of c.cases) {
        const table = new Map();
        k.specials_b64.forEach(function (b, i) { table.set(bytesOf(b), k.ids[i]); });
        const model = { merges: k.merges, vocab: [], vocabStrings: [] };
        const enc = new MergeEncoder(engine, model, table.size ? { specialTokens: table } : undefined);
        if (k.docs_b64) {
            const docs = k.docs_b64.map(bytesOf);
            const r = enc.encodeBatchSpans(docs, k.opts);
            if (!(r.tokens instanceof Uint32Array) || !(r.starts instanceof Float64Array) || !(r.offsets instanceof Float64Array)) {
                fail(k.name + ': result shape');
            }
            if (!same(r.tokens, k.tokens) || !same(r.starts, k.starts) || !same(r.offsets, k.offsets)) fail(k.name);
            const old = enc.encodeBatch(docs, k.opts);
            if (!same(r.tokens, old.tokens) || !same(r.offsets, old.offsets)) fail(k.name + ': encodeBatch differs');
            // one buffer with its offsets is the same call
            const total = docs.reduce(function (a, d) { return a + d.length; }, 0);
            const cat = new Uint8Array(total);
            const offs = [0];
            docs.forEach(function (d) { cat.set(d, offs[offs.length - 1]); offs.push(offs[offs.length - 1] + d.length); });
            const r2 = enc.encodeBatchSpans(cat, Object.assign({ offsets: offs }, k.opts));
            if (!same(r2.tokens, k.tokens) || !same(r2.starts, k.starts) || !same(r2.offsets, k.offsets)) fail(k.name + ', offsets');
            checks += 3;
        } else {
            const bytes = bytesOf(k.text_b64);
            const r = enc.encodeBytesSpans(bytes, k.opts);
            if (!(r.tokens instanceof Uint32Array) || !(r.starts instanceof Float64Array) || 'offsets' in r) fail(k.name + ': result shape');
            if (!same(r.tokens, k.tokens) || !same(r.starts, k.starts)) fail(k.name);
            if (!same(r.tokens, enc.encodeBytes(bytes, k.opts))) fail(k.name + ': encodeBytes differs');
            if (r.starts[r.starts.length - 1] !== bytes.length) fail(k.name + ': the closing entry');
            checks += 3;
        }
    }
    // the option errors are encodeBytes's and encodeBatch's
    const plain = new MergeEncoder(engine, { merges: [[97, 97, 256]] });
    const two = new Uint8Array([97, 97]);
    const bad = [{ wordStarts: new Uint8Array(2), words: 'gpt4' }, { words: 'gpt2' }, { wordStarts: new Uint8Array(3) },
        { wordStarts: [1, 0] }, { special: true }];
    for (const o of bad) {
        if (!throwsType(function () { plain.encodeBytes(two, o); })) fail('encodeBytes must throw: ' + JSON.stringify(o));
        if (!throwsType(function () { plain.encodeBytesSpans(two, o); })) fail('encodeBytesSpans must throw: ' + JSON.stringify(o));
        if (!throwsType(function () { plain.encodeBatch([two], o); })) fail('encodeBatch must throw: ' + JSON.stringify(o));
        if (!throwsType(function () { plain.encodeBatchSpans([two], o); })) fail('encodeBatchSpans must throw: ' + JSON.stringify(o));
        checks += 2;
    }
    let threw = false;
    try { plain.encodeBatchSpans(two, { offsets: [0, 2, 1] }); } catch (err) { threw = /status -1/.test(err.message); }
    if (!threw) fail('decreasing offsets must throw with the status');
    const e = plain.encodeBytesSpans(new Uint8Array(0));
    if (e.tokens.length !== 0 || !same(e.starts, [0])) fail('empty input');
    checks += 2;
    engine.destroy();
    console.log('ok ' + checks + ' checks');
}
main().catch(function (e) { fail(e && e.stack || e); });
