// GPU checks of TrieTokenizer.decodeBytes / decodeBatch through the N-API addon:
// the bytes must equal what the CPU oracle decoded (argv[2] JSON: {vocab, docs[][],
// docs_b64[], stream_b64}), and what the host loop decode() returns.
import fs from 'fs';
import { BPEEngine, TrieTokenizer } from '../../gpu-bpe_amd/js/index.js';

const c = JSON.parse(fs.readFileSync(process.argv[2]));
function fail(msg) { console.error('FAIL ' + msg); process.exit(1); }
function same(a, b) { return a.length === b.length && Buffer.from(a.buffer, a.byteOffset, a.length).equals(Buffer.from(b.buffer, b.byteOffset, b.length)); }
function bytes(b64) { return new Uint8Array(Buffer.from(b64, 'base64')); }

async function main() {
    const engine = await new BPEEngine().init();
    for (const k of ['k_dec_len', 'k_dec_scatter', 'k_dec_doc_off']) if (!(k in engine.pipelines)) fail('kernel inventory: ' + k);
    const tok = TrieTokenizer.fromVocab(engine, c.vocab, {});
    const docs = c.docs.map(function (d) { return Uint32Array.from(d); });
    const want = c.docs_b64.map(bytes);
    if (!docs.some(function (d) { return d.length === 0; })) fail('the case needs an empty document');
    let checks = 0;
    // one stream
    const stream = Uint32Array.from([].concat(...c.docs));
    const whole = await tok.decodeBytes(stream);
    if (!(whole instanceof Uint8Array)) fail('decodeBytes type');
    if (!same(whole, bytes(c.stream_b64))) fail('decodeBytes against the oracle');
    if (!same(whole, tok.decode(stream))) fail('decodeBytes(x) equals decode(x)');
    if (!same(await tok.decodeBytes(Array.from(stream)), whole)) fail('decodeBytes of a plain array');
    if ((await tok.decodeBytes(new Uint32Array(0))).length !== 0) fail('decodeBytes of nothing');
    checks += 4;
    // many documents
    const views = await tok.decodeBatch(docs);
    if (views.length !== docs.length) fail('view count');
    for (let d = 0; d < docs.length; d++) {
        if (!(views[d] instanceof Uint8Array)) fail('view type ' + d);
        if (!same(views[d], want[d])) fail('bytes of document ' + d);
        if (!same(views[d], tok.decode(docs[d]))) fail('decodeBatch equals decode, document ' + d);
        if (d && views[d].buffer !== views[0].buffer) fail('views share one buffer');
        checks++;
    }
    // a batch call and a single-stream call in flight together on one engine
    const both = await Promise.all([tok.decodeBatch(docs), tok.decodeBytes(stream)]);
    for (let d = 0; d < docs.length; d++) if (!same(both[0][d], want[d])) fail('concurrent batch, document ' + d);
    if (!same(both[1], whole)) fail('concurrent decodeBytes');
    checks += 2;
    // nothing to decode: no device call
    if ((await tok.decodeBatch([])).length !== 0) fail('empty batch');
    const empties = await tok.decodeBatch([new Uint32Array(0), new Uint32Array(0)]);
    if (empties.length !== 2 || empties[0].length !== 0 || empties[1].length !== 0) fail('batch of empty documents');
    checks += 2;
    // bad offsets through the addon reject with the library's status
    const n = (await import('../../gpu-bpe_amd/js/native.js')).native();
    let threw = false;
    try {
        await n.decodeBatch(engine.device, tok._deviceVocab(), docs[2], new Float64Array([0, docs[2].length + 1]));
    } catch (e) { threw = /status -1/.test(e.message); }
    if (!threw) fail('bad offsets must reject');
    checks++;
    // free the vocab while a batch is in flight: it completes, nothing is used after free
    const pending = tok.decodeBatch(docs);
    tok.destroy();
    const late = await pending;
    for (let d = 0; d < docs.length; d++) if (!same(late[d], want[d])) fail('batch across vocab free, document ' + d);
    checks++;
    tok.destroy();
    engine.destroy();
    console.log('ok ' + checks + ' checks');
}
main().catch(function (e) { fail(e && e.stack || e); });
