// GPU checks of TrieTokenizer.encodeBatch through the N-API addon: every view
// must equal the tokens the CPU oracle produced for that document alone
// (argv[2] JSON: {vocab, chunkSize, docs_b64[], tokens[][], text_b64, text_tokens}).
import fs from 'fs';
import { BPEEngine, TrieTokenizer } from '../../gpu-bpe_amd/js/index.js';

const c = JSON.parse(fs.readFileSync(process.argv[2]));
function fail(msg) { console.error('FAIL ' + msg); process.exit(1); }
function same(a, b) { return JSON.stringify(Array.from(a)) === JSON.stringify(b); }

async function main() {
    const engine = await new BPEEngine().init();
    if (!('k_trie_walk_batch' in engine.pipelines)) fail('kernel inventory');
    const tok = TrieTokenizer.fromVocab(engine, c.vocab, c.chunkSize ? { chunkSize: c.chunkSize } : {});
    const docs = c.docs_b64.map(function (b) { return new Uint8Array(Buffer.from(b, 'base64')); });
    if (!docs.some(function (d) { return d.length === 0; })) fail('the case needs an empty document');
    let checks = 0;
    const views = await tok.encodeBatch(docs);
    if (views.length !== docs.length) fail('view count');
    for (let d = 0; d < docs.length; d++) {
        if (!(views[d] instanceof Uint32Array)) fail('view type ' + d);
        if (!same(views[d], c.tokens[d])) fail('tokens of document ' + d);
        if (d && views[d].buffer !== views[0].buffer) fail('views share one buffer');
        checks++;
    }
    // a batch call and a single-stream call in flight together on one engine
    const text = new Uint8Array(Buffer.from(c.text_b64, 'base64'));
    const both = await Promise.all([tok.encodeBatch(docs), tok.encodeBytes(text)]);
    for (let d = 0; d < docs.length; d++) if (!same(both[0][d], c.tokens[d])) fail('concurrent batch, document ' + d);
    if (!same(both[1], c.text_tokens)) fail('concurrent encodeBytes');
    checks += 2;
    // nothing to encode: no device call
    const none = await tok.encodeBatch([]);
    if (none.length !== 0) fail('empty batch');
    const empties = await tok.encodeBatch([new Uint8Array(0), new Uint8Array(0)]);
    if (empties.length !== 2 || empties[0].length !== 0 || empties[1].length !== 0) fail('batch of empty documents');
    checks += 2;
    // bad offsets through the addon reject with the library's status
    const n = (await import('../../gpu-bpe_amd/js/native.js')).native();
    let threw = false;
    try {
        await n.encodeBatch(engine.device, tok._trie, docs[1], new Float64Array([0, docs[1].length + 1]), tok.chunkSize);
    } catch (e) { threw = /status -1/.test(e.message); }
    if (!threw) fail('bad offsets must reject');
    checks++;
    // free the trie while a batch is in flight: it completes, nothing is used after free
    const pending = tok.encodeBatch(docs);
    tok.destroy();
    const late = await pending;
    for (let d = 0; d < docs.length; d++) if (!same(late[d], c.tokens[d])) fail('batch across trie free, document ' + d);
    checks++;
    engine.destroy();
    console.log('ok ' + checks + ' checks');
}
main().catch(function (e) { fail(e && e.stack || e); });
