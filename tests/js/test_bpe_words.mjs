// GPU checks of MergeEncoder.encodeBytes / encode with word starts through the N-API
// addon: the tokens must equal what the per-word CPU oracle gave (argv[2] JSON:
// {merges, text_b64, mask[], want: {none, mask, heuristic, gpt4}}).
import fs from 'fs';
import { BPEEngine, MergeEncoder } from '../../gpu-bpe_amd/js/index.js';

const c = JSON.parse(fs.readFileSync(process.argv[2]));
function fail(msg) { console.error('FAIL ' + msg); process.exit(1); }
function same(a, b) { return a.length === b.length && Array.from(a).every(function (v, i) { return v === b[i]; }); }

async function main() {
    const engine = await new BPEEngine().init();
    for (const k of ['k_me_long', 'k_me_walk_words']) if (!(k in engine.pipelines)) fail('kernel inventory: ' + k);
    const enc = new MergeEncoder(engine, { merges: c.merges, vocab: [], vocabStrings: [] });
    const bytes = new Uint8Array(Buffer.from(c.text_b64, 'base64'));
    const mask = Uint8Array.from(c.mask);
    let checks = 0;
    // calls without opts behave as before
    if (!same(enc.encodeBytes(bytes), c.want.none)) fail('encodeBytes without opts');
    if (!same(enc.encodeBytes(bytes, {}), c.want.none)) fail('encodeBytes with empty opts');
    checks += 2;
    // the three modes
    if (!same(enc.encodeBytes(bytes, { wordStarts: mask }), c.want.mask)) fail('wordStarts');
    if (!same(enc.encodeBytes(bytes, { words: 'heuristic' }), c.want.heuristic)) fail("words: 'heuristic'");
    if (!same(enc.encodeBytes(bytes, { words: 'gpt4' }), c.want.gpt4)) fail("words: 'gpt4'");
    checks += 3;
    if (same(c.want.gpt4, c.want.none)) fail('the case needs an input on which words change the tokens');
    // encode(text, opts) passes them through
    const text = Buffer.from(bytes).toString('utf8');
    const r = await enc.encode(text, { words: 'gpt4' });
    if (!same(r.tokens, c.want.gpt4) || r.text !== text) fail('encode(text, opts)');
    if (!same((await enc.encode(text)).tokens, c.want.none)) fail('encode(text)');
    checks += 2;
    // nothing to encode
    if (enc.encodeBytes(new Uint8Array(0), { words: 'gpt4' }).length !== 0) fail('empty input');
    if (enc.encodeBytes(new Uint8Array(0), { wordStarts: new Uint8Array(0) }).length !== 0) fail('empty input and mask');
    checks += 2;
    // bad arguments
    const bad = [{ wordStarts: mask, words: 'gpt4' }, { wordStarts: mask.subarray(1) }, { words: 'words' }, { wordStarts: [1, 0] }];
    for (const opts of bad) {
        let threw = false;
        try { enc.encodeBytes(bytes, opts); } catch (e) { threw = e instanceof TypeError; }
        if (!threw) fail('bad opts must throw: ' + JSON.stringify(Object.keys(opts)));
        checks++;
    }
    // a mode the library does not know comes back with its status
    const n = (await import('../../gpu-bpe_amd/js/native.js')).native();
    let threw = false;
    try { n.bpeEncodeWords(engine.device, enc._h, bytes, null, 9); } catch (e) { threw = /status -1/.test(e.message); }
    if (!threw) fail('an unknown mode must throw with the status');
    threw = false;
    try { n.bpeEncodeWords(engine.device, enc._h, bytes, null, 1); } catch (e) { threw = /status -1/.test(e.message); }
    if (!threw) fail('mode 1 without a mask must throw with the status');
    checks += 2;
    engine.destroy();
    console.log('ok ' + checks + ' checks');
}
main().catch(function (e) { fail(e && e.stack || e); });
