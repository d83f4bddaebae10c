// GPU checks of MergeEncoder on models with ids above 0xFFFF through the N-API addon: the
// constructor takes the wide upload, and the tokens equal the CPU references' (argv[2] JSON:
// {cases: [{name, merges, text_b64, want: {none, gpt4}}]}).
import fs from 'fs';
import { BPEEngine, MergeEncoder } from '../../gpu-bpe_amd/js/index.js';

const c = JSON.parse(fs.readFileSync(process.argv[2]));
function fail(msg) { console.error('FAIL ' + msg); process.exit(1); }
function same(a, b) { return a.length === b.length && Array.from(a).every(function (v, i) { return v === b[i]; }); }

async function main() {
    const engine = await new BPEEngine().init();
    if (!('k_me_walk_wide' in engine.pipelines)) fail('kernel inventory: k_me_walk_wide');
    let checks = 1;
    for (const k of c.cases) {
        const enc = new MergeEncoder(engine, { merges: k.merges, vocab: [], vocabStrings: [] });
        if (enc.wide !== true) fail(k.name + ': the wide upload was not taken');
        const bytes = new Uint8Array(Buffer.from(k.text_b64, 'base64'));
        if (!same(enc.encodeBytes(bytes), k.want.none)) fail(k.name + ': whole string');
        if (!same(enc.encodeBytes(bytes, { words: 'gpt4' }), k.want.gpt4)) fail(k.name + ": words: 'gpt4'");
        checks += 3;
    }
    // a narrow list still takes the narrow upload; an id above the bound comes back with the status and the merge
    const narrow = new MergeEncoder(engine, { merges: [[97, 98, 0xFFFF]], vocab: [], vocabStrings: [] });
    if (narrow.wide !== false || !same(narrow.encodeBytes(Uint8Array.from([97, 98])), [0xFFFF])) fail('narrow list');
    let threw = false;
    try {
        new MergeEncoder(engine, { merges: [[97, 98, 256], [97, 97, 0x1000000]], vocab: [], vocabStrings: [] });
    } catch (e) { threw = /status -1/.test(e.message) && /merge 1 /.test(e.message); }
    if (!threw) fail('an id above 0xFFFFFF must throw with the status and the merge');
    checks += 2;
    engine.destroy();
    console.log('ok ' + checks + ' checks');
}
main().catch(function (e) { fail(e && e.stack || e); });
