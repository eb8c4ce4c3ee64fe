// Runs the `strategy` option of the JS facade (RawDeflate, Deflate, and
// GZip's deflateOptions; include/zt_strategy.h) over cases prepared by
// tests/test_js_strategy.py.  Prints one JSON result per case; bytes travel as
// hex.
import fs from 'fs';
import { RawDeflate, Deflate, GZip, Strategy } from '../../zlib.ts_amd/lib/index.js';

const hex = (s) => Uint8Array.from(Buffer.from(s, 'hex'));
const tohex = (a) => Buffer.from(a.buffer, a.byteOffset, a.length).toString('hex');
const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = [];
for (const c of cases) {
    const r = { id: c.id };
    try {
        const input = hex(c.in);
        const opts = Object.assign({}, c.opts);
        if (c.op === 'constants') {
            r.constants = Strategy;
        } else if (c.op === 'raw') {
            if (c.dictionary) opts.dictionary = hex(c.dictionary);
            const d = new RawDeflate(input, opts);
            r.out = tohex(d.compress());
            r.strategy = d.strategy === undefined ? null : d.strategy;
        } else if (c.op === 'zlib') {
            const d = new Deflate(input, opts);
            r.out = tohex(d.compress());
            r.adler32 = d.adler32;
            r.strategy = d.strategy === undefined ? null : d.strategy;
        } else if (c.op === 'gzip') {
            const g = new GZip(input, { deflateOptions: opts, mtime: 7, buildIndex: !!c.buildIndex });
            r.out = tohex(g.compress());
            r.crc32 = g.crc32;
        } else {
            throw new Error('unknown op ' + c.op);
        }
    } catch (e) {
        r.error = { message: typeof e === 'string' ? e : e.message, status: e.ztStatus };
    }
    out.push(r);
}
console.log(JSON.stringify(out));
