// Runs the `dictionary` option of the JS facade (zlib.ts_amd/lib RawDeflate /
// RawInflate / Deflate / Inflate) over cases prepared by tests/test_js_dict.py
// and prints one JSON result per case.  Bytes travel as hex.
import fs from 'fs';
import { RawDeflate, RawInflate, Deflate, Inflate } from '../../zlib.ts_amd/lib/index.js';

const hex = (s) => Uint8Array.from(Buffer.from(s, 'hex'));
const tohex = (a) => Buffer.from(a.buffer, a.byteOffset, a.length).toString('hex');
const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = [];
for (const c of cases) {
    const r = { id: c.id };
    try {
        const opts = Object.assign({}, c.opts || {});
        if (c.dictionary !== undefined && c.dictionary !== null) opts.dictionary = hex(c.dictionary);
        const input = hex(c.in);
        if (c.op === 'rawDeflate') {
            r.out = tohex(new RawDeflate(input, opts).compress());
        } else if (c.op === 'rawInflate') {
            const x = new RawInflate(input, opts);
            r.out = tohex(x.decompress());
            r.ip = x.ip;
        } else if (c.op === 'deflate') {
            const x = new Deflate(input, opts);
            r.out = tohex(x.compress());
            r.adler32 = x.adler32;
        } else if (c.op === 'inflate') {
            const x = new Inflate(input, opts);
            r.out = tohex(x.decompress());
            r.ip = x.ip;
            r.adler32 = x.adler32;
        } else {
            throw new Error('unknown op ' + c.op);
        }
    } catch (e) {
        r.error = { message: typeof e === 'string' ? e : e.message, status: e.ztStatus };
    }
    out.push(r);
}
console.log(JSON.stringify(out));
