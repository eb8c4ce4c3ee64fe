// Runs the `buildIndex: true` option of the JS facade's writers (zlib.ts_amd/lib
// RawDeflate, GZip, Deflate) over inputs prepared by
// tests/test_js_deflate_index.py: per case the written bytes, the index left
// in streamIndex, RawInflate.buildIndex() of the same bytes and ranges read
// through streamIndex.  Inputs come from files; results travel as hex.
import fs from 'fs';
import { RawDeflate, GZip, Deflate, RawInflate } from '../../zlib.ts_amd/lib/index.js';

const tohex = (a) => Buffer.from(a.buffer, a.byteOffset, a.length).toString('hex');
const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = [];
for (const c of cases) {
    const r = { id: c.id };
    try {
        const input = Uint8Array.from(fs.readFileSync(c.file));
        const opts = Object.assign({}, c.opts || {});
        if (c.prefix) opts.outputBuffer = Uint8Array.from(Buffer.from(c.prefix, 'hex'));
        const make = (o) => c.kind === 'raw' ? new RawDeflate(input, o) : c.kind === 'gzip' ? new GZip(input, o)
            : new Deflate(input, o);
        const w = make(Object.assign({}, opts, { buildIndex: true }));
        const bytes = w.compress();
        const plainOpts = Object.assign({}, opts);
        if (c.prefix) plainOpts.outputBuffer = Uint8Array.from(Buffer.from(c.prefix, 'hex'));
        const p = make(plainOpts);
        const plain = p.compress();
        r.sameBytes = Buffer.compare(Buffer.from(bytes), Buffer.from(plain)) === 0;
        r.plainHasNoIndex = p.streamIndex === undefined;
        r.length = bytes.length;
        r.streamIndex = tohex(w.streamIndex);
        const x = new RawInflate(bytes, { index: c.start });
        r.built = tohex(x.buildIndex());
        r.ranges = x.decompressRanges(w.streamIndex, c.ranges).map(tohex);
        r.range = tohex(x.decompressRange(w.streamIndex, c.ranges[0][0], c.ranges[0][1]));
    } catch (e) {
        r.error = { message: typeof e === 'string' ? e : e.message, status: e.ztStatus };
    }
    out.push(r);
}
console.log(JSON.stringify({ results: out }));
