// Runs GUnzip.decompressBatch / Inflate.decompressBatch of the JS facade
// (zlib.ts_amd/lib) over batches prepared by tests/test_js_container_batch.py
// and prints one JSON result per batch.  Bytes travel as hex.
import fs from 'fs';
import { GUnzip, Inflate } from '../../zlib.ts_amd/lib/index.js';

const hex = (s) => Uint8Array.from(Buffer.from(s, 'hex'));
const tohex = (a) => Buffer.from(a.buffer, a.byteOffset, a.length).toString('hex');
const batches = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = [];
for (const b of batches) {
    const r = { id: b.id };
    try {
        const inputs = b.items.map(hex);
        let res;
        if (b.op === 'gunzip') {
            res = GUnzip.decompressBatch(inputs);
        } else if (b.op === 'inflate') {
            const opts = Object.assign({}, b.opts || {});
            if (b.dictionary !== undefined && b.dictionary !== null) opts.dictionary = hex(b.dictionary);
            res = Inflate.decompressBatch(inputs, opts);
        } else {
            throw new Error('unknown op ' + b.op);
        }
        r.isArray = Array.isArray(res);
        r.items = res.map((x) => {
            if (x instanceof Error) return { error: { message: x.message, status: x.ztStatus } };
            const o = { out: tohex(x.output) };
            if (x.ip !== undefined) o.ip = x.ip;
            if (x.adler32 !== undefined) o.adler32 = x.adler32;
            if (x.members) {
                o.members = x.members.map((m) => ({
                    flg: m.flg, mtime: m.mtime.getTime() / 1000, xfl: m.xfl, os: m.os, xlen: m.xlen, name: m.name,
                    comment: m.comment, crc16: m.crc16, data: tohex(m.data),
                }));
            }
            return o;
        });
    } catch (e) {
        r.error = { message: typeof e === 'string' ? e : e.message, status: e.ztStatus };
    }
    out.push(r);
}
console.log(JSON.stringify(out));
