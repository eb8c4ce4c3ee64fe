// Runs RawInflateSession of the JS facade (zlib.ts_amd/lib/InflateSession.js)
// over cases prepared by tests/test_js_session.py: a stream pushed in pieces,
// only the new bytes each time.  Prints one JSON result per case; bytes travel
// as hex.
import fs from 'fs';
import { RawInflateSession } from '../../zlib.ts_amd/lib/index.js';

const hex = (s) => Uint8Array.from(Buffer.from(s, 'hex'));
const tohex = (a) => Buffer.from(a.buffer, a.byteOffset, a.length).toString('hex');
const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = [];
for (const c of cases) {
    const r = { id: c.id };
    try {
        const input = hex(c.in);
        if (c.op === 'session') {
            const s = new RawInflateSession();
            const parts = [];
            let prev = 0;
            c.cuts.forEach((cut, k) => {
                parts.push(s.push(input.subarray(prev, cut), k === c.cuts.length - 1));
                prev = cut;
            });
            r.calls = parts.map((p) => p.length);
            r.out = tohex(Buffer.concat(parts.map((p) => Buffer.from(p.buffer, p.byteOffset, p.length))));
            r.finished = s.finished;
            r.unused = s.unused;
            r.crc32 = s.crc32;
            r.adler32 = s.adler32;
            s.close();
            try {
                s.push(new Uint8Array(1));
                r.closed = false;
            } catch (e) {
                r.closed = true;
            }
        } else if (c.op === 'many') {
            // the same stream through two sessions fed in one call
            const ss = [new RawInflateSession(), new RawInflateSession()];
            const acc = [[], []];
            let prev = 0;
            c.cuts.forEach((cut, k) => {
                const res = RawInflateSession.pushMany(ss, [input.subarray(prev, cut), input.subarray(prev, cut)],
                    k === c.cuts.length - 1);
                res.forEach((x, i) => acc[i].push(Buffer.from(x.output.buffer, x.output.byteOffset, x.output.length)));
                prev = cut;
            });
            r.outs = acc.map((a) => tohex(Buffer.concat(a)));
            r.finished = ss.every((s) => s.finished);
            ss.forEach((s) => s.close());
        } else if (c.op === 'bad') {
            const s = new RawInflateSession();
            s.push(input, false);
        } else {
            throw new Error('unknown op ' + c.op);
        }
    } catch (e) {
        r.error = { message: typeof e === 'string' ? e : e.message, status: e.ztStatus };
    }
    out.push(r);
}
console.log(JSON.stringify(out));
