// Runs GUnzipSession / ZlibInflateSession of the JS facade
// (zlib.ts_amd/lib/ContainerSession.js) over cases prepared by
// tests/test_js_container_session.py: a gzip file or a zlib stream pushed in
// pieces, only the new bytes each time.  Prints one JSON result per case;
// bytes travel as hex.
import fs from 'fs';
import { GUnzipSession, ZlibInflateSession } from '../../zlib.ts_amd/lib/index.js';

const hex = (s) => Uint8Array.from(Buffer.from(s, 'hex'));
const buf = (a) => Buffer.from(a.buffer, a.byteOffset, a.length);
const tohex = (a) => buf(a).toString('hex');
const make = (c) => (c.kind === 'gzip' ? new GUnzipSession()
    : new ZlibInflateSession({ dictionary: c.dict ? hex(c.dict) : undefined, verify: c.verify !== false }));
const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = [];
for (const c of cases) {
    const r = { id: c.id };
    try {
        const input = hex(c.in);
        if (c.op === 'session') {
            const s = make(c);
            const parts = [];
            let prev = 0;
            c.cuts.forEach((cut, k) => {
                parts.push(s.push(input.subarray(prev, cut), k === c.cuts.length - 1));
                prev = cut;
            });
            r.calls = parts.map((p) => p.length);
            r.out = tohex(Buffer.concat(parts.map(buf)));
            r.finished = s.finished;
            r.unused = s.unused;
            r.members = s.members.map((m) => ({
                flg: m.flg, mtime: m.mtime, crc32: m.crc32, isize: m.isize, dataOff: m.dataOff, dataLen: m.dataLen,
                inOff: m.inOff, name: m.name ? tohex(m.name) : null, comment: m.comment ? tohex(m.comment) : null,
            }));
            s.close();
            try {
                s.push(new Uint8Array(1));
                r.closed = false;
            } catch (e) {
                r.closed = true;
            }
        } else if (c.op === 'many') {
            // a gzip and a zlib session fed in one call
            const inputs = [input, hex(c.in2)];
            const ss = [new GUnzipSession(), new ZlibInflateSession()];
            const acc = [[], []];
            for (let k = 0; k < c.rounds; ++k) {
                const chunks = inputs.map((x) => x.subarray(Math.floor(x.length * k / c.rounds),
                    Math.floor(x.length * (k + 1) / c.rounds)));
                const res = GUnzipSession.pushMany(ss, chunks, k === c.rounds - 1);
                res.forEach((x, i) => acc[i].push(buf(x.output)));
                r.statuses = res.map((x) => x.status || 0);
            }
            r.outs = acc.map((a) => tohex(Buffer.concat(a)));
            r.finished = ss.every((s) => s.finished);
            ss.forEach((s) => s.close());
        } else if (c.op === 'bad') {
            const s = make(c);
            s.push(input, true);
        } else {
            throw new Error('unknown op ' + c.op);
        }
    } catch (e) {
        r.error = { message: typeof e === 'string' ? e : e.message, status: e.ztStatus };
        if (e.output) r.errorOutput = tohex(e.output);
    }
    out.push(r);
}
console.log(JSON.stringify(out));
