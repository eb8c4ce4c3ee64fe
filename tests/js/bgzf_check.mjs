// Runs the BGZF classes of the JS facade (zlib.ts_amd/lib BGZF.js: BGZip,
// BGUnzip) over cases prepared by tests/test_js_bgzf.py and prints one JSON
// result per case.  Inputs come from files; results travel as SHA-256 (whole
// files) or hex (ranges).  Virtual offsets arrive as decimal strings (BigInt).
import crypto from 'crypto';
import fs from 'fs';
import { BGZip, BGUnzip, bgzfVirtualOffset, ZT } from '../../zlib.ts_amd/lib/index.js';

const tohex = (a) => Buffer.from(a.buffer, a.byteOffset, a.length).toString('hex');
const sha = (a) => crypto.createHash('sha256').update(Buffer.from(a.buffer, a.byteOffset, a.length)).digest('hex');
const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = [];
for (const c of cases) {
    const r = { id: c.id };
    try {
        const input = Uint8Array.from(fs.readFileSync(c.file));
        if (c.compress) {
            const z = new BGZip(input, Object.assign({ buildIndex: true }, c.compress));
            const f = z.compress();
            r.file = sha(f);
            r.gzi = sha(z.gzi);
            r.plainHasNoIndex = new BGZip(input, c.compress).gzi === null;
            const u = new BGUnzip(f, { gzi: z.gzi });
            r.roundTrip = sha(u.decompress()) === sha(input);
        } else {
            const u = new BGUnzip(input);
            if (c.decompress) r.output = sha(u.decompress());
            if (c.ranges) r.walked = u.readRanges(c.ranges).map(tohex);
            r.built = sha(u.buildIndex());
            if (c.ranges) r.indexed = u.readRanges(c.ranges).map(tohex);
            if (c.range) r.range = tohex(u.readRange(c.range[0], c.range[1]));
            if (c.virtual) {
                r.virtual = c.virtual.map((v) => tohex(u.readVirtual(BigInt(v[0]), BigInt(v[1]))));
                r.chunks = u.readVirtualChunks(c.virtual).map(tohex);
            }
        }
    } catch (e) {
        r.error = { message: typeof e === 'string' ? e : e.message, status: e.ztStatus };
    }
    out.push(r);
}
console.log(JSON.stringify({
    results: out, codes: [ZT.BGZF_FORMAT, ZT.BGZF_INDEX],
    voffset: bgzfVirtualOffset(70000, 123).toString(),
}));
