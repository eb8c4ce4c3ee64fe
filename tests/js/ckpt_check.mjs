// Runs the checkpoint methods of the JS facade (zlib.ts_amd/lib RawInflate:
// buildCheckpoints / decompressRangeAt / decompressRangesAt) over cases
// prepared by tests/test_js_ckpt.py and prints one JSON result per case.
// Streams come from files (they are megabytes); results travel as hex.
import fs from 'fs';
import { RawInflate, ZT } from '../../zlib.ts_amd/lib/index.js';

const tohex = (a) => Buffer.from(a.buffer, a.byteOffset, a.length).toString('hex');
const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = [];
for (const c of cases) {
    const r = { id: c.id };
    try {
        const input = Uint8Array.from(fs.readFileSync(c.file));
        const x = new RawInflate(input, c.opts || {});
        const blob = c.blobFile ? Uint8Array.from(fs.readFileSync(c.blobFile)) : x.buildCheckpoints(c.build || {});
        r.blobLength = blob.length;
        r.magic = Buffer.from(blob.buffer, blob.byteOffset, 4).toString('latin1');
        r.nunits = new DataView(blob.buffer, blob.byteOffset).getUint32(8, true);
        r.nwin = new DataView(blob.buffer, blob.byteOffset).getUint32(12, true);
        if (c.range) r.range = tohex(x.decompressRangeAt(blob, c.range[0], c.range[1]));
        if (c.ranges) r.ranges = x.decompressRangesAt(blob, c.ranges).map(tohex);
        r.ip = x.ip;
    } catch (e) {
        r.error = { message: typeof e === 'string' ? e : e.message, status: e.ztStatus };
    }
    out.push(r);
}
console.log(JSON.stringify({ results: out, codes: [ZT.NO_INDEX, ZT.INDEX, ZT.INDEX_MISMATCH] }));
