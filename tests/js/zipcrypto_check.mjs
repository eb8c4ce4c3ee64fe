// Runs the password paths of the JS facade (zlib.ts_amd/lib Zip / Unzip) over
// cases prepared by tests/test_js_zipcrypto.py and prints one JSON result per
// case.  Passwords travel as hex (bytes) or as `str` (a JS string).
import fs from 'fs';
import { Zip, Unzip } from '../../zlib.ts_amd/lib/index.js';

const hex = (s) => Uint8Array.from(Buffer.from(s, 'hex'));
const tohex = (a) => Buffer.from(a.buffer, a.byteOffset, a.length).toString('hex');
const pw = (p) => (p === undefined || p === null) ? undefined : (p.str !== undefined ? p.str : hex(p.hex));
const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = [];
for (const c of cases) {
    const r = { id: c.id };
    try {
        if (c.op === 'zip') {
            // c.files: [{fn, in (hex), opts, password?}], c.password: the archive's
            const z = new Zip(c.comment || []);
            if (pw(c.password) !== undefined) z.setPassword(pw(c.password));
            for (const f of c.files) {
                const o = Object.assign({}, f.opts, { date: new Date(...c.date) });
                if (pw(f.password) !== undefined) o.password = pw(f.password);
                if (f.cryptLead !== undefined) o.cryptLead = hex(f.cryptLead);
                z.addFile(hex(f.in), f.fn, o);
            }
            r.out = tohex(z.compress());
        } else if (c.op === 'unzip') {
            // c.ctor: constructor password, c.set: setPassword, c.each[i]: getFileData(i, {password})
            const input = hex(c.in);
            const opts = { verify: !!c.verify };
            if (pw(c.ctor) !== undefined) opts.password = pw(c.ctor);
            const u = new Unzip(input, opts);
            if (pw(c.set) !== undefined) u.setPassword(pw(c.set));
            r.names = u.getFilenames();
            r.files = r.names.map((nm, i) => {
                try {
                    const o = c.each && pw(c.each[i]) !== undefined ? { password: pw(c.each[i]) } : {};
                    const d = c.byName ? u.decompress(nm, o) : u.getFileData(i, o);
                    return { ok: true, out: tohex(d) };
                } catch (e) {
                    return { ok: false, message: e.message };
                }
            });
            r.inputSame = tohex(input) === c.in;
        } else {
            throw new Error('unknown op ' + c.op);
        }
    } catch (e) {
        r.error = { message: e.message, status: e.ztStatus };
    }
    out.push(r);
}
console.log(JSON.stringify(out));
