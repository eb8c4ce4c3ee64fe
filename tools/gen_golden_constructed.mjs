// tools/gen_golden_constructed.mjs -- what the REFERENCE's RawInflate does with
// the hand-built streams of tests/deflate_builder.py.
//
// Like tools/gen_golden.mjs: the reference's compiled JS (/root/reference/js)
// is copied to a throw-away directory under /tmp (never into this repository)
// with a package.json {"type":"module"} and the BitStream.js symlink, and only
// its OUTPUTS are written, to tests/golden/inflate_constructed.json.  Refuses
// to run when /root/reference is absent.
//
//   python tests/deflate_builder.py --dump /tmp/constructed
//   node tools/gen_golden_constructed.mjs /tmp/constructed [outfile]
//
// Every stream is decoded in a child process of its own with a time limit:
// on an incomplete code-length set the reference can loop for ever (its
// unassigned table entries decode as length 0), and such a case is recorded
// as "reference": "no result".  Records: case name, length and sha256 of the
// stream (its hex when it is at most 4 KiB), and either the output's length
// and sha256 with `.ip`, or the error text.
import fs from 'fs';
import os from 'os';
import path from 'path';
import crypto from 'crypto';
import url from 'url';
import { spawnSync } from 'child_process';

const REF = '/root/reference/js';
if (!fs.existsSync(REF)) {
  console.error('gen_golden_constructed: /root/reference is not present; refusing to run');
  process.exit(2);
}
const self = url.fileURLToPath(import.meta.url);
const sha = (b) => crypto.createHash('sha256').update(b).digest('hex');
const INLINE = 4096;
const LIMIT_MS = 30000;

async function child(shim, file) {
  const { RawInflate } = await import(url.pathToFileURL(path.join(shim, 'RawInflate.js')).href);
  const stream = new Uint8Array(fs.readFileSync(file));
  const rec = {};
  try {
    const ri = new RawInflate(stream);
    const o = ri.decompress();
    const b = Buffer.from(o.buffer, o.byteOffset, o.length);
    rec.out = { len: b.length, sha256: sha(b) };
    rec.ip = ri.ip;
  } catch (e) { rec.error = String(e.message || e); }
  process.stdout.write(JSON.stringify(rec));
}

function main() {
  const dir = process.argv[2];
  if (!dir || !fs.existsSync(path.join(dir, 'index.json'))) {
    console.error('usage: node tools/gen_golden_constructed.mjs DIR [outfile]   (DIR: deflate_builder.py --dump DIR)');
    process.exit(2);
  }
  const outfile = process.argv[3] || path.join(path.dirname(self), '..', 'tests', 'golden', 'inflate_constructed.json');
  const shim = fs.mkdtempSync(path.join(os.tmpdir(), 'zref-'));
  for (const f of fs.readdirSync(REF)) if (f.endsWith('.js')) fs.copyFileSync(path.join(REF, f), path.join(shim, f));
  fs.writeFileSync(path.join(shim, 'package.json'), '{"type":"module"}');
  fs.symlinkSync('Bitstream.js', path.join(shim, 'BitStream.js'));
  const records = [];
  for (const c of JSON.parse(fs.readFileSync(path.join(dir, 'index.json'), 'utf8'))) {
    const file = path.join(dir, c.name + '.bin');
    const data = fs.readFileSync(file);
    const rec = { name: c.name, stream: { len: data.length, sha256: sha(data) } };
    if (data.length <= INLINE) rec.stream.hex = data.toString('hex');
    const r = spawnSync(process.execPath, ['--max-old-space-size=2048', self, '--child', shim, file],
      { timeout: LIMIT_MS, maxBuffer: 1 << 20, encoding: 'utf8' });
    let got = null;
    try { got = JSON.parse(r.stdout); } catch (e) { got = null; }
    if (r.status === 0 && got) Object.assign(rec, got);
    else rec.reference = 'no result';
    records.push(rec);
  }
  fs.writeFileSync(outfile, JSON.stringify({ records }, null, 0).replace(/\},\{"name"/g, '},\n{"name"') + '\n');
  console.log('inflate_constructed:', records.length, 'records,', records.filter((r) => r.reference).length, 'without a result');
  fs.rmSync ? fs.rmSync(shim, { recursive: true, force: true }) : fs.rmdirSync(shim, { recursive: true });
}

if (process.argv[2] === '--child') child(process.argv[3], process.argv[4]).catch((e) => { console.error(e); process.exit(1); });
else main();
