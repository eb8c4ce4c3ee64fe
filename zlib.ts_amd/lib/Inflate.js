// zlib Inflate with the reference's surface (src/Inflate.ts:15-93): the
// constructor validates CMF/FLG and throws the reference's errors;
// decompress() inflates on the GPU and, with `verify`, checks the Adler-32
// (libzt zt_zlib_decompress).  `ip` is the reference's: past the stream.
import native, { dflt, refError } from './native.js';
import { batchError } from './GUnzip.js';

export class Inflate {
    constructor(input, opts = {}) {
        this.input = input instanceof Uint8Array ? input : new Uint8Array(input);
        this.index = dflt(opts.index, 0);
        this.ip = this.index;
        this.verify = dflt(opts.verify, false);
        this.adler32 = undefined;
        // preset dictionary (Uint8Array), named as in Node's zlib; this build's
        // extra option: the reference has none
        this.dictionary = opts.dictionary == null ? undefined
            : opts.dictionary instanceof Uint8Array ? opts.dictionary : new Uint8Array(opts.dictionary);
        const cmf = this.input[this.ip++];
        const flg = this.input[this.ip++];
        if ((cmf & 0x0f) != 8) throw new Error('unsupported compression method');
        if (((cmf << 8) + flg) % 31 !== 0) throw new Error('invalid fcheck flag:' + ((cmf << 8) + flg) % 31);
        // (with the `dictionary` option an FDICT stream is decoded: zt_zlib_decompress_dict)
        if ((flg & 0x20) && !(this.dictionary && this.dictionary.length)) throw new Error('fdict flag is not supported');
    }

    decompress() {
        let r;
        try {
            r = native.zlibDecompress(this.input, this.index, this.verify, this.dictionary);
        } catch (e) {
            throw refError(e);
        }
        this.ip = r.ip;
        if (this.verify) this.adler32 = r.adler32;
        return r.output;
    }

    // Many zlib streams in one call (zt_zlib_decompress_batch, with
    // `dictionary` zt_zlib_decompress_batch_dict): an array with, per input,
    // {output, ip, adler32} (adler32 only with `verify`) or, for a failed
    // input, the Error the constructor or decompress() would throw (returned,
    // not thrown).  This build's extra: the reference has no batch call.
    static decompressBatch(inputs, opts = {}) {
        const ins = Array.from(inputs, (x) => (x instanceof Uint8Array ? x : new Uint8Array(x)));
        const verify = dflt(opts.verify, false);
        const dict = opts.dictionary == null ? undefined
            : opts.dictionary instanceof Uint8Array ? opts.dictionary : new Uint8Array(opts.dictionary);
        let rs;
        try {
            rs = native.zlibDecompressBatch(ins, verify, dict);
        } catch (e) {
            throw refError(e);
        }
        return rs.map((r) => {
            if (r.status !== undefined) return batchError(r);
            const o = { output: r.output, ip: r.ip };
            if (verify) o.adler32 = r.adler32;
            return o;
        });
    }
}
