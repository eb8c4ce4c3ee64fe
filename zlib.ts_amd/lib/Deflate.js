// zlib Deflate with the reference's surface (src/Deflate.ts:16-99): CMF/FLG
// (FLEVEL = compressionType), raw DEFLATE and the big-endian Adler-32, built
// by libzt (zt_zlib_compress) from one device copy of the input.
import native, { dflt, refError, strategyAlone } from './native.js';
import { CompressionType } from './Constants.js';

export class Deflate {
    constructor(input, opts = {}) {
        this.input = input instanceof Uint8Array ? input : new Uint8Array(input);
        this.output = new Uint8Array(0x8000);
        this.compressionType = dflt(opts.compressionType, CompressionType.DYNAMIC);
        this.lazy = dflt(opts.lazy, 0);
        this.level = dflt(opts.level, 6);
        // this build's extra option: Strategy.RLE / Strategy.HUFFMAN_ONLY (include/zt_strategy.h)
        this.strategy = opts.strategy == null ? undefined : opts.strategy;
        // preset dictionary (Uint8Array), named as in Node's zlib; this build's
        // extra option: the reference has none
        this.dictionary = opts.dictionary == null ? undefined
            : opts.dictionary instanceof Uint8Array ? opts.dictionary : new Uint8Array(opts.dictionary);
        this.adler32 = undefined;
        // this build's extra option: buildIndex: true leaves the stream's range
        // index (include/zt_index.h) in streamIndex after compress(); the stream
        // and the blob go straight into RawInflate.decompressRange.  Not with a
        // preset dictionary: the range path has none.
        this.buildIndex = dflt(opts.buildIndex, false);
        this.streamIndex = undefined;
    }

    static compress(input, opts) {
        return new Deflate(input, opts).compress();
    }

    compress() {
        let r;
        try {
            strategyAlone(this.strategy, this.dictionary, this.buildIndex);
            if (this.buildIndex) {
                if (this.dictionary !== undefined) {
                    const err = new Error('an indexed stream cannot use a preset dictionary');
                    err.ztStatus = -103;
                    throw err;
                }
                r = native.zlibCompressIndexed(this.input, this.compressionType, this.lazy, this.level);
                this.streamIndex = r.index;
            } else {
                r = native.zlibCompress(this.input, this.compressionType, this.lazy, this.level, this.dictionary, this.strategy);
            }
        } catch (e) {
            if (e.ztStatus === -1) throw 'invalid compression type';
            throw refError(e);
        }
        this.adler32 = r.adler32;
        this.output = r.output;
        return r.output;
    }
}
