// BGZF (blocked gzip, SAM spec 4.1; include/zt_bgzf.h): BGZip writes a chain of
// independent gzip blocks of at most 64 KiB with the end marker, BGUnzip reads
// the whole file on an exact one-pass path, byte ranges and virtual-offset
// chunks by uploading and decoding only the blocks they touch, and builds the
// .gzi index.  This build's extra: the reference has no BGZF classes.
import native, { refError, dflt } from './native.js';

const u8 = (x) => (x instanceof Uint8Array ? x : new Uint8Array(x));
const call = (fn) => {
    try {
        return fn();
    } catch (e) {
        throw refError(e);
    }
};

export const BGZF_BLOCK_MAX = 65280;

// the virtual offset (a BigInt) of byte `uoffset` of the block at `coffset`
export const bgzfVirtualOffset = (coffset, uoffset) => (BigInt(coffset) << 16n) | BigInt(uoffset);

export class BGZip {
    // opts: {level, compressionType, blockSize (0 or 4096..65280), buildIndex}
    constructor(input, opts) {
        const o = opts || {};
        this.input = u8(input);
        this.level = dflt(o.level, -1);
        this.compressionType = dflt(o.compressionType, 2);
        this.blockSize = dflt(o.blockSize, 0);
        this.buildIndex = !!o.buildIndex;
        this.gzi = null;
    }

    compress() {
        const r = call(() => native.bgzfCompress(this.input, this.compressionType, this.level, this.blockSize,
            this.buildIndex));
        if (this.buildIndex) this.gzi = r.gzi;
        return r.output;
    }
}

export class BGUnzip {
    // opts: {gzi}: the file's .gzi (a Uint8Array); without one the range
    // calls walk the block chain on the host
    constructor(input, opts) {
        this.input = u8(input);
        this.gzi = opts && opts.gzi ? u8(opts.gzi) : null;
    }

    decompress() {
        return call(() => native.bgzfDecompress(this.input));
    }

    // the file's .gzi from a host walk (no decode); kept for the range calls
    buildIndex() {
        this.gzi = call(() => native.bgzfIndex(this.input));
        return this.gzi;
    }

    readRange(off, len) {
        return this.readRanges([[off, len]])[0];
    }

    // [[off, len], ...] by uncompressed offset, pread style; the first failing range throws
    readRanges(ranges) {
        const offs = Float64Array.from(ranges, (r) => r[0]);
        const lens = Float64Array.from(ranges, (r) => r[1]);
        return call(() => native.bgzfReadRanges(this.input, this.gzi, offs, lens));
    }

    // the bytes from virtual offset `beg` up to `end` (BigInts)
    readVirtual(beg, end) {
        return this.readVirtualChunks([[beg, end]])[0];
    }

    readVirtualChunks(chunks) {
        const begs = BigUint64Array.from(chunks, (c) => BigInt(c[0]));
        const ends = BigUint64Array.from(chunks, (c) => BigInt(c[1]));
        return call(() => native.bgzfReadVirtual(this.input, begs, ends));
    }
}
