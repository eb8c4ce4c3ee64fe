// RawInflate with the reference's surface (src/RawInflate.ts:63-143): same
// options (index, bufferSize, bufferType, resize) and public fields (ip, op,
// buffer, output); decoding runs in libzt on the GPU (zt_inflate_raw).
// `refStrict: true` reproduces the reference's over-strict end-of-input check
// (src/RawInflate.ts:187) and its exact `ip` bookkeeping.
import native, { dflt, refError } from './native.js';
import { BufferType, DefaultInflateBufferSize } from './Constants.js';

export { BufferType };

export class RawInflate {
    constructor(input, opts = {}) {
        this.input = input instanceof Uint8Array ? input : new Uint8Array(input);
        this.ip = dflt(opts.index, 0);
        this.streamStart = this.ip;  // where the stream starts (buildIndex: decompress() moves ip)
        this.bufferSize = dflt(opts.bufferSize, DefaultInflateBufferSize);
        this.bufferType = dflt(opts.bufferType, BufferType.ADAPTIVE);
        this.resize = dflt(opts.resize, false);
        this.refStrict = dflt(opts.refStrict, false);
        // preset dictionary (Uint8Array), named as in Node's zlib; this build's
        // extra option: the reference has none
        this.dictionary = opts.dictionary == null ? undefined
            : opts.dictionary instanceof Uint8Array ? opts.dictionary : new Uint8Array(opts.dictionary);
        this.buffer = null;
        this.output = new Uint8Array(0);
        this.op = 0;
    }

    decompress() {
        if (this.bufferType !== BufferType.BLOCK && this.bufferType !== BufferType.ADAPTIVE) {
            throw new Error('invalid inflate mode');
        }
        let r;
        try {
            r = native.inflateRaw(this.input, this.ip, this.bufferType, this.bufferSize, this.refStrict,
                                  this.dictionary);
        } catch (e) {
            // libzt's message is the reference's text ('input buffer is broken', ...)
            throw new Error(e.message);
        }
        this.ip = r.ip;
        this.output = r.output;
        this.op = r.output.length;
        this.buffer = r.output;
        return r.output;
    }

    // Indexed random access (include/zt_index.h; this build's extension: the
    // reference has none).  buildIndex() decodes the stream once and returns
    // its index blob (a Uint8Array that may be stored); decompressRange /
    // decompressRanges then decode only what the ranges need.  All three start
    // at the constructor's `index` option and leave ip / output untouched.
    // A stream without sync points throws 'stream has no usable sync points'
    // (ztStatus -60); decode it with decompress().
    buildIndex() {
        try {
            return native.inflateIndexBuild(this.input, this.streamStart);
        } catch (e) {
            throw refError(e);
        }
    }

    decompressRange(indexBlob, offset, length) {
        return this.decompressRanges(indexBlob, [[offset, length]])[0];
    }

    // ranges: [[offset, length], ...] (pread semantics: a length is clamped to
    // the end of the output, an offset past it throws) -> Uint8Array[]
    decompressRanges(indexBlob, ranges) {
        const off = new Float64Array(ranges.length), len = new Float64Array(ranges.length);
        for (let i = 0; i < ranges.length; i++) {
            off[i] = ranges[i][0];
            len[i] = ranges[i][1];
        }
        try {
            return native.inflateRanges(this.input, indexBlob, off, len);
        } catch (e) {
            throw refError(e);
        }
    }

    // Checkpoint index (include/zt_checkpoint.h): random access into streams
    // WITHOUT sync points -- what zlib, pigz, Python and Node write, and the
    // reference's own one-block output.  buildCheckpoints() decodes the stream
    // once and returns its checkpoint blob (a Uint8Array that may be stored;
    // span: output bytes between window checkpoints, default 1 MiB, at least
    // 64 KiB); decompressRangeAt / decompressRangesAt then decode only from the
    // last window checkpoint before a range.  Same conventions as the three
    // methods above; the two kinds of blob are not interchangeable (ztStatus -61).
    buildCheckpoints(opts = {}) {
        try {
            return native.inflateCkptBuild(this.input, this.streamStart, dflt(opts.span, 0));
        } catch (e) {
            throw refError(e);
        }
    }

    decompressRangeAt(blob, offset, length) {
        return this.decompressRangesAt(blob, [[offset, length]])[0];
    }

    decompressRangesAt(blob, ranges) {
        const off = new Float64Array(ranges.length), len = new Float64Array(ranges.length);
        for (let i = 0; i < ranges.length; i++) {
            off[i] = ranges[i][0];
            len[i] = ranges[i][1];
        }
        try {
            return native.inflateCkptRanges(this.input, blob, off, len);
        } catch (e) {
            throw refError(e);
        }
    }
}
