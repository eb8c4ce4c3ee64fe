// RawInflateSession: raw inflate fed chunk by chunk through an inflate session
// of the engine (include/zt_stream.h).  push(chunk, last) takes only the new
// bytes and returns the bytes they complete: decoding resumes at a token, so
// output arrives while a block is still incomplete (RawInflateStream decodes
// whole blocks from the whole input received so far).  The session's state --
// the 32 KiB history, the block being decoded, the checksums -- stays on the
// device; one session decodes at the rate of one wavefront, and
// RawInflateSession.pushMany feeds many sessions in one call.
import native, { refError } from './native.js';

const asU8 = (x) => (x instanceof Uint8Array ? x : new Uint8Array(x || 0));

export class RawInflateSession {
    // window: preset history (a raw-deflate dictionary), optional
    constructor(window) {
        try {
            this._s = native.sessionCreate(window ? asU8(window) : undefined);
        } catch (e) {
            throw refError(e);
        }
    }

    // Feeds the new bytes; last: no more input will come.  Returns this call's output.
    push(chunk, last = false) {
        if (!this._s) throw new Error('the session is closed');
        try {
            return native.sessionFeed(this._s, asU8(chunk), last ? 1 : 0);
        } catch (e) {
            throw refError(e);
        }
    }

    // chunk i to session i in one call (one wavefront per session); last: one
    // flag or one per session.  Returns [{output} | {status, message}].
    static pushMany(sessions, chunks, last = false) {
        const flags = Array.isArray(last) ? last.map(Boolean) : Boolean(last);
        return native.sessionsFeed(sessions.map((s) => s._s), chunks.map(asU8), flags);
    }

    info() {
        if (!this._s) throw new Error('the session is closed');
        return native.sessionInfo(this._s);
    }

    get finished() { return this.info().finished; }
    // fed bytes behind the stream's end (a container's trailer)
    get unused() {
        const i = this.info();
        return i.totalIn - Math.ceil(i.endBits / 8);
    }
    get crc32() { return this.info().crc32; }
    get adler32() { return this.info().adler32; }

    close() {
        if (this._s) native.sessionDestroy(this._s);
        this._s = null;
    }
}
