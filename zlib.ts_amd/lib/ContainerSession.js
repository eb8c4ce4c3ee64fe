// GUnzipSession / ZlibInflateSession: a gzip file (any number of members) or
// a zlib stream (FDICT included) pushed chunk by chunk through a container
// session of the engine (include/zt_stream_container.h).  push(chunk, last)
// takes only the new bytes and returns the bytes they complete; headers and
// trailers are followed on the host, every body is decoded by the inflate
// sessions' kernel, and the checks and error texts are those of GUnzip /
// Inflate on the whole input.  pushMany feeds many sessions in one call.
import native, { refError } from './native.js';

const asU8 = (x) => (x instanceof Uint8Array ? x : new Uint8Array(x || 0));
const FORMAT_GZIP = 1;
const FORMAT_ZLIB = 2;

class ContainerSession {
    constructor(format, dictionary, verify) {
        try {
            this._s = native.containerSessionCreate(format, dictionary ? asU8(dictionary) : undefined, verify ? 1 : 0);
        } catch (e) {
            throw refError(e);
        }
    }

    // Feeds the new bytes; last: no more input will come.  Returns this call's
    // output.  The error it throws carries `output`: the bytes this call decoded
    // before the error (the members in front of a corrupt one, for example).
    push(chunk, last = false) {
        if (!this._s) throw new Error('the session is closed');
        try {
            return native.containerSessionFeed(this._s, asU8(chunk), last ? 1 : 0);
        } catch (e) {
            const err = refError(e);
            err.output = e.output || new Uint8Array(0);
            throw err;
        }
    }

    // chunk i to session i in one call (gzip and zlib sessions may be mixed);
    // last: one flag or one per session.  Returns [{output} | {status, message, output}].
    static pushMany(sessions, chunks, last = false) {
        const flags = Array.isArray(last) ? last.map(Boolean) : Boolean(last);
        return native.containerSessionsFeed(sessions.map((s) => s._s), chunks.map(asU8), flags);
    }

    info() {
        if (!this._s) throw new Error('the session is closed');
        return native.containerSessionInfo(this._s);
    }

    // the members whose trailer was checked: header fields, name / comment
    // bytes, dataOff / dataLen in the total output, inOff in the total input
    get members() { return this.info().members; }
    get finished() { return this.info().finished; }
    // zlib: fed bytes behind the Adler-32
    get unused() { return this.info().unused; }

    close() {
        if (this._s) native.containerSessionDestroy(this._s);
        this._s = null;
    }
}

export class GUnzipSession extends ContainerSession {
    constructor(opts = {}) {
        super(FORMAT_GZIP, undefined, opts.verify !== false);
    }
}

export class ZlibInflateSession extends ContainerSession {
    // opts.dictionary: used when the stream carries FDICT; opts.verify: compare the Adler-32 (default true)
    constructor(opts = {}) {
        super(FORMAT_ZLIB, opts.dictionary, opts.verify !== false);
    }
}
