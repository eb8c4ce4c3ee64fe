// Unzip with the reference's surface (src/Unzip.ts:196-342): getFilenames(),
// decompress(filename), getFileData(index), parseFileHeader(), verify.  The
// first call decodes the whole archive in libzt (zt_unzip): the central
// directory and local headers are parsed with the reference's checks and
// messages and every DEFLATE member is inflated in one GPU batch; each
// getFileData(i) then returns entry i or throws its error as the reference
// would.  The password option, setPassword and the per-call {password} of
// getFileData / decompress (src/Unzip.ts:263-282) decrypt ZipCrypto entries on
// the GPU (zt_unzip_pw); the decoded archive is cached per password, and unlike
// the reference the input is never written.
import native, { dflt, refError } from './native.js';
import { passwordBytes } from './Zip.js';

function readString(input, off, len) {
    let s = '';
    for (let i = 0; i < len; ++i) s += String.fromCharCode(input[off + i]);
    return s;
}

export class Unzip {
    constructor(input, opts = {}) {
        this.input = input instanceof Uint8Array ? input : new Uint8Array(input);
        this.ip = 0;
        this.EOCD = null;
        this.verify = !!opts.verify;
        if (opts.password) this.password = passwordBytes(opts.password);
        this.decoded = new Map();  // password (hex, '' for none) -> decoded archive
    }

    // `password` falsy: none, as the reference's `if (!password) throw`
    decode(password) {
        const pw = password ? passwordBytes(password) : null;
        const key = pw ? 'p' + Buffer.from(pw).toString('hex') : '';
        if (this.decoded.has(key)) return this.decoded.get(key);
        let r;
        try {
            r = native.unzip(this.input, this.verify, pw);
        } catch (e) {
            throw refError(e);
        }
        this.decoded.set(key, r);
        return r;
    }

    parseFileHeader() {
        if (this.fileHeaderList) return;
        const r = this.decode(this.password);
        const list = [];
        const table = {};
        r.entries.forEach((e, i) => {
            const fh = Object.assign({}, e);
            fh.filename = readString(this.input, e.nameOff, e.nameLen);
            fh.fileNameLength = e.nameLen;
            fh.comment = this.input.subarray(e.commentOff, e.commentOff + e.commentLen);
            fh.fileCommentLength = e.commentLen;
            list[i] = fh;
            table[fh.filename] = i;
        });
        this.fileHeaderList = list;
        this.filenameToIndex = table;
    }

    getFileData(index, opts = {}) {
        this.parseFileHeader();
        if (this.fileHeaderList[index] === undefined) throw new Error('wrong index');
        // src/Unzip.ts:265: the call's password, else the archive's
        const r = this.decode(dflt(opts.password, this.password));
        const e = r.entries[index];
        if (e.status !== 0) throw new Error(e.message);
        return r.output.subarray(e.dataOff, e.dataOff + e.dataLen);
    }

    getFilenames() {
        this.parseFileHeader();
        return this.fileHeaderList.map((e) => e.filename);
    }

    decompress(filename, opts = {}) {
        this.parseFileHeader();
        const index = this.filenameToIndex[filename];
        if (index === undefined) throw new Error(filename + ' not found');
        return this.getFileData(index, opts);
    }

    setPassword(password) {
        this.password = passwordBytes(password);
    }
}
