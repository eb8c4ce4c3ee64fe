// GUnzip with the reference's surface (src/GUnzip.ts:6-203): decompress()
// returns every member's data concatenated, getMembers() the parsed headers.
// Header parsing, the DEFLATE bodies (segment-parallel when they carry
// restart points) and the CRC-32 checks run in libzt (zt_gunzip).
import native, { refError } from './native.js';

const latin1 = (u8) => {
    let s = '';
    for (let i = 0; i < u8.length; ++i) s += String.fromCharCode(u8[i]);
    return s;
};

// members of one native result as getMembers() shapes them (`input`: the
// bytes the offsets index, from `base`)
const shapeMembers = (input, base, r, onMember) => r.members.map((m) => {
    const member = {
        id1: 0x1f, id2: 0x8b, cm: 8, flg: m.flg, mtime: new Date(m.mtime * 1000), xfl: m.xfl, os: m.os,
        data: r.output.subarray(m.dataOff, m.dataOff + m.dataLen),
    };
    if (m.flg & 0x04) member.xlen = m.xlen;
    if (m.flg & 0x08) member.name = latin1(input.subarray(base + m.nameOff, base + m.nameOff + m.nameLen));
    if (m.flg & 0x10) {
        member.comment = latin1(input.subarray(base + m.commentOff, base + m.commentOff + m.commentLen));
    }
    if (m.crc16 >= 0) member.crc16 = m.crc16;
    if (onMember) onMember(m);
    return member;
});

// a failed item of a batch call as the Error decompress() would throw
export const batchError = (f) => {
    const e = new Error(f.message);
    e.ztStatus = f.status;
    return refError(e);
};

export class GUnzip {
    constructor(input) {
        this.input = input instanceof Uint8Array ? input : new Uint8Array(input);
        this.ip = 0;
        this.members = [];
        this.decompressed = false;
        this.crc32 = null;
    }

    getMembers() {
        if (!this.decompressed) this.decompress();
        return this.members.slice();
    }

    decompress() {
        let r;
        try {
            r = native.gunzip(this.input.subarray(this.ip));
        } catch (e) {
            throw refError(e);
        }
        this.members.push(...shapeMembers(this.input, this.ip, r, (m) => { this.crc32 = m.crc32; }));
        this.ip = this.input.length;
        this.decompressed = true;
        return r.output;
    }

    // Many gzip files in one call (zt_gunzip_batch): an array with, per
    // input, {output, members} -- members shaped as getMembers() -- or, for a
    // failed input, the Error decompress() would throw (returned, not
    // thrown; the other inputs still decode).  This build's extra: the
    // reference has no batch call.
    static decompressBatch(inputs) {
        const ins = Array.from(inputs, (x) => (x instanceof Uint8Array ? x : new Uint8Array(x)));
        let rs;
        try {
            rs = native.gunzipBatch(ins);
        } catch (e) {
            throw refError(e);
        }
        return rs.map((r, i) => (r.status !== undefined ? batchError(r)
            : { output: r.output, members: shapeMembers(ins[i], 0, r) }));
    }
}
