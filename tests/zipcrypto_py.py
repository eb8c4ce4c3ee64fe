"""ZipCrypto restated in pure Python (src/ZipCrypto.ts; APPNOTE 6.1) and a
small zip builder -- the checker of the password tests, pinned to the
reference's fixtures by tests/test_zipcrypto_ref.py.  About 2 s per MiB."""
import struct
import zlib

TABLE = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ (0xEDB88320 if _c & 1 else 0)
    TABLE.append(_c)


def crypt(password, data, decrypt=False):
    """encode (or decode) `data` under the key of `password` (bytes)."""
    k0, k1, k2 = 305419896, 591751049, 878082192
    out = bytearray()
    for i, b in enumerate(bytes(password) + bytes(data)):
        t = (k2 & 0xFFFF) | 2
        ks = ((t * (t ^ 1)) >> 8) & 0xFF
        p = b ^ ks if decrypt and i >= len(password) else b
        if i >= len(password):
            out.append(b ^ ks)
        k0 = TABLE[(k0 ^ p) & 0xFF] ^ (k0 >> 8)
        k1 = ((k1 + (k0 & 0xFF)) * 134775813 + 1) & 0xFFFFFFFF
        k2 = TABLE[(k2 ^ (k1 >> 24)) & 0xFF] ^ (k2 >> 8)
    return bytes(out)


def header(crc, mode=0, lead=bytes(10)):
    """Plaintext of the 12-byte encryption header: mode 0 as src/Zip.ts:169-174
    writes it, mode 1 with the CRC's high bytes (what other tools check)."""
    tail = [(crc >> 16) & 0xFF, (crc >> 24) & 0xFF] if mode else [(crc >> 8) & 0xFF, crc & 0xFF]
    return bytes(lead) + bytes(tail)


def build_zip(entries):
    """entries: dicts with name, data, method (0 | 8), and optionally password,
    mode, lead, dd (data descriptor: local CRC and sizes 0, flag bit 3)."""
    lo, cd = b"", b""
    for e in entries:
        data, name = bytes(e["data"]), bytes(e["name"])
        crc = zlib.crc32(data)
        body = data
        if e["method"] == 8:
            co = zlib.compressobj(6, zlib.DEFLATED, -15)
            body = co.compress(data) + co.flush()
        pw = e.get("password")
        if pw is not None:
            body = crypt(pw, header(crc, e.get("mode", 0), e.get("lead", bytes(10))) + body)
        flags = (1 if pw is not None else 0) | (8 if e.get("dd") else 0)
        sizes = (0, 0, 0) if e.get("dd") else (crc, len(body), len(data))
        off = len(lo)
        lo += struct.pack("<4sHHHHHIIIHH", b"PK\x03\x04", 20, flags, e["method"], 0, 0x21, *sizes, len(name), 0) + name
        lo += body + (struct.pack("<4sIII", b"PK\x07\x08", crc, len(body), len(data)) if e.get("dd") else b"")
        cd += struct.pack("<4sBBHHHHHIIIHHHHHII", b"PK\x01\x02", 20, 3, 20, flags, e["method"], 0, 0x21, crc,
                          len(body), len(data), len(name), 0, 0, 0, 0, 0, off) + name
    return lo + cd + struct.pack("<4sHHHHIIH", b"PK\x05\x06", 0, 0, len(entries), len(entries), len(cd), len(lo), 0)
