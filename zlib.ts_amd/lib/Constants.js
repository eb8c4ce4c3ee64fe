// Mirrors src/Constants.ts:1-24 of the reference (values used by the facade).
export const CompressionType = { NONE: 0, FIXED: 1, DYNAMIC: 2 };
// deflate strategies (include/zt_strategy.h; zlib's numbers): this build's
// extra option, the reference has none
export const Strategy = { DEFAULT: 0, HUFFMAN_ONLY: 2, RLE: 3 };
export const BufferType = { BLOCK: 0, ADAPTIVE: 1 };
export const DefaultBufferSize = 0x8000;
export const DefaultDeflateBufferSize = 0x8000;
export const DefaultInflateBufferSize = 0x8000;
export const MaxBackwardLength = 32768;
export const MaxCopyLength = 258;
