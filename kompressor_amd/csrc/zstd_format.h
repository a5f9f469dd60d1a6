// zstd_format.h -- the framing of RFC 8878, from bytes to fields, and nothing else: no status codes, no LDS, no lanes, no kernels.
// Every function is pure: bytes plus a bound in, fields out; none reads at or beyond the bound it is given, and none knows its caller.
// What a field means to a walker (which error, stop staging, which sort key) and the order of its checks are the walker's business
// (zstd_decode.h, zstd_predecode.h, zstd_frame_info.h).  Compiled by hipcc for device and host and by g++ for tests/emu/.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define ZF_HD __host__ __device__ inline
#else
#define ZF_HD static inline
#endif

#define ZF_MAGIC        0xFD2FB528u
#define ZF_SKIP_MAGIC   0x184D2A50u            // ... to 0x184D2A5F: a skippable frame (magic, 4-byte size, payload)
#define ZF_SKIP_MASK    0xFFFFFFF0u
#define ZF_BLOCK_MAX    (128u << 10)           // a block's content, and so a block's literals, at most

ZF_HD uint32_t zf_ld16(const uint8_t* p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }
ZF_HD uint32_t zf_ld24(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }
ZF_HD uint32_t zf_ld32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }

// a little-endian field of n = 0 .. 8 bytes
ZF_HD uint64_t zf_le(const uint8_t* p, uint32_t n)
{
    if (n == 8) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
    if (n == 4) return zf_ld32(p);
    uint64_t v = 0;
    for (uint32_t k = 0; k < n; k++) v |= (uint64_t)p[k] << (8 * k);
    return v;
}

// ---- frame header: magic (4), descriptor (1), [window (1)], [dictionary ID (0, 1, 2, 4)], [content size (0, 1, 2, 4, 8)] ----
struct ZfDescriptor { uint32_t single, checksum, reserved, did_bytes, fcs_bytes, header_size; };      // header_size: 6 .. 18, the magic included
ZF_HD ZfDescriptor zf_descriptor(uint32_t fhd)
{
    ZfDescriptor d; uint32_t const did_code = fhd & 3u, fcs_code = fhd >> 6;
    d.single = (fhd >> 5) & 1u; d.checksum = (fhd >> 2) & 1u; d.reserved = (fhd >> 3) & 1u;
    d.did_bytes = did_code == 3u ? 4u : did_code; d.fcs_bytes = fcs_code ? 1u << fcs_code : d.single;
    d.header_size = 5u + (d.single ^ 1u) + d.did_bytes + d.fcs_bytes;
    return d;
}
struct ZfWindow { uint32_t log; uint64_t size; };            // log: 10 .. 41 (the decoders here refuse what is above 31)
ZF_HD ZfWindow zf_window(uint32_t window_byte)
{
    ZfWindow w; w.log = 10u + (window_byte >> 3); w.size = 1ull << w.log; w.size += (w.size >> 3) * (window_byte & 7u);
    return w;
}
// the content size field of fcs_bytes = 1, 2, 4, 8 bytes (the 2-byte form counts from 256)
ZF_HD uint64_t zf_content_size(const uint8_t* p, uint32_t fcs_bytes) { return zf_le(p, fcs_bytes) + (fcs_bytes == 2u ? 256u : 0u); }
// the most bytes a compressed block of the frame may take: min(window size, 128 KiB); a single-segment frame's window is its content
// size.  hdr: the frame's magic; d.header_size bytes lie there.
ZF_HD uint32_t zf_block_max(const uint8_t* hdr, ZfDescriptor d)
{
    uint64_t const w = d.single ? zf_content_size(hdr + 5 + d.did_bytes, d.fcs_bytes) : zf_window(hdr[5]).size;
    return w < ZF_BLOCK_MAX ? (uint32_t)w : ZF_BLOCK_MAX;
}

// ---- block header: 3 bytes.  type: 0 raw, 1 RLE (size = the run; one byte follows), 2 compressed, 3 reserved ----
struct ZfBlock { uint32_t last, type, size; };
ZF_HD ZfBlock zf_block(const uint8_t* p)
{
    uint32_t const bh = zf_ld24(p); ZfBlock b; b.last = bh & 1u; b.type = (bh >> 1) & 3u; b.size = bh >> 3;
    return b;
}

// ---- literals section header: the first 1 .. 5 of the block's `avail` bytes ----
// type: 0 raw, 1 RLE, 2 Huffman-coded, 3 Huffman-coded with the previous block's tree.  fits = 0: the header's own bytes (1, 2 or 3 for
// raw / RLE; 5 for the coded types, whatever their size format, as ZSTD_decodeLiteralsBlock asks) exceed avail, and only `type` means
// anything.  section: the whole section's bytes, header included (raw: the literals; RLE: one byte).  comp = 0, streams = 1 for raw / RLE.
struct ZfLiterals { uint32_t fits, type, header, regen, comp, streams, section; };
ZF_HD ZfLiterals zf_literals(const uint8_t* p, uint32_t avail)
{
    ZfLiterals l; l.fits = 0; l.type = 0; l.header = 0; l.regen = 0; l.comp = 0; l.streams = 1; l.section = 0;
    if (avail < 1u) return l;
    uint32_t const b0 = p[0], sf = (b0 >> 2) & 3u; l.type = b0 & 3u;
    if (l.type < 2u) {
        l.header = (sf & 1u) ? (sf == 1u ? 2u : 3u) : 1u;
        if (avail < l.header) return l;
        l.regen = l.header == 1u ? b0 >> 3 : l.header == 2u ? zf_ld16(p) >> 4 : zf_ld24(p) >> 4;
        l.section = l.header + (l.type == 0u ? l.regen : 1u);
    } else {
        l.header = sf < 2u ? 3u : sf + 2u;
        if (avail < 5u) return l;
        uint32_t const w = zf_ld32(p);
        if (sf < 2u) { l.regen = (w >> 4) & 0x3FFu; l.comp = (w >> 14) & 0x3FFu; l.streams = sf ? 4u : 1u; }
        else if (sf == 2u) { l.regen = (w >> 4) & 0x3FFFu; l.comp = w >> 18; l.streams = 4u; }
        else { l.regen = (w >> 4) & 0x3FFFFu; l.comp = (w >> 22) + ((uint32_t)p[4] << 10); l.streams = 4u; }
        l.section = l.header + l.comp;
    }
    l.fits = 1; return l;
}

// ---- sequences section header: the count in 1, 2 or 3 bytes from p[pos], then -- unless the count is 0 -- the modes byte ----
// have_count / have_modes: the bytes lie below `end`.  next: the position behind what was read.
struct ZfSequences { uint32_t have_count, have_modes, count, modes, next; };
ZF_HD ZfSequences zf_sequences(const uint8_t* p, uint32_t pos, uint32_t end)
{
    ZfSequences s; s.have_count = 0; s.have_modes = 0; s.count = 0; s.modes = 0; s.next = pos;
    if (pos >= end) return s;
    uint32_t const b0 = p[pos], n = b0 < 128u ? 1u : b0 < 255u ? 2u : 3u;
    if (end - pos < n) return s;
    s.count = n == 1u ? b0 : n == 2u ? ((b0 - 128u) << 8) + p[pos + 1] : zf_ld16(p + pos + 1) + 0x7F00u;
    s.have_count = 1; s.next = pos + n;
    if (s.count && s.next < end) { s.modes = p[s.next++]; s.have_modes = 1; }
    return s;
}
