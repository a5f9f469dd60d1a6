// zstd_seekable.h -- zstd's seekable container (contrib/seekable_format upstream): independent frames back to back, then one skippable
// frame, the seek table, as the file's last bytes.  Any zstd decoder reads the file as an ordinary .zst (it skips the table); a seekable
// reader decodes only the frames that cover a byte range.  All fields little-endian:
//   seek table = 5E 2A 4D 18 | Frame_Size u32 | entries | footer          Frame_Size = n * entry_bytes + 9
//   entry      = Compressed_Size u32 | Decompressed_Size u32 | [Checksum u32: the low 32 bits of XXH64(seed 0) of the frame's content]
//   footer     = Number_Of_Frames u32 | Descriptor u8 | B1 EA 92 8F       Descriptor: bit 7 checksums, bits 6..2 reserved (must be 0)
//
// kx_seekable_index is ONE body compiled three ways, as kx_frame_info is: by hipcc for the kernel (kmp_zstd_seekable_open), by hipcc's
// host pass for kmp_zstd_seekable_index_host and by g++ for the emulator and the stand-alone sanitizer program (tests/emu/).  It needs
// <stdint.h>, the public header and zstd_format.h.  Every read lies below an explicit bound: nothing outside [blob, blob + size) is
// touched, whatever the bytes are.  The order of its checks decides which status a damaged blob gets (libzstd's numbers):
//   fewer than 17 bytes, or the last four are not the seekable magic    10
//   a reserved descriptor bit                                            20
//   more than 2^27 frames, or a table larger than the blob               20
//   no skippable magic 0x184D2A5E where the table must begin             10
//   Frame_Size differs from n * entry_bytes + 9                          20
//   an entry that decodes to more than 1 GiB                             20
//   the compressed sizes do not sum to the table's offset                20   (this project's own check)
//
// The kernel bodies (plan, XXH64, table) follow under KX_DEV: they are written against kx_wave.h, which the includer brings.
#pragma once
#include <stdint.h>
#include "../../include/kompressor_hip.h"
#include "zstd_format.h"

#define KSK_MAGIC        0x8F92EAB1u
#define KSK_SKIP_MAGIC   0x184D2A5Eu
#define KSK_MAX_FRAMES   (1u << 27)
#define KSK_MAX_CONTENT  (1u << 30)          // decompressed bytes of one entry
#define KSK_FOOTER       9u
#define KSK_HEADER       8u

ZF_HD uint32_t ksk_entry_bytes(uint32_t flags) { return (flags & 1u) ? 12u : 8u; }
ZF_HD uint64_t ksk_table_bytes(uint64_t n, uint32_t flags) { return n * ksk_entry_bytes(flags) + KSK_HEADER + KSK_FOOTER; }

// the checks in front of the entries -> status; n / flags / table_off are set once they are known to be sound
ZF_HD uint32_t ksk_locate(const uint8_t* blob, uint64_t size, uint32_t* n_out, uint32_t* flags_out, uint64_t* table_off)
{
    if (size < KSK_HEADER + KSK_FOOTER) return 10;
    if (zf_ld32(blob + size - 4) != KSK_MAGIC) return 10;
    uint32_t const desc = blob[size - 5];
    if (desc & 0x7Cu) return 20;
    uint32_t const n = zf_ld32(blob + size - 9), flags = desc >> 7;
    if (n > KSK_MAX_FRAMES) return 20;
    uint64_t const table = ksk_table_bytes(n, flags);
    if (table > size) return 20;
    uint64_t const at = size - table;
    if (zf_ld32(blob + at) != KSK_SKIP_MAGIC) return 10;
    if (zf_ld32(blob + at + 4) != (uint32_t)(table - KSK_HEADER)) return 20;
    *n_out = n; *flags_out = flags; *table_off = at;
    return 0;
}

ZF_HD void kx_seekable_index(const uint8_t* blob, uint64_t size, kmp_seekable_stat* out)
{
    uint32_t n = 0, flags = 0, max_content = 0, max_compressed = 0; uint64_t at = 0, content = 0, compressed = 0;
    uint32_t status = ksk_locate(blob, size, &n, &flags, &at);
    if (!status) {
        uint32_t const eb = ksk_entry_bytes(flags);
        const uint8_t* e = blob + at + KSK_HEADER;                     // n * eb bytes, all inside the table that the blob holds
        for (uint32_t i = 0; i < n; i++, e += eb) {
            uint32_t const c = zf_ld32(e), d = zf_ld32(e + 4);
            if (d > KSK_MAX_CONTENT) { status = 20; break; }
            compressed += c; content += d;
            max_content = d > max_content ? d : max_content; max_compressed = c > max_compressed ? c : max_compressed;
        }
        if (!status && compressed != at) status = 20;
    }
    if (status) { n = 0; flags = 0; at = 0; content = 0; max_content = 0; max_compressed = 0; }
    out->content = content; out->table_off = at; out->frames = n; out->max_frame = max_content; out->max_compressed = max_compressed;
    out->flags = flags; out->status = status; out->reserved = 0;
}

#ifdef KX_DEV
#include "zstd_decode.h"             // (kxxh_round, kxxh_merge and the parts of kxxh64)

// ---- k_seekable_index: the body above on one lane (a chain of 8-byte reads over a table the host reads back anyway) ---------------
KX_DEV void seekable_index_body(const u8* blob, u64 size, kmp_seekable_stat* out)
{
    if (kx_block() == 0 && kx_wave() == 0 && kx_lane() == 0) kx_seekable_index(blob, size, out);
}

// ---- k_seekable_plan: the chunks of one buffer as a batch ------------------------------------------------------------------------
// chunk i = src[i * frame_bytes .. + min(frame_bytes, what is left)); its frame goes to the sparse area at i * stride
struct KSeekPlanArgs { u64 src_size; u32 frame_bytes; u32 n; u64 stride; u64* in_off; u32* in_len; u64* out_off; };

KX_DEV void seekable_plan_body(const KSeekPlanArgs& a)
{
    u32 const per_block = (u32)kx_nwaves() * 64u;
    for (u64 i = (u64)kx_block() * per_block + (u32)kx_wave() * 64u + (u32)kx_lane(); i < a.n; i += (u64)kx_nblocks() * per_block) {
        u64 const at = i * a.frame_bytes, left = a.src_size - at;
        a.in_off[i] = at; a.in_len[i] = left < a.frame_bytes ? (u32)left : a.frame_bytes; a.out_off[i] = i * a.stride;
    }
}

// ---- k_seekable_xxh64: XXH64 of n pieces, a quad of lanes per piece ---------------------------------------------------------------
// XXH64 walks its input in stripes of 32 bytes with four accumulators, each a serial chain (multiply, rotate, multiply) over its own
// 8 bytes of every stripe: lane j of a quad owns accumulator j, so the four lanes of a quad read the 32 contiguous bytes of a stripe, a
// wave reads 16 pieces at a time, and a 128-byte line serves four consecutive steps of its quad out of the cache.  KSX_AHEAD stripes
// are loaded before the first is consumed: the loads are independent of the chain, and with as few as one wave per SIMD (16 384 chunks
// are 1 024 waves) it is the loads in flight that decide the rate.  The trip count over the pieces is wave-uniform, so every lane
// reaches the quad exchange; the folded hash, the tail below 32 bytes and the avalanche are lane 0's (kxxh64_fold / kxxh64_finish).
// cks != null: cks[i] = the low 32 bits.  Else the verified read: frame i's entry in the container's table (12 bytes, at
// expect + 12 i, unaligned) holds the decoded size and the checksum; a frame that decoded cleanly (status 0) to another size gets
// status 20, with another checksum 22 (libzstd's "Restored data doesn't match checksum").
enum { KSX_AHEAD = 8 };
struct KSeekXxhArgs { const u8* src; const u64* off; const u32* len; u32 n; u32* cks; const u8* expect; u32* status; };

KX_DEV u64 ksx_quad64(u64 v, int k)
{
    u32 const lo = (u32)v, hi = (u32)(v >> 32);
    u32 const a = k == 0 ? kx_quad_bcast<0>(lo) : k == 1 ? kx_quad_bcast<1>(lo) : k == 2 ? kx_quad_bcast<2>(lo) : kx_quad_bcast<3>(lo);
    u32 const b = k == 0 ? kx_quad_bcast<0>(hi) : k == 1 ? kx_quad_bcast<1>(hi) : k == 2 ? kx_quad_bcast<2>(hi) : kx_quad_bcast<3>(hi);
    return (u64)a | ((u64)b << 32);
}

KX_DEV void seekable_xxh64_body(const KSeekXxhArgs& a)
{
    u32 const lane = (u32)kx_lane(), j = lane & 3u;
    u32 const waves = kx_nblocks() * (u32)kx_nwaves(), wave = kx_block() * (u32)kx_nwaves() + (u32)kx_wave();
    u32 const trips = (a.n + 16u * waves - 1u) / (16u * waves);
    for (u32 t = 0; t < trips; t++) {
        u64 const i64 = ((u64)t * waves + wave) * 16u + (lane >> 2);
        bool const live = i64 < a.n;
        u32 const i = live ? (u32)i64 : 0u;
        u32 len = live ? a.len[i] : 0u;
        if (live && !a.cks && a.status[i] != 0u) len = 0u;              // (a frame the decoder rejected: nothing to sum)
        const u8* const p = a.src + (live ? a.off[i] : 0ull);
        const u8* q = p + 8u * j;
        u32 const stripes = len >> 5;
        u64 v = kxxh64_start(j);
        u32 s = 0;
        for (; s + KSX_AHEAD <= stripes; s += KSX_AHEAD, q += 32u * KSX_AHEAD) {
            u64 w[KSX_AHEAD];
#pragma unroll
            for (int k = 0; k < KSX_AHEAD; k++) w[k] = kx_ld64(q + 32 * k);
#pragma unroll
            for (int k = 0; k < KSX_AHEAD; k++) v = kxxh_round(v, w[k]);
        }
        for (; s < stripes; s++, q += 32) v = kxxh_round(v, kx_ld64(q));
        u64 const v1 = ksx_quad64(v, 0), v2 = ksx_quad64(v, 1), v3 = ksx_quad64(v, 2), v4 = ksx_quad64(v, 3);
        if (live && j == 0u) {
            u64 const h = kxxh64_finish(stripes ? kxxh64_fold(v1, v2, v3, v4) : 2870177450012600261ULL, p, stripes << 5, len);
            if (a.cks) a.cks[i] = (u32)h;
            else if (a.status[i] == 0u) {
                const u8* const e = a.expect + 12ull * i;
                if (kx_ld32(e + 4) != len) a.status[i] = 20u;
                else if (kx_ld32(e + 8) != (u32)h) a.status[i] = 22u;
            }
        }
    }
}

// ---- k_seekable_table: the seek table behind the last frame, one workgroup ---------------------------------------------------------
// Runs after the compaction: dense_off[n] is where the frames end.  The table lands at whatever byte offset that is, so every field
// goes out through kx_st32 (no alignment assumed).  result[0] = the container's size, or 0 when a chunk has no frame (its out_len is 0:
// the batch refused it); result[1] = the context's status word as it stands (kmp_batch_status reads and clears it).
struct KSeekTableArgs { u8* dst; const u64* dense_off; const u32* clen; const u32* dlen; const u32* cks; u32 n; u32 flags; const u32* ctx_status; u64* result; };

KX_DEV void seekable_table_body(const KSeekTableArgs& a)
{
    KX_SHARED u32 failed;
    u32 const threads = (u32)kx_nwaves() * 64u, t = (u32)kx_wave() * 64u + (u32)kx_lane();
    if (t == 0) failed = 0;
    kx_block_sync();
    u64 const frames_end = a.n ? a.dense_off[a.n] : 0ull;
    u32 const eb = ksk_entry_bytes(a.flags);
    u8* const table = a.dst + frames_end;
    u32 bad = 0;
    for (u32 i = t; i < a.n; i += threads) {
        u32 const c = a.clen[i];
        u8* const e = table + KSK_HEADER + (u64)i * eb;
        kx_st32(e, c); kx_st32(e + 4, a.dlen[i]);
        if (a.flags & 1u) kx_st32(e + 8, a.cks[i]);
        bad |= c == 0u ? 1u : 0u;
    }
    if (bad) kx_lds_or(&failed, 1u);
    kx_block_sync();
    if (t == 0) {
        u64 const entries = (u64)a.n * eb;
        u8* const f = table + KSK_HEADER + entries;
        kx_st32(table, KSK_SKIP_MAGIC); kx_st32(table + 4, (u32)entries + KSK_FOOTER);
        kx_st32(f, a.n); f[4] = (u8)(a.flags << 7); kx_st32(f + 5, KSK_MAGIC);
        a.result[0] = failed ? 0ull : frames_end + KSK_HEADER + entries + KSK_FOOTER;
        a.result[1] = a.ctx_status ? (u64)a.ctx_status[0] : 0ull;
    }
}
#endif
