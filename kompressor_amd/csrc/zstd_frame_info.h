// zstd_frame_info.h -- what a batch of zstd frames declares about itself, without decoding it: libzstd's
// ZSTD_findDecompressedSize, ZSTD_decompressBound and ZSTD_findFrameCompressedSize in batched form (kmp_zstd_frame_info_batch,
// kmp_zstd_frame_info_host) and the layout a decode needs made of the answers (kmp_batch_layout).
//
// kx_frame_info is ONE body compiled three ways: by hipcc for the kernel, by hipcc's host pass for the host call and by g++ for the
// emulator and the stand-alone sanitizer program (tests/emu/): it needs <stdint.h>, the public header and zstd_format.h.  It restates the walk of
// libzstd 1.5.7 (lib/decompress/zstd_decompress.c: ZSTD_findFrameSizeInfo, ZSTD_getFrameHeader_advanced, readSkippableFrameSize,
// ZSTD_getcBlockSize) in that library's order of checks, because the order decides which error a damaged entry gets:
//   fewer than 5 bytes          72 when they are a prefix of the zstd magic or of a skippable magic (low nibble free), else 10
//   skippable magic, < 8 bytes  72;  size + 8 wraps 32 bits: 14;  size + 8 beyond the entry: 72
//   another magic               10  (0xFD2FB525 .. 27, the formats of zstd 0.5 .. 0.7, are known to the library: below)
//   header longer than entry    72  -- before the reserved bit (14) and the window (16: a window log above 31) are looked at
//   block header cut short      72;  block type 3: 20;  block beyond the entry: 72;  checksum cut short: 72
// Every read lies below an explicit bound: nothing outside [src, src + len) is touched, wherever the entry lies.
//
// The kernel bodies (zstd_frame_info_body, batch_layout_body) follow under KX_DEV: they are written against kx_wave.h, which the
// includer brings (the product's or the emulator's).
#pragma once
#include <stdint.h>
#include "../../include/kompressor_hip.h"
#include "zstd_format.h"

#define KFI_CONTENT_ERROR (~0ull - 1)          // ZSTD_CONTENTSIZE_ERROR: what the library's size functions answer for a total they cannot give

// One entry, frame by frame.  Fields as include/kompressor_hip.h documents them; frames / dict_id / flags cover the frames in front of
// the first one that is rejected.
ZF_HD void kx_frame_info(const uint8_t* src, uint32_t len, kmp_zstd_frame_info* out)
{
    uint64_t content = 0, bound = 0;
    uint32_t status = 0, frames = 0, dict_id = 0, flags = 0;
    uint32_t pos = 0;
    while (pos < len) {
        const uint8_t* const p = src + pos;
        uint32_t const rem = len - pos;
        if (rem >= 4 && zf_ld32(p) - 0xFD2FB525u <= 2u) {
            // The binary library carries the frame formats of zstd 0.5, 0.6 and 0.7 (ZSTD_LEGACY_SUPPORT 5) and sizes their frames too
            // (ZSTDv05/06/07_findFrameSizeInfoLegacy, ZSTD_getDecompressedSize_legacy).  The decoders here do not decode them: flags bit 2.
            uint32_t const v = zf_ld32(p) - 0xFD2FB520u;
            if (rem < (v == 7u ? 8u : 5u)) { status = 72; break; }
            uint32_t const d = p[4];
            uint32_t const fcs_code = d >> 6;
            uint32_t hs = 5, fcs_bytes = 0, fcs_ok = 1;
            if (v == 6u) { fcs_bytes = fcs_code == 3u ? 8u : fcs_code; hs = 5u + fcs_bytes; fcs_ok = !(d & 0x20u); }
            if (v == 7u) {
                uint32_t const direct = (d >> 5) & 1u, did_bytes = (d & 3u) == 3u ? 4u : d & 3u;
                fcs_bytes = fcs_code ? 1u << fcs_code : direct;
                hs = 5u + (direct ^ 1u) + did_bytes + fcs_bytes;
            }
            if (v >= 6u && rem < hs + 3u) { status = 72; break; }
            uint32_t at = hs, blocks = 0;
            for (;;) {
                if (rem - at < 3u) { status = 72; break; }
                uint32_t const type = p[at] >> 6;                                    // 0 compressed, 1 raw, 2 RLE, 3 end
                uint32_t const csz = (uint32_t)p[at + 2] | ((uint32_t)p[at + 1] << 8) | (((uint32_t)p[at] & 7u) << 16);
                uint32_t const c = type == 3u ? 0u : type == 2u ? 1u : csz;
                at += 3u;
                if (c > rem - at) { status = 72; break; }
                if (v == 7u ? type == 3u : c == 0u) break;                           // (0.5 and 0.6 stop at an empty block of any type)
                at += c; blocks++;
            }
            if (status) break;
            uint64_t fcs = 0;                                                        // 0: none declared, or a header its version refuses
            if (v >= 6u && fcs_bytes) {
                uint32_t q = hs - fcs_bytes;
                for (uint32_t k = 0; k < fcs_bytes; k++) fcs |= (uint64_t)p[q + k] << (8 * k);
                if (v == 6u ? fcs_code == 2u : fcs_code == 1u) fcs += 256;
            }
            if (v == 7u) {
                uint64_t window = 0;
                if (d & 8u) fcs_ok = 0;
                if (!(d & 0x20u)) {
                    uint32_t const wlog = (p[5] >> 3) + 10u;
                    if (wlog > 27u) fcs_ok = 0;
                    window = 1ull << (wlog & 31u); window += (window >> 3) * (p[5] & 7u);
                }
                if (!window) window = (uint32_t)fcs;
                if (window > (1ull << 27)) fcs_ok = 0;
            }
            if (!fcs_ok || fcs == 0) fcs = ~0ull;
            uint64_t const fb = (uint64_t)blocks << 17;
            if (bound != KFI_CONTENT_ERROR) bound += fb;
            if (content < KFI_CONTENT_ERROR) content = fcs >= KFI_CONTENT_ERROR ? fcs : content + fcs < content ? KFI_CONTENT_ERROR : content + fcs;
            frames++;
            flags |= 4u;
            pos += at;
            continue;
        }
        if (rem < 5) {
            // ZSTD_getFrameHeader: the bytes present laid over the zstd magic, then over the first skippable magic
            uint32_t const n = rem < 4 ? rem : 4;
            uint32_t a = ZF_MAGIC, b = ZF_SKIP_MAGIC;
            for (uint32_t k = 0; k < n; k++) {
                uint32_t const m = 0xFFu << (8 * k), v = (uint32_t)p[k] << (8 * k);
                a = (a & ~m) | v; b = (b & ~m) | v;
            }
            status = (a == ZF_MAGIC || (b & ZF_SKIP_MASK) == ZF_SKIP_MAGIC) ? 72u : 10u;
            break;
        }
        uint32_t const magic = zf_ld32(p);
        if ((magic & ZF_SKIP_MASK) == ZF_SKIP_MAGIC) {
            if (rem < 8) { status = 72; break; }
            uint32_t const sz = zf_ld32(p + 4);
            if ((uint32_t)(sz + 8u) < sz) { status = 14; break; }
            if (sz + 8u > rem) { status = 72; break; }
            pos += sz + 8u;
            flags |= 2u;
            continue;
        }
        if (magic != ZF_MAGIC) { status = 10; break; }
        ZfDescriptor const fd = zf_descriptor(p[4]);
        if (rem < fd.header_size) { status = 72; break; }
        if (fd.reserved) { status = 14; break; }
        uint32_t q = 5; uint64_t window = 0;
        if (!fd.single) {
            ZfWindow const w = zf_window(p[q++]);
            if (w.log > 31u) { status = 16; break; }
            window = w.size;
        }
        uint32_t const did = (uint32_t)zf_le(p + q, fd.did_bytes); q += fd.did_bytes;
        uint64_t const fcs = fd.fcs_bytes ? zf_content_size(p + q, fd.fcs_bytes) : ~0ull;
        if (fd.single) window = fcs;
        uint64_t const block_max = window < ZF_BLOCK_MAX ? window : (uint64_t)ZF_BLOCK_MAX;
        // the blocks: 3 header bytes each, then the block's bytes (an RLE block: one)
        uint32_t at = fd.header_size, blocks = 0;
        for (;;) {
            if (rem - at < 3u) { status = 72; break; }
            ZfBlock const bh = zf_block(p + at);
            if (bh.type == 3u) { status = 20; break; }
            uint32_t const csize = bh.type == 1u ? 1u : bh.size;
            if (3u + csize > rem - at) { status = 72; break; }
            at += 3u + csize;
            blocks++;
            if (bh.last) break;
        }
        if (status) break;
        if (fd.checksum) {
            if (rem - at < 4u) { status = 72; break; }
            at += 4u;
        }
        // ZSTD_decompressBound's sum and ZSTD_findDecompressedSize's: the first frame without a size (or with one of the two reserved
        // values in an 8-byte field) decides the latter
        uint64_t const fb = fcs != ~0ull ? fcs : (uint64_t)blocks * block_max;
        if (bound != KFI_CONTENT_ERROR) bound = fb == KFI_CONTENT_ERROR ? KFI_CONTENT_ERROR : bound + fb;
        if (content < KFI_CONTENT_ERROR) content = fcs >= KFI_CONTENT_ERROR ? fcs : content + fcs < content ? KFI_CONTENT_ERROR : content + fcs;
        if (!frames) dict_id = did;
        frames++;
        if (fd.checksum) flags |= 1u;
        pos += at;
    }
    if (status) { content = 0; bound = 0; }
    out->content = content; out->bound = bound; out->status = status; out->frames = frames; out->dict_id = dict_id; out->flags = flags;
}

#ifdef KX_DEV
// ---- k_zstd_frame_info: a lane per entry ---------------------------------------------------------------------------------------
// A header is at most 18 bytes and the block walk is a chain of dependent 3-byte reads: nothing a wave could share.  Every frame's
// blocks are walked, declared size or not (where the frame ends is part of the answer, and an entry may hold more frames); what
// differs between the lanes of a wave is the number of blocks, and the wave takes as long as its longest chain.
struct KFrameInfoArgs { const u8* src; const u64* in_off; const u32* in_len; u32 n; kmp_zstd_frame_info* info; };

KX_DEV void zstd_frame_info_body(const KFrameInfoArgs& a)
{
    u32 const per_block = (u32)kx_nwaves() * 64u;
    u32 const stride = kx_nblocks() * per_block;
    for (u32 i = kx_block() * per_block + (u32)kx_wave() * 64u + (u32)kx_lane(); i < a.n; i += stride) {
        kmp_zstd_frame_info r;
        kx_frame_info(a.src + a.in_off[i], a.in_len[i], &r);
        a.info[i] = r;
    }
}

// ---- k_batch_layout: capacities and offsets of a decode, one workgroup ---------------------------------------------------------
// cap[i] = bound[i], or 0 where the entry was rejected or its bound does not fit 32 bits; off[i] = the sum of the caps in front of it,
// each rounded up to `align`; total[0] = the sum, total[1] = the entries given 0 for one of the two reasons.  Each thread owns a run of
// consecutive entries (n / threads, rounded up): its sum, an inclusive scan over the lanes of its wave (kx_shfl, 32 bits at a time), the
// waves' totals through LDS, then the run once more to write.  No atomics: the same input gives the same output.
enum { KFI_LAYOUT_WAVES = 16 };
struct KLayoutArgs { const kmp_zstd_frame_info* info; u32 n; u32 align; u64* out_off; u32* out_cap; u64* total; };

KX_DEV u32 kfi_cap(const kmp_zstd_frame_info& f, u32* refused)
{
    bool const bad = f.status != 0 || f.bound >= (1ull << 32);
    *refused += bad ? 1u : 0u;
    return bad ? 0u : (u32)f.bound;
}
KX_DEV u64 kfi_shfl64(u64 v, int src) { return (u64)kx_shfl((u32)v, src) | ((u64)kx_shfl((u32)(v >> 32), src) << 32); }

KX_DEV void batch_layout_body(const KLayoutArgs& a)
{
    KX_SHARED u64 wave_sum[KFI_LAYOUT_WAVES];
    KX_SHARED u32 wave_bad[KFI_LAYOUT_WAVES];
    int const lane = kx_lane(), wave = kx_wave(), waves = kx_nwaves();
    u32 const threads = (u32)waves * 64u, t = (u32)wave * 64u + (u32)lane;
    u32 const per = (a.n + threads - 1) / threads;
    u64 const b64 = (u64)t * per;
    u32 const b = b64 < a.n ? (u32)b64 : a.n, e = a.n - b < per ? a.n : b + per;
    u64 const mask = (u64)a.align - 1;
    u64 sum = 0; u32 bad = 0;
    for (u32 i = b; i < e; i++) sum += ((u64)kfi_cap(a.info[i], &bad) + mask) & ~mask;
    u64 inc = sum; u32 badinc = bad;
    for (int o = 1; o < 64; o <<= 1) {
        u64 const v = kfi_shfl64(inc, lane - o); u32 const w = kx_shfl(badinc, lane - o);
        if (lane >= o) { inc += v; badinc += w; }
    }
    if (lane == 63) { wave_sum[wave] = inc; wave_bad[wave] = badinc; }
    kx_block_sync();
    u64 run = inc - sum;
    for (int w = 0; w < wave; w++) run += wave_sum[w];
    u32 unused = 0;
    for (u32 i = b; i < e; i++) {
        u32 const cap = kfi_cap(a.info[i], &unused);
        a.out_cap[i] = cap; a.out_off[i] = run;
        run += ((u64)cap + mask) & ~mask;
    }
    if (t == threads - 1) {
        u32 nb = 0;
        for (int w = 0; w < waves; w++) nb += wave_bad[w];
        a.total[0] = run; a.total[1] = nb;
    }
}
#endif
