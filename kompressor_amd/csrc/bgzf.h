// bgzf.h -- BGZF (SAM specification 4.1; bgzip, htslib, Bio.bgzf): a series of gzip members of at most 64 KiB of input each, every one
// carrying its own size in a gzip extra field, then an empty member as the end-of-file marker.  Any gzip reader reads the file as
// ordinary multi-member gzip; a BGZF reader decodes only the members that cover a byte range.  All fields little-endian:
//   member = 1f 8b 08 04 | MTIME u32 | XFL | OS | XLEN u16 | subfields (SI1 SI2 SLEN u16 data; 'B' 'C' 02 00 BSIZE u16 = member bytes - 1)
//            | raw DEFLATE payload | CRC32 u32 | ISIZE u32
//   marker = 1f8b08040000000000ff0600424302001b0003000000000000000000
//
// kx_bgzf_head -- the test of a member's head at one position -- and kx_bgzf_walk -- the members followed from offset 0 -- are ONE
// body compiled three ways, as kx_seekable_index is: by hipcc for the kernels, by hipcc's host pass for kmp_bgzf_index_host and by g++
// for the emulator and the stand-alone sanitizer program (tests/emu/).  They need <stdint.h>, the public header and zstd_format.h.  No
// byte outside [p, size) of the blob is read, whatever the bytes are.  The order of the head's checks decides which status a damaged blob
// gets (zlib's numbers; r = size - p):
//   the first min(r, 4) bytes are not 1f 8b 08 04                                  -3
//   r < 12                                                                         -5
//   XLEN < 6                                                                       -3
//   r < 12 + XLEN                                                                  -5
//   a subfield that runs past XLEN; BC with SLEN != 2; a second BC; no BC          -3
//   BSIZE + 1 < 12 + XLEN + 2 + 8                                                  -3
//   r < BSIZE + 1                                                                  -5
//   ISIZE > 65 536                                                                 -3
//
// The kernel bodies follow under KX_DEV: they are written against kx_wave.h, which the includer brings.  The parallel open:
//   scan (count)  every wave takes tiles of KBZ_TILE positions; a lane reads 8 bytes and looks at its 4 positions for the magic (the
//                 magic cannot overlap itself: at most one of the 4 matches), runs the head test there and counts the valid heads
//   prefix        one workgroup: the exclusive scan of the tile counts; the total goes to the host, which allocates
//   scan (fill)   the same pass writes the candidates in position order: tile base + the wave's running count + the lane's ballot rank
//   link          succ[i] = the candidate at pos + total (binary search), KBZ_END at the blob's end, KBZ_DEAD when none stands there
//   double        jump[k][i] = jump[k-1][jump[k-1][i]], one launch per level
//   mark          mark[0] = candidate 0 stands at offset 0; from the top level down every marked i marks jump[k][i]: after level 0
//                 exactly the chain from offset 0 is marked (a false chain that merges into it adds nothing: only marked entries mark)
//   gather        one workgroup: the scan of the marks and of the marked ISIZEs, the handle's arrays, the stat
#pragma once
#include <stdint.h>
#include "../../include/kompressor_hip.h"
#include "zstd_format.h"

#define KBZ_MAGIC          0x04088B1Fu
#define KBZ_BLOCK_MAX      65280u          // input bytes of a member (htslib's block size)
#define KBZ_MEMBER_MAX     65536u          // what BSIZE can express; also the largest ISIZE a reader accepts
#define KBZ_HEAD           18u             // header of a member with the BC subfield alone
#define KBZ_WRAP           26u             // ... and the trailer
#define KBZ_EOF_BYTES      28u
#define KBZ_END            0xFFFFFFFFu
#define KBZ_DEAD           0xFFFFFFFEu
#define KBZ_MAX_CANDIDATES (1u << 20)      // above this the open walks serially: the doubling tables would reach 84 MB
#define KBZ_TILE           4096u           // positions a wave counts at a time: 16 steps of 64 lanes x 4 positions

struct KBgzfHead { uint32_t total, xlen, isize, extra; };      // extra: subfields besides BC

ZF_HD int32_t kx_bgzf_head(const uint8_t* blob, uint64_t size, uint64_t p, KBgzfHead* h)
{
    uint64_t const r = size - p;
    const uint8_t* const b = blob + p;
    for (uint32_t i = 0; i < 4u && i < r; i++) if (b[i] != (uint8_t)(KBZ_MAGIC >> (8u * i))) return -3;
    if (r < 12u) return -5;
    uint32_t const xlen = zf_ld16(b + 10);
    if (xlen < 6u) return -3;
    if (r < 12u + xlen) return -5;
    uint32_t q = 0, found = 0, bsize = 0, extra = 0;
    while (q < xlen) {
        if (xlen - q < 4u) return -3;
        const uint8_t* const s = b + 12u + q;
        uint32_t const slen = zf_ld16(s + 2);
        if (slen > xlen - q - 4u) return -3;
        if (s[0] == 'B' && s[1] == 'C') {
            if (slen != 2u || found) return -3;
            found = 1; bsize = zf_ld16(s + 4);
        } else extra = 1;
        q += 4u + slen;
    }
    if (!found) return -3;
    uint32_t const total = bsize + 1u;
    if (total < 12u + xlen + 2u + 8u) return -3;
    if (r < total) return -5;
    uint32_t const isize = zf_ld32(b + total - 4u);
    if (isize > KBZ_MEMBER_MAX) return -3;
    h->total = total; h->xlen = xlen; h->isize = isize; h->extra = extra;
    return 0;
}

// the 28 bytes of a valid head of 28 bytes at b are the marker's
ZF_HD uint32_t kbz_is_eof(const uint8_t* b, uint32_t total)
{
    return total == KBZ_EOF_BYTES && zf_ld32(b + 4) == 0u && zf_ld32(b + 8) == 0x0006FF00u && zf_ld32(b + 12) == 0x00024342u
           && zf_ld32(b + 16) == 0x0003001Bu && zf_ld32(b + 20) == 0u && zf_ld32(b + 24) == 0u;
}

// what a reader keeps of every member, as kmp_inflate_batch takes it: where the payload lies, its bytes, ISIZE
struct KBgzfArrays { uint64_t* in_off; uint32_t* in_len; uint32_t* out_cap; };

ZF_HD void kbz_stat_set(kmp_bgzf_stat* out, uint64_t content, uint32_t blocks, uint32_t max_block, uint32_t max_compressed, uint32_t flags, int32_t status)
{
    if (status) { content = 0; blocks = 0; max_block = 0; max_compressed = 0; flags = 0; }
    out->content = content; out->blocks = blocks; out->max_block = max_block; out->max_compressed = max_compressed;
    out->flags = flags; out->status = status; out->reserved = 0;
}

// The serial walk.  member_off / content_off (each may be null): entry i < cap is written as member i is passed, and entry `blocks`
// (the blob's size, the content's) at the end when it fits; arr (may be null): the same for the reader's arrays.  A caller that wants
// nothing written for a damaged blob walks once with cap 0 and looks at the status first.
ZF_HD void kx_bgzf_walk_into(const uint8_t* blob, uint64_t size, kmp_bgzf_stat* stat, uint64_t* member_off, uint64_t* content_off, uint64_t cap,
                             const KBgzfArrays* arr)
{
    uint64_t p = 0, content = 0, n = 0;
    uint32_t max_block = 0, max_compressed = 0, flags = 0;
    int32_t status = size ? 0 : -5;
    while (!status && p < size) {
        KBgzfHead h;
        status = kx_bgzf_head(blob, size, p, &h);
        if (status) break;
        if (n < cap) {
            if (member_off) member_off[n] = p;
            if (content_off) content_off[n] = content;
            if (arr) { arr->in_off[n] = p + 12u + h.xlen; arr->in_len[n] = h.total - 20u - h.xlen; arr->out_cap[n] = h.isize; }
        }
        max_block = h.isize > max_block ? h.isize : max_block; max_compressed = h.total > max_compressed ? h.total : max_compressed;
        flags = (flags & 2u) | (h.extra ? 2u : 0u) | kbz_is_eof(blob + p, h.total);
        n++; p += h.total; content += h.isize;
    }
    if (!status && n > 0xFFFFFFFFull) status = -3;
    if (!status && n < cap) {
        if (member_off) member_off[n] = p;
        if (content_off) content_off[n] = content;
    }
    kbz_stat_set(stat, content, (uint32_t)n, max_block, max_compressed, flags, status);
}
ZF_HD void kx_bgzf_walk(const uint8_t* blob, uint64_t size, kmp_bgzf_stat* stat, uint64_t* member_off, uint64_t* content_off, uint64_t cap)
{
    kx_bgzf_walk_into(blob, size, stat, member_off, content_off, cap, nullptr);
}

#ifdef KX_DEV
#include "deflate_encode.h"          // (kx_wave_crc32)

// ---- k_bgzf_walk: the walk on one lane, the yardstick of the parallel open and its fallback ---------------------------------------
KX_DEV void bgzf_walk_body(const u8* blob, u64 size, kmp_bgzf_stat* stat, u64* member_off, u64* content_off, u64 cap, KBgzfArrays arr)
{
    if (kx_block() == 0 && kx_wave() == 0 && kx_lane() == 0) kx_bgzf_walk_into(blob, size, stat, member_off, content_off, cap, arr.in_off ? &arr : nullptr);
}

// ---- k_bgzf_wrap: header and trailer around every payload, a wave (a workgroup of one wave) per block ------------------------------
// The batch wrote block i's raw DEFLATE stream KBZ_HEAD bytes into its stride slot (out_len[i] bytes, 0: the batch refused the block).
// out_len[i] becomes the member's size, or 0 for a block without a stream or a member BSIZE cannot express.
struct KBgzfWrapArgs { const u8* src; const u64* in_off; const u32* in_len; u8* frames; const u64* out_off; u32* out_len; u32 n; };

KX_DEV void bgzf_wrap_body(const KBgzfWrapArgs& a)
{
    KX_SHARED u32 tab[256];
    int const lane = kx_lane();
    for (u32 i = kx_block(); i < a.n; i += kx_nblocks()) {
        u32 const len = a.in_len[i], plen = a.out_len[i];
        u32 const crc = kx_wave_crc32(a.src + a.in_off[i], len, tab, lane);
        u32 const total = plen + KBZ_WRAP;
        bool const ok = plen != 0u && total <= KBZ_MEMBER_MAX;
        if (lane == 0) {
            if (ok) {
                u8* const m = a.frames + a.out_off[i];
                kx_st32(m, KBZ_MAGIC); kx_st32(m + 4, 0u); kx_st32(m + 8, 0x0006FF00u); kx_st32(m + 12, 0x00024342u); kx_st16(m + 16, total - 1u);
                kx_st32(m + KBZ_HEAD + plen, crc); kx_st32(m + KBZ_HEAD + plen + 4u, len);
            }
            a.out_len[i] = ok ? total : 0u;
        }
    }
}

// ---- k_bgzf_finish: the marker behind the last member and the result, one workgroup ------------------------------------------------
// Runs after the compaction: dense_off[n] is where the members end.  result[0] = the container's size, or 0 when a block has no member;
// result[1] = the context's status word as it stands.
struct KBgzfFinishArgs { u8* dst; const u64* dense_off; const u32* out_len; u32 n; u32 flags; const u32* ctx_status; u64* result; };

KX_DEV void bgzf_finish_body(const KBgzfFinishArgs& a)
{
    KX_SHARED u32 failed;
    u32 const threads = (u32)kx_nwaves() * 64u, t = (u32)kx_wave() * 64u + (u32)kx_lane();
    if (t == 0) failed = 0;
    kx_block_sync();
    u32 bad = 0;
    for (u32 i = t; i < a.n; i += threads) bad |= a.out_len[i] == 0u ? 1u : 0u;
    if (bad) kx_lds_or(&failed, 1u);
    kx_block_sync();
    if (t == 0) {
        u64 end = a.n ? a.dense_off[a.n] : 0ull;
        if (!failed && !(a.flags & KMP_BGZF_NO_EOF)) {
            u8* const m = a.dst + end;
            kx_st32(m, KBZ_MAGIC); kx_st32(m + 4, 0u); kx_st32(m + 8, 0x0006FF00u); kx_st32(m + 12, 0x00024342u); kx_st32(m + 16, 0x0003001Bu);
            kx_st32(m + 20, 0u); kx_st32(m + 24, 0u);
            end += KBZ_EOF_BYTES;
        }
        a.result[0] = failed ? 0ull : end;
        a.result[1] = a.ctx_status ? (u64)a.ctx_status[0] : 0ull;
    }
}

// ---- k_bgzf_scan: the candidates, counted (tile_base null) or written in position order --------------------------------------------
// Bound by the read of the blob: every byte once from memory (the 4-byte halo of a lane is its neighbour's line).  The head test runs
// only where the magic stands.
struct KBgzfCand { u64 pos; u32 total; u32 isize; u32 xlen; u32 extra; };        // 24 bytes
struct KBgzfScanArgs { const u8* blob; u64 size; u64 ntiles; u32* tile_count; const u32* tile_base; KBgzfCand* cand; };

KX_DEV void bgzf_scan_body(const KBgzfScanArgs& a)
{
    u32 const lane = (u32)kx_lane();
    u64 const waves = (u64)kx_nblocks() * (u32)kx_nwaves(), wave = (u64)kx_block() * (u32)kx_nwaves() + (u32)kx_wave();
    for (u64 tile = wave; tile < a.ntiles; tile += waves) {
        u32 count = 0;
        u32 const base = a.tile_base ? a.tile_base[tile] : 0u;
        for (u32 step = 0; step < KBZ_TILE / 256u; step++) {
            u64 const p0 = tile * KBZ_TILE + step * 256u + lane * 4u;
            bool hit = false; u64 hp = 0; KBgzfHead h; h.total = 0; h.xlen = 0; h.isize = 0; h.extra = 0;
            if (p0 < a.size) {
                u64 w = 0;
                if (p0 + 8u <= a.size) w = kx_ld64(a.blob + p0);
                else for (u32 k = 0; k < (u32)(a.size - p0); k++) w |= (u64)a.blob[p0 + k] << (8u * k);      // (no byte of the magic is 0)
                for (u32 k = 0; k < 4u; k++)
                    if ((u32)(w >> (8u * k)) == KBZ_MAGIC) { hp = p0 + k; hit = kx_bgzf_head(a.blob, a.size, hp, &h) == 0; break; }
            }
            u64 const votes = kx_ballot(hit);
            if (a.tile_base && hit) {
                KBgzfCand c; c.pos = hp; c.total = h.total; c.isize = h.isize; c.xlen = h.xlen; c.extra = h.extra;
                a.cand[base + count + kx_popc64(votes & ((1ull << lane) - 1ull))] = c;
            }
            count += kx_popc64(votes);
        }
        if (!a.tile_base && lane == 0) a.tile_count[tile] = count;
    }
}

// ---- k_bgzf_prefix: the exclusive scan of n counts in place, one workgroup; v[n] = the total --------------------------------------
KX_DEV void bgzf_prefix_body(u32* v, u64 n)
{
    KX_SHARED u32 part[1024];
    u32 const threads = (u32)kx_nwaves() * 64u, t = (u32)kx_wave() * 64u + (u32)kx_lane();
    u64 const chunk = (n + threads - 1u) / threads;
    u64 const lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    u32 s = 0;
    for (u64 i = lo; i < hi; i++) s += v[i];
    part[t] = s;
    kx_block_sync();
    u32 run = 0;
    for (u32 j = 0; j < t; j++) run += part[j];
    for (u64 i = lo; i < hi; i++) { u32 const x = v[i]; v[i] = run; run += x; }
    if (t == threads - 1u) v[n] = run;
}

// ---- k_bgzf_link: successors (level 0 of the jump table) and the first mark --------------------------------------------------------
struct KBgzfLinkArgs { const KBgzfCand* cand; u32 n; u64 size; u32* succ; u32* mark; };

KX_DEV void bgzf_link_body(const KBgzfLinkArgs& a)
{
    u32 const per = (u32)kx_nwaves() * 64u;
    for (u64 i = (u64)kx_block() * per + (u32)kx_wave() * 64u + (u32)kx_lane(); i < a.n; i += (u64)kx_nblocks() * per) {
        u64 const want = a.cand[i].pos + a.cand[i].total;
        u32 s = KBZ_DEAD;
        if (want == a.size) s = KBZ_END;
        else {
            u32 lo = (u32)i + 1u, hi = a.n;                     // the first candidate at or behind `want`
            while (lo < hi) { u32 const mid = lo + (hi - lo) / 2u; if (a.cand[mid].pos < want) lo = mid + 1u; else hi = mid; }
            if (lo < a.n && a.cand[lo].pos == want) s = lo;
        }
        a.succ[i] = s;
        a.mark[i] = (i == 0 && a.cand[0].pos == 0) ? 1u : 0u;
    }
}

// ---- k_bgzf_double / k_bgzf_mark: one level each -----------------------------------------------------------------------------------
KX_DEV void bgzf_double_body(const u32* prev, u32* next, u32 n)
{
    u32 const per = (u32)kx_nwaves() * 64u;
    for (u64 i = (u64)kx_block() * per + (u32)kx_wave() * 64u + (u32)kx_lane(); i < n; i += (u64)kx_nblocks() * per) {
        u32 const j = prev[i];
        next[i] = j >= KBZ_DEAD ? j : prev[j];
    }
}
// (a mark set by another lane of the same launch may or may not be seen: either way only entries of the chain mark entries of the chain)
KX_DEV void bgzf_mark_body(const u32* jump, u32* mark, u32 n)
{
    u32 const per = (u32)kx_nwaves() * 64u;
    for (u64 i = (u64)kx_block() * per + (u32)kx_wave() * 64u + (u32)kx_lane(); i < n; i += (u64)kx_nblocks() * per) {
        if (!mark[i]) continue;
        u32 const j = jump[i];
        if (j < KBZ_DEAD) mark[j] = 1u;
    }
}

// ---- k_bgzf_gather: the marked candidates become the reader's arrays and the stat, one workgroup ----------------------------------
// member_off / content_off: blocks + 1 entries; status: 0 when the chain ends at the blob's end, else the head test's where it stops
struct KBgzfGatherArgs { const u8* blob; u64 size; const KBgzfCand* cand; const u32* succ; const u32* mark; u32 n;
                         u64* member_off; u64* content_off; KBgzfArrays arr; kmp_bgzf_stat* stat; };

KX_DEV void bgzf_gather_body(const KBgzfGatherArgs& a)
{
    KX_SHARED u32 pn[1024]; KX_SHARED u64 pc[1024]; KX_SHARED u32 pmb[1024]; KX_SHARED u32 pmc[1024]; KX_SHARED u32 pfl[1024];
    KX_SHARED int32_t end_status; KX_SHARED u32 end_eof;
    u32 const threads = (u32)kx_nwaves() * 64u, t = (u32)kx_wave() * 64u + (u32)kx_lane();
    u32 const chunk = (a.n + threads - 1u) / threads;
    u32 const lo = (u64)t * chunk < a.n ? t * chunk : a.n, hi = (u64)lo + chunk < a.n ? lo + chunk : a.n;
    u32 cnt = 0, mb = 0, mc = 0, fl = 0; u64 sum = 0;
    for (u32 i = lo; i < hi; i++) {
        if (!a.mark[i]) continue;
        KBgzfCand const c = a.cand[i];
        cnt++; sum += c.isize; mb = c.isize > mb ? c.isize : mb; mc = c.total > mc ? c.total : mc; fl |= c.extra ? 2u : 0u;
        u32 const s = a.succ[i];
        if (s >= KBZ_DEAD) {                                    // the chain's last member: one lane gets here
            KBgzfHead h;
            end_status = s == KBZ_END ? 0 : kx_bgzf_head(a.blob, a.size, c.pos + c.total, &h);
            end_eof = kbz_is_eof(a.blob + c.pos, c.total);
        }
    }
    pn[t] = cnt; pc[t] = sum; pmb[t] = mb; pmc[t] = mc; pfl[t] = fl;
    kx_block_sync();
    u32 idx = 0; u64 content = 0;
    for (u32 j = 0; j < t; j++) { idx += pn[j]; content += pc[j]; }
    for (u32 i = lo; i < hi; i++) {
        if (!a.mark[i]) continue;
        KBgzfCand const c = a.cand[i];
        a.member_off[idx] = c.pos; a.content_off[idx] = content;
        a.arr.in_off[idx] = c.pos + 12u + c.xlen; a.arr.in_len[idx] = c.total - 20u - c.xlen; a.arr.out_cap[idx] = c.isize;
        idx++; content += c.isize;
    }
    if (t == 0) {
        u32 blocks = 0, max_block = 0, max_compressed = 0, flags = 0; u64 total = 0;
        for (u32 j = 0; j < threads; j++) {
            blocks += pn[j]; total += pc[j]; flags |= pfl[j];
            max_block = pmb[j] > max_block ? pmb[j] : max_block; max_compressed = pmc[j] > max_compressed ? pmc[j] : max_compressed;
        }
        int32_t status;
        if (blocks) { status = end_status; flags |= end_eof; }
        else { KBgzfHead h; status = a.size ? kx_bgzf_head(a.blob, a.size, 0, &h) : -5; }
        if (!status) { a.member_off[blocks] = a.size; a.content_off[blocks] = total; }
        kbz_stat_set(a.stat, total, blocks, max_block, max_compressed, flags, status);
    }
}

// ---- k_bgzf_verify: what the trailers say against what was decoded, a wave (a workgroup of one wave) per member -------------------
// The payloads went through kmp_inflate_batch as raw streams: a member that decoded cleanly to another size than its ISIZE gets -3, and
// with `verify` one whose CRC-32 differs from the trailer's -3 as well.  A status the decoder set stays.  The trailer stands behind
// the payload: at in_off[i] + in_len[i].
struct KBgzfVerifyArgs { const u8* blob; const u64* in_off; const u32* in_len; const u8* dst; const u64* out_off; const u32* out_len; const u32* out_cap;
                         int32_t* status; u32 n; u32 verify; };

KX_DEV void bgzf_verify_body(const KBgzfVerifyArgs& a)
{
    KX_SHARED u32 tab[256];
    int const lane = kx_lane();
    for (u32 i = kx_block(); i < a.n; i += kx_nblocks()) {
        int32_t st = a.status[i];
        u32 const len = a.out_len[i];
        if (st == 0 && len != a.out_cap[i]) st = -3;
        bool const sum = st == 0 && a.verify != 0u;              // (the same on every lane: all reach the barriers inside)
        u32 const crc = kx_wave_crc32(a.dst + a.out_off[i], sum ? len : 0u, tab, lane);
        if (sum && crc != kx_ld32(a.blob + a.in_off[i] + a.in_len[i])) st = -3;
        if (lane == 0) a.status[i] = st;
    }
}
#endif
