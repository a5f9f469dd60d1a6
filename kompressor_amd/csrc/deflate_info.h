// deflate_info.h -- how large a batch of DEFLATE streams decodes to, without decoding it: the sizing pass behind
// kmp_inflate_info_batch.  A DEFLATE stream declares no size (raw and zlib streams carry none, gzip's ISIZE stands at the end
// and is mod 2^32), so the only way to learn it is to walk the Huffman codes.  inflate_size_body is that walk, a LANE per
// stream, and writes nothing but the 32 bytes of kmp_inflate_info per stream; kmp_batch_layout takes the array as it is.
//
// What it shares with the pre-decoder (deflate_predecode.h, included, not edited): the per-lane state in LDS -- KipStream: the
// ring of input words, the 8-bit literal/length and 6-bit distance first-level tables, the canonical lists --, the
// register-held ranges of the longer codes (kip_long), and the phases: every lane tops its ring up, the lanes at a block
// header read it, then every lane walks up to KIP_SYMS symbols out of LDS.  What it does not share:
//   * no store in the symbol loop: a literal is op++, a match op += len after dist <= op (dist <= 32 768 holds by the
//     construction of the distance code: symbol 29 + 13 extra bits ends there).  No capacity, no staging; op has 64 bits.
//   * it answers for EVERY stream: stored blocks (LEN / NLEN read, the bytes skipped by re-seating the ring), the whole gzip
//     header (FEXTRA / FNAME / FCOMMENT / FHCRC), the code sets zlib accepts beyond complete ones (a set made of one code of
//     length 1; a block with no distance code that uses none), and every error: -3 (Z_DATA_ERROR) for what zlib refuses,
//     -5 (Z_BUF_ERROR) when the entry ends before its last block does -- wherever that happens: the reader counts the bits
//     it took against the bits the entry has, and a read past the end is never "zeros that happen to decode".
//   * the end: the last block must end inside the last byte of the deflate region (the entry minus wrapper and trailer);
//     bytes left over are -3.  gzip's ISIZE must equal the size mod 2^32.
// NOT verified: the Adler-32 / CRC-32 VALUES of the trailers -- there is no output to sum.  The decoder that runs afterwards
// (kmp_inflate_batch) reports them.  (The gzip header's FHCRC, a sum over header bytes, is verified, as zlib does.)
// An entry too short to hold its wrapper (zlib: 6 bytes, gzip: 18, raw: 1) is -5 whatever its bytes are.  A rejected entry
// answers its status alone: every other field is 0.
//
// Every byte is read below an explicit bound: nothing outside [in_off[i], in_off[i] + in_len[i]) is touched.
// Termination: every phase of a lane that is not finished takes at least one bit of its stream -- a symbol is at least one
// bit, a block header three, a stored block with LEN 0 thirty-two and more -- and a lane that took more bits than its entry
// has stops at the next check; so a lane runs at most 8 * in_len + 64 phases.  The loop keeps a guard on that number.
#pragma once
#include "../../include/kompressor_hip.h"
#include "deflate_predecode.h"

struct KisArgs { const u8* src; const u64* in_off; const u32* in_len; u32 n_slices; kmp_inflate_info* info; u32 format; };

// the words [w, w + 4) of a stream of nbytes bytes (zero past its end), whatever w is
KX_DEV KxQuad kis_load4(const u8* sp, u32 nbytes, u32 w)
{
    u64 const o = 4ull * w;
    if (o + 16u <= (u64)nbytes) return kx_ld128u(sp + o);
    u32 v[4] = { 0, 0, 0, 0 };
    for (u32 k = 0; k < 16u && o + k < (u64)nbytes; k++) v[k >> 2] |= (u32)sp[o + k] << (8u * (k & 3u));
    KxQuad q; q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
    return q;
}

// counts per code length; returns what is left of the code space (0: complete, < 0: over-subscribed), codes = symbols with a length
KX_DEV int kis_counts(u16* count, const u8* lens, int n, u32& codes)
{
    for (int l = 0; l < 16; l++) count[l] = 0;
    for (int s = 0; s < n; s++) count[lens[s]]++;
    codes = (u32)n - count[0];
    count[0] = 0;
    int left = 1;
    for (int l = 1; l < 16; l++) { left <<= 1; left -= count[l]; if (left < 0) return -1; }
    return left;
}

// CRC-32 (the gzip polynomial) of a few header bytes, bit by bit: a gzip header with FHCRC is rare and short
KX_DEV u32 kis_crc32(const u8* p, u32 n)
{
    u32 c = 0xFFFFFFFFu;
    for (u32 i = 0; i < n; i++) { c ^= p[i]; for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u))); }
    return ~c;
}

// The wrapper of an entry: where its deflate region lies (src[spos, send)), the info flags and the window.  0 or the status.
KX_DEV int kis_wrapper(const u8* src, u32 srcSize, u32 format, u32& spos, u32& send, u32& flags, u32& wbits)
{
    u32 fmt = format & 0xFFu; u32 const wmax = (format >> 8) ? (format >> 8) : 15u;
    spos = 0; send = srcSize; flags = 0; wbits = 0;
    if (fmt == 3) fmt = (srcSize >= 2 && src[0] == 0x1F && src[1] == 0x8B) ? 2u : 1u;
    if (fmt == 2) {
        if (srcSize < 18) return KI_BUF_ERROR;
        if (src[0] != 0x1F || src[1] != 0x8B || src[2] != 8 || (src[3] & 0xE0)) return KI_DATA_ERROR;
        u32 const flg = src[3]; u32 p = 10; u32 const lim = srcSize - 8;          // (p <= lim from here on, checked before every read)
        if (flg & 4u) {
            if (lim - p < 2u) return KI_BUF_ERROR;
            u32 const xlen = (u32)src[p] | ((u32)src[p + 1] << 8); p += 2;
            if (lim - p < xlen) return KI_BUF_ERROR;
            p += xlen;
        }
        for (u32 bit = 8u; bit <= 16u; bit <<= 1) if (flg & bit) {                // FNAME, then FCOMMENT: to the zero byte
            while (p < lim && src[p]) p++;
            if (p >= lim) return KI_BUF_ERROR;
            p++;
        }
        if (flg & 2u) {
            if (lim - p < 2u) return KI_BUF_ERROR;
            if ((kis_crc32(src, p) & 0xFFFFu) != ((u32)src[p] | ((u32)src[p + 1] << 8))) return KI_DATA_ERROR;
            p += 2;
        }
        spos = p; send = lim; flags = 8u | ((flg & 0x1Eu) ? 16u : 0u);
        return 0;
    }
    if (fmt == 1) {
        if (srcSize < 6) return KI_BUF_ERROR;
        u32 const cmf = src[0], flg = src[1];
        if ((cmf & 0x0F) != 8 || (cmf >> 4) + 8u > wmax || ((cmf << 8) | flg) % 31 != 0 || (flg & 0x20)) return KI_DATA_ERROR;
        spos = 2; send = srcSize - 4; wbits = (cmf >> 4) + 8u;
    }
    return 0;
}

// bits of the stream taken so far; more than it has: the entry ended first
#define KIS_USED() (32ull * (u64)br.rp - (u64)(u32)br.cnt)
#define KIS_OVER() (KIS_USED() > 8ull * (u64)nbytes)
// at least 32 bits in the container afterwards (zeros past the end of the stream: KIS_OVER tells)
#define KIS_FILL() { if (br.cnt <= 32) { \
        if (br.rp == br.wp) { KxQuad const q_ = kis_load4(sp, nbytes, br.wp); kip_put4(S, br, q_); } \
        br.buf |= (u64)S.ring[br.rp & (KIP_RING - 1)] << br.cnt; br.cnt += 32; br.rp++; } }
#define KIS_TAKE(dst_, n_) { u32 const n__ = (n_); dst_ = (u32)(br.buf & ((1ull << n__) - 1ull)); br.buf >>= n__; br.cnt -= (int)n__; }
// this lane is done with status e_ -- unless it has already read past its end: then nothing it saw since counts, and zlib would
// still be waiting for input
#define KIS_FAIL(e_) { st = KIS_OVER() ? (int)KI_BUF_ERROR : (int)(e_); fin = true; }
#define KIS_INVALID (511u | (1u << 9))          /* first-level entry of a code no symbol has (incomplete sets): one bit, symbol 511 */

KX_DEV void inflate_size_body(const KisArgs& a)
{
    KX_SHARED KipStream lds[KIP_STREAMS];
    int const lane = kx_lane();
    bool const mine = lane < KIP_STREAMS;
    u32 const f = kx_block() * (u32)KIP_STREAMS + (u32)(mine ? lane : 0);
    bool const live = mine && f < a.n_slices;
    KipStream& S = lds[mine ? lane : 0];
    const u8* sp = a.src; u32 nbytes = 0;
    const u8* src = a.src; u32 srcSize = 0;
    int st = 0; u32 flags = 0, wbits = 0, blocks = 0;
    if (live) {
        src = a.src + a.in_off[f]; srcSize = a.in_len[f];
        u32 spos, send;
        st = kis_wrapper(src, srcSize, a.format, spos, send, flags, wbits);
        if (!st) { sp = src + spos; nbytes = send - spos; }
    }
    KipBits br; br.buf = 0; br.cnt = 0; br.rp = 0; br.wp = 0;
    u32 nwords = (u32)(((u64)nbytes + 3u) >> 2);
    bool fin = !live || st != 0;                             // this lane has nothing more to do
    bool inBlock = false, last = false;
    u64 op = 0;                                              // bytes the stream has decoded to
    u64 const max_phases = 8ull * srcSize + 64u; u64 phases = 0;
    KipLong LL, DL;                                          // the long codes of the block
    LL.e[0] = LL.e[1] = LL.e[2] = LL.e[3] = 0; LL.lo0 = 0; LL.ib = 0; DL = LL;
    while (kx_any(!fin)) {
        if (!fin && ++phases > max_phases) { st = KI_DATA_ERROR; fin = true; }       // (the guard: see the head of this file)
        // ---- top the ring up: every free group of four words, up to eight groups ----------------------------------------
        {
            KxQuad q[8]; u32 const wp0 = br.wp; u32 const room = KIP_RING - (br.wp - br.rp);
#pragma unroll
            for (int u = 0; u < 8; u++) { q[u].x = 0; q[u].y = 0; q[u].z = 0; q[u].w = 0; if (!fin && room >= 4u * (u32)(u + 1) && wp0 + 4u * (u32)u < nwords) q[u] = kis_load4(sp, nbytes, wp0 + 4u * (u32)u); }
#pragma unroll
            for (int u = 0; u < 8; u++) if (!fin && room >= 4u * (u32)(u + 1) && wp0 + 4u * (u32)u < nwords) kip_put4(S, br, q[u]);
        }
        // ---- block headers -----------------------------------------------------------------------------------------------
        if (!fin && !inBlock) {
            if (last) {
                // the stream must end inside the last byte of its region and leave nothing behind
                if (((KIS_USED() + 7u) >> 3) != (u64)nbytes) st = KI_DATA_ERROR;
                else if (flags & 8u) {
                    u32 const isize = (u32)src[srcSize - 4] | ((u32)src[srcSize - 3] << 8) | ((u32)src[srcSize - 2] << 16) | ((u32)src[srcSize - 1] << 24);
                    if (isize != (u32)op) st = KI_DATA_ERROR;
                }
                fin = true;
            } else {
                u32 hdr; KIS_FILL() KIS_TAKE(hdr, 3)
                last = hdr & 1u; u32 const btype = hdr >> 1;
                blocks++;
                if (btype == 3) KIS_FAIL(KI_DATA_ERROR)
                else if (btype == 0) {
                    // stored: to the byte boundary, LEN / NLEN, then LEN bytes are skipped by re-seating the ring behind them
                    u32 const drop = (u32)br.cnt & 7u; br.buf >>= drop; br.cnt -= (int)drop;
                    u32 len, nlen; KIS_FILL() KIS_TAKE(len, 16) KIS_TAKE(nlen, 16)
                    if (KIS_OVER() || (len ^ 0xFFFFu) != nlen) KIS_FAIL(KI_DATA_ERROR)
                    else {
                        u32 const at = (u32)(KIS_USED() >> 3);                         // (<= nbytes: not over)
                        if (len > nbytes - at) { st = KI_BUF_ERROR; fin = true; }
                        else {
                            sp += at + len; nbytes -= at + len; nwords = (u32)(((u64)nbytes + 3u) >> 2);
                            br.buf = 0; br.cnt = 0; br.rp = 0; br.wp = 0;
                            op += len; flags |= 1u;
                        }
                    }
                } else {
                    u32 hlit = 288, hdist = 32;
                    flags |= btype == 1 ? 2u : 4u;
                    if (btype == 1) {
                        // (the fixed codes: 288 literal/length symbols, of which 286 and 287 never stand in a valid stream, and 32
                        //  distance symbols of 5 bits, of which 30 and 31 do not: the symbol loop refuses them when they come)
                        for (int s = 0; s < 288; s++) S.t.lens[s] = (u8)kd_static_llen((u32)s);
                        for (int s = 0; s < 32; s++) S.t.lens[288 + s] = 5;
                    } else {
                        u32 hclen; KIS_FILL() KIS_TAKE(hlit, 5) KIS_TAKE(hdist, 5) KIS_TAKE(hclen, 4)
                        hlit += 257; hdist += 1; hclen += 4;
                        if (hlit > 286 || hdist > 30) KIS_FAIL(KI_DATA_ERROR)
                        else {
                            // the code-length code: at most 7 bits, read by the canonical walk
                            // (its lengths, counts and sorted list borrow the distance lists, which are built after it)
                            u8* const cl = S.dsort; u16* const ccount = S.dcount; u8* const csort = S.lsortHi;
                            for (int i = 0; i < 19; i++) cl[i] = 0;
                            for (u32 i = 0; i < hclen; i++) {
                                u32 v; KIS_FILL() KIS_TAKE(v, 3)
                                u32 const pos = i < 3 ? 16u + i : (i == 3 ? 0u : ((i & 1u) ? 7u - ((i - 5u) >> 1) : 8u + ((i - 4u) >> 1)));   // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
                                cl[pos] = (u8)v;
                            }
                            u32 ccodes = 0;
                            int const cleft = kis_counts(ccount, cl, 19, ccodes);
                            if (ccodes == 0) {
                                // zlib builds a table of one-bit invalid entries for a set without codes and reads every length from
                                // it as 0: hlit + hdist bits go by, and the block has no end-of-block code
                                for (u32 i = 0; i < hlit + hdist; i += 32u) { u32 x; u32 const k = hlit + hdist - i < 32u ? hlit + hdist - i : 32u; KIS_FILL() KIS_TAKE(x, k) (void)x; }
                                KIS_FAIL(KI_DATA_ERROR)
                            }
                            else if (cleft != 0) KIS_FAIL(KI_DATA_ERROR)
                            else {
                                S.offs[1] = 0;
                                for (int l = 1; l < 15; l++) S.offs[l + 1] = (u16)(S.offs[l] + ccount[l]);
                                for (u32 s = 0; s < 19; s++) if (cl[s]) csort[S.offs[cl[s]]++] = (u8)s;
                                u32 idx = 0, prevLen = 0;
                                while (idx < hlit + hdist && !fin) {
                                    KIS_FILL()
                                    u32 index = 0, clen = 0;
                                    if (!kip_walk(br.buf, ccount, index, clen) || clen > 7) { KIS_FAIL(KI_DATA_ERROR) break; }
                                    br.buf >>= clen; br.cnt -= (int)clen;
                                    u32 const sym = csort[index];
                                    if (sym < 16) { S.t.lens[idx++] = (u8)sym; prevLen = sym; }
                                    else {
                                        u32 rep, val = 0, x;
                                        if (sym == 16) { if (idx == 0) { KIS_FAIL(KI_DATA_ERROR) break; } KIS_TAKE(x, 2) rep = 3 + x; val = prevLen; }
                                        else if (sym == 17) { KIS_TAKE(x, 3) rep = 3 + x; }
                                        else { KIS_TAKE(x, 7) rep = 11 + x; }
                                        if (idx + rep > hlit + hdist) { KIS_FAIL(KI_DATA_ERROR) break; }
                                        while (rep--) S.t.lens[idx++] = (u8)val;
                                        prevLen = val;
                                    }
                                }
                                if (!fin && (KIS_OVER() || S.t.lens[256] == 0)) KIS_FAIL(KI_DATA_ERROR)       // no end-of-block code
                            }
                        }
                    }
                    if (!fin) {
                        // distance side first (its lengths sit behind the literal/length ones, whose table then takes their place).
                        // zlib's rule for both sets: over-subscribed is an error; incomplete is one unless the set is a single code of
                        // length 1 -- or, for distances, no code at all: then every entry is invalid, and a match is the error
                        const u8* const dl = S.t.lens + hlit;
                        u32 dcodes = 0, lcodes = 0;
                        int const dleft = kis_counts(S.dcount, dl, (int)hdist, dcodes);
                        bool good = dleft == 0 || (dleft > 0 && (dcodes == 0 || (dcodes == 1 && S.dcount[1] == 1)));
                        if (good) {
                            S.offs[1] = 0;
                            for (int l = 1; l < 15; l++) S.offs[l + 1] = (u16)(S.offs[l] + S.dcount[l]);
                            for (int i = 0; i < 32; i++) S.dsort[i] = 99;
                            for (u32 s = 0; s < hdist; s++) if (dl[s]) S.dsort[S.offs[dl[s]]++] = (u8)s;
                            for (int i = 0; i < 64; i++) S.d1[i] = dleft ? (u16)KIS_INVALID : (u16)0;
                            u32 code = 0, k = 0;
                            for (u32 l = 1; l <= 15; l++) {
                                for (u32 c = 0; c < S.dcount[l]; c++, k++, code++) {
                                    if (l <= 6) { u32 const rev = kd_bi_reverse(code, (int)l); for (u32 i = rev; i < 64u; i += 1u << l) S.d1[i] = (u16)((u32)S.dsort[k] | (l << 9)); }
                                }
                                code <<= 1;
                            }
                            kip_long_build<6, 5>(S.dcount, DL);
                            int const lleft = kis_counts(S.lcount, S.t.lens, (int)hlit, lcodes);
                            good = lleft == 0 || (lleft > 0 && lcodes == 1 && S.lcount[1] == 1);
                            if (good) {
                                S.offs[1] = 0;
                                for (int l = 1; l < 15; l++) S.offs[l + 1] = (u16)(S.offs[l] + S.lcount[l]);
                                for (int i = 0; i < 36; i++) S.lsortHi[i] = 0;
                                for (u32 s = 0; s < hlit; s++) {
                                    u32 const l = S.t.lens[s];
                                    if (l) { u32 const o = S.offs[l]++; S.lsortLo[o] = (u8)s; if (s & 256u) S.lsortHi[o >> 3] |= (u8)(1u << (o & 7u)); }
                                }
                                for (int i = 0; i < 256; i++) S.t.l1[i] = lleft ? (u16)KIS_INVALID : (u16)0;      // (the lengths are gone from here on)
                                u32 code2 = 0, k2 = 0;
                                for (u32 l = 1; l <= 15; l++) {
                                    u32 const cnt = S.lcount[l];
                                    if (l <= 8) for (u32 c = 0; c < cnt; c++, k2++, code2++) {
                                        u32 const rev = kd_bi_reverse(code2, (int)l); u32 const e = kip_lsym(S, k2) | (l << 9);
                                        for (u32 i = rev; i < 256u; i += 1u << l) S.t.l1[i] = (u16)e;
                                    }
                                    else { k2 += cnt; code2 += cnt; }
                                    code2 <<= 1;
                                }
                                kip_long_build<8, 9>(S.lcount, LL);
                                inBlock = true;
                            }
                        }
                        if (!good) KIS_FAIL(KI_DATA_ERROR)
                    }
                }
            }
        }
        // ---- symbols: nothing is stored -----------------------------------------------------------------------------------
        for (int n = 0; n < KIP_SYMS; n++) {
            bool const go = !fin && inBlock && ((br.wp - br.rp) >= 2u || br.wp >= nwords);      // 64 bits at hand besides the container, or the stream's tail
            if (!kx_any(go)) break;
            if (go) {
                KIS_FILL()
                u32 e = S.t.l1[br.buf & 255u]; u32 sym, clen = e >> 9;
                if (clen) sym = e & 511u;
                else {
                    u32 index = 0;
                    kip_long<8, 9>(br.buf, LL, index, clen);
                    sym = index < 288u ? kip_lsym(S, index) : 999u;
                }
                br.buf >>= clen; br.cnt -= (int)clen;
                if (sym < 256) op++;
                else if (sym == 256) inBlock = false;
                else if (sym > 285) KIS_FAIL(KI_DATA_ERROR)
                else {
                    u32 const lc = sym - 257; u32 len, x;
                    if (lc < 8) len = 3 + lc; else if (lc == 28) len = 258;
                    else { u32 const eb = (lc - 4) >> 2; KIS_TAKE(x, eb) len = 3 + ((4 + (lc & 3u)) << eb) + x; }
                    KIS_FILL()
                    u32 de = S.d1[br.buf & 63u]; u32 dsym, dlen = de >> 9;
                    if (dlen) dsym = de & 511u;
                    else {
                        u32 index = 0;
                        kip_long<6, 5>(br.buf, DL, index, dlen);
                        dsym = index < 32u ? S.dsort[index] : 99u;
                    }
                    br.buf >>= dlen; br.cnt -= (int)dlen;
                    if (dsym > 29) KIS_FAIL(KI_DATA_ERROR)
                    else {
                        u32 dist;
                        if (dsym < 4) dist = dsym + 1; else { u32 const eb = (dsym - 2) >> 1; KIS_TAKE(x, eb) dist = 1 + ((2 + (dsym & 1u)) << eb) + x; }
                        if ((u64)dist > op) KIS_FAIL(KI_DATA_ERROR)
                        else op += len;
                    }
                }
                if (!fin && KIS_OVER()) { st = KI_BUF_ERROR; fin = true; }                      // the entry ended inside this symbol
            }
        }
    }
    if (live) {
        kmp_inflate_info r;
        bool const ok = st == 0;
        r.content = ok ? op : 0; r.bound = r.content; r.status = st;
        r.blocks = ok ? blocks : 0u; r.flags = ok ? flags : 0u; r.window_bits = ok ? wbits : 0u;
        a.info[f] = r;
    }
}
#undef KIS_USED
#undef KIS_OVER
#undef KIS_FILL
#undef KIS_TAKE
#undef KIS_FAIL
#undef KIS_INVALID
