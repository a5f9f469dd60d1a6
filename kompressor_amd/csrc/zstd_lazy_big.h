// zstd_lazy_big.h -- zstd levels 5 .. 10 for slices of 128 KiB + 1 .. 2 MiB: frames of several blocks, as ZSTD_compress2 writes them into a
// buffer of ZSTD_compressBound bytes.  No dictionary; the window never moves (windowLog covers the slice), so there is no extDict variant.
//
// What libzstd does: ZSTD_compress_frameChunk cuts the input into blocks (128 KiB, or where the pre-splitter sees the statistics change once
// the frame has saved 3 bytes), parses each with ZSTD_compressBlock_lazy_generic (depth 0 / 1 / 2) over the row-based match finder, and
// carries from block to block: the row table and its tags, nextToUpdate (with the catch-up rule after a long match), the repeat offsets,
// the literals' Huffman table and the three sequence tables.  Block k + 1's size needs block k's compressed size, so parse and frame step
// alternate: one wave owns a slice and walks the chain (k_zstd_big's shape).
//
// Unlike the one-block kernels of zstd_lazy.h (which sort the positions first: every position of a block enters the tables, so a position's
// candidates are known before the parse), this parser keeps libzstd's own tables in device memory, per slice: 4 bytes x 2^hashLog of
// positions and 1 byte x 2^hashLog of tags (20 MiB at level 10 above 1 MiB).  A row (16 / 32 / 64 entries) is one wave-wide look; the
// positions between two searches go in 64 at a time, lanes of one row in turn.
#pragma once
#include "zstd_entropy.h"
#include "zstd_lazy.h"

#define KX_LAZY_BIG_MAX (2u << 20)            /* the oracle (and libzstd's parameter table as restated here) is pinned up to 2 MiB */

// ZSTD_getCParams(level, n, 0) for 128 KiB < n <= 2 MiB at levels 5 .. 10 (tests/golden/zstd_lazy_big_golden.json "params"); strat 0: not served
struct KLazyBigPar { u32 W, H, S, mml, strat, rowLog; };
KX_DEV KLazyBigPar kx_lazy_big_params(u32 level, u32 n)
{
    KLazyBigPar p; p.W = 0; p.H = 0; p.S = 0; p.mml = 0; p.strat = 0; p.rowLog = 0;
    if (n <= KX_BLOCK_MAX || n > KX_LAZY_BIG_MAX || level < 5u || level > 10u) return p;
    u32 const l = level - 5u;
    if (n <= 262144u) {
        static const u32 Ht[6] = { 18, 19, 19, 19, 19, 19 };
        static const u32 St[6] = { 5, 3, 4, 4, 5, 6 }; static const u32 Mt[6] = { 5, 5, 4, 4, 4, 4 }; static const u32 Tt[6] = { 3, 4, 4, 5, 5, 5 };
        p.W = 18; p.H = Ht[l]; p.S = St[l]; p.mml = Mt[l]; p.strat = Tt[l];
    } else {
        static const u32 Wt[6] = { 21, 21, 21, 21, 22, 22 };
        static const u32 Ht[6] = { 19, 19, 20, 20, 21, 22 }; static const u32 St[6] = { 3, 3, 4, 4, 4, 5 }; static const u32 Tt[6] = { 3, 4, 4, 5, 5, 5 };
        p.W = Wt[l]; p.H = Ht[l]; p.S = St[l]; p.mml = 5; p.strat = Tt[l];
    }
    u32 const srcLog = kx_hb32(n - 1u) + 1u;
    if (p.W > srcLog) p.W = srcLog;
    if (p.H > p.W + 1u) p.H = p.W + 1u;
    p.rowLog = p.S < 4u ? 4u : p.S > 6u ? 6u : p.S;
    return p;
}
// ... and level 4's one "greedy" row above a block: ZSTD_getCParams(4, 128 KiB < n <= 256 KiB) = { 18, 16, 17, 3, 5, 2, greedy } (its other rows
// above 16 KiB are double-fast: kx_params_l4).  n > 2^17, so neither clamp to the source applies.  One-shot frames only.
KX_DEV KLazyBigPar kx_lazy_big_params_l4(u32 n)
{
    KLazyBigPar p; p.W = 0; p.H = 0; p.S = 0; p.mml = 0; p.strat = 0; p.rowLog = 0;
    if (n > KX_BLOCK_MAX && n <= 262144u) { p.W = 18; p.H = 17; p.S = 3; p.mml = 5; p.strat = 3; p.rowLog = 4; }
    return p;
}
// what the one-shot chain kernel runs a slice with at a.level
KX_DEV KLazyBigPar kx_lazy_big_params_one_shot(u32 level, u32 n) { return level == 4u ? kx_lazy_big_params_l4(n) : kx_lazy_big_params(level, n); }
// A stream (size unknown when the frame starts) gets the unknown-size row whatever its length turns out to be, 0 .. 2 MiB: the row above
// 256 KiB without the clamps to the source size, minMatch 5 (tests/golden/zstd_lazy_stream_golden.json "params")
KX_DEV KLazyBigPar kx_lazy_big_params_stream(u32 level, u32 n)
{
    KLazyBigPar p; p.W = 0; p.H = 0; p.S = 0; p.mml = 0; p.strat = 0; p.rowLog = 0;
    if (n > KX_LAZY_BIG_MAX || level < 5u || level > 10u) return p;
    u32 const l = level - 5u;
    static const u32 Wt[6] = { 21, 21, 21, 21, 22, 22 };
    static const u32 Ht[6] = { 19, 19, 20, 20, 21, 22 }; static const u32 St[6] = { 3, 3, 4, 4, 4, 5 }; static const u32 Tt[6] = { 3, 4, 4, 5, 5, 5 };
    p.W = Wt[l]; p.H = Ht[l]; p.S = St[l]; p.mml = 5; p.strat = Tt[l];
    p.rowLog = p.S < 4u ? 4u : p.S > 6u ? 6u : p.S;
    return p;
}
// mode: KFrameArgs.stream.  The staged frames of the reference's driver (KXF_REFERENCE) know their size: the parameters of the one-shot frames
KX_DEV KLazyBigPar kx_lazy_big_params_mode(u32 level, u32 n, u32 mode)
{
    return (mode == KXF_STREAM || mode == KXF_STREAM_EMPTY_END) ? kx_lazy_big_params_stream(level, n) : kx_lazy_big_params(level, n);
}
// the largest hashLog a slice of up to cap bytes can get (level 10): what a slice's table slot is sized by (5 bytes << this)
inline u32 kx_lazy_big_hash_log_max(u32 cap)
{
    if (cap > KX_LAZY_BIG_MAX) cap = KX_LAZY_BIG_MAX;
    if (cap <= 262144u) return 19u;
    u32 srcLog = 0; while ((1u << srcLog) < cap) srcLog++;
    return srcLog + 1u < 22u ? srcLog + 1u : 22u;
}
// ... and a stream's at a level, whatever its length
inline u32 kx_lazy_big_hash_log_stream(int level) { static const u32 Ht[6] = { 19, 19, 20, 20, 21, 22 }; return (level >= 5 && level <= 10) ? Ht[level - 5] : 22u; }

struct KLazyBigArgs {
    KFrameArgs e;                 // the frame step's arguments (strategy / level2 / cls unused)
    u32 level;
    u8* tables; u64 slot_bytes;   // per slice of the launch: 4 << H bytes of positions (index = position + 2, 0 = empty), then 1 << H bytes of tags
    KSeqPrev* prev;               // per slice: the previous block's sequence tables
    KSeq* seqs_w; KSliceMeta* meta_w;      // (the parse's side of e.seqs / e.meta)
};

// This block's part of the chain, beside KFrameState (in registers: the wave walks the whole chain)
struct KLazyBigState { u32 ntu; };           // ms->nextToUpdate as a position of the slice

struct KLazyBigLds { u32 mark[1024]; u32 split[2048]; };      // row marks of an insert step; the pre-splitter's fingerprints

// positions [from, to) enter the row table in order (ZSTD_row_update_internal without its gap rule: the caller applies it)
KX_DEV void kzlb_insert_range(const u8* src, u32* hashTable, u8* tagTable, const KLazyBigPar& P, KLazyBigLds& l2, u32 from, u32 to, int lane)
{
    u32 const rowMask = (1u << P.rowLog) - 1u, hBits = P.H - P.rowLog + 8u;
    for (u32 base = from; base < to; base += 64u) {
        u32 const p = base + (u32)lane; bool const valid = p < to;
        u32 const hash = valid ? kx_hash_short(kx_ld64(src + p), hBits, P.mml) : 0u;
        u32 const relRow = (hash >> 8) << P.rowLog;
        // lanes of one row take their turn in position order: rank r of k.  Most lanes are alone in their row: a lane finds out through a
        // mark in LDS (1 024 marks: a lane that reads another's mark shares its row, or its mark only; the ballots below sort that out)
        u32 rk = 0, grpN = 1;
        if (to - base > 1u) {
            u32 const mk = (relRow >> P.rowLog) & 1023u;
            if (valid) l2.mark[mk] = (u32)lane;
            kx_lockstep();
            bool const shared = valid && l2.mark[mk] != (u32)lane;
            for (u64 todo = kx_ballot(shared); todo; ) {
                int const L = (int)kx_ctz64(todo);
                u32 const rowL = kx_bcast(relRow, L);
                u64 const grp = kx_ballot(valid && relRow == rowL);
                if (valid && relRow == rowL) { rk = kx_popc64(grp & ((1ull << lane) - 1ull)); grpN = kx_popc64(grp); }
                todo &= ~grp;
            }
        }
        // ZSTD_row_nextIndex j times from the row's head: the slots run mask, mask - 1, .. 1, mask, ..
        u32 const head = valid ? (u32)tagTable[relRow] & rowMask : 0u;
        kx_lockstep();
        u32 const h0 = head ? head : 1u;
        u32 const mypos = (h0 - 1u + rowMask * 64u - (rk + 1u)) % rowMask + 1u;
        if (valid && rk + rowMask >= grpN) { tagTable[relRow + mypos] = (u8)hash; hashTable[relRow + mypos] = p + 2u; }      // (a slot taken twice in one step keeps the later position)
        if (valid && rk + 1u == grpN) tagTable[relRow] = (u8)mypos;
        kx_lockstep();
    }
}

// ZSTD_RowFindBestMatch at position cur (wave-uniform): longest match among the row's entries with cur's tag, newest first, at most nbAttempts;
// cur itself enters the row.  ml 3 = nothing.  iend: the block's end (matches stop there).
KX_DEV void kzlb_find(const u8* src, u32* hashTable, u8* tagTable, const KLazyBigPar& P, KLazyBigLds& l2, KLazyBigState& st, bool skipping,
                      u32 cur, u32 iend, int lane, u32& mlOut, u32& offOut)
{
    u32 const rowEntries = 1u << P.rowLog, rowMask = rowEntries - 1u, hBits = P.H - P.rowLog + 8u;
    u32 const nbAttempts = 1u << (P.S < P.rowLog ? P.S : P.rowLog);
    if (!skipping) {
        // ZSTD_row_update: everything since nextToUpdate; of a gap above 384 the first 96 and the last 32 positions only
        if (cur - st.ntu > 384u) { kzlb_insert_range(src, hashTable, tagTable, P, l2, st.ntu, st.ntu + 96u, lane); st.ntu = cur - 32u; }
        kzlb_insert_range(src, hashTable, tagTable, P, l2, st.ntu, cur, lane);
    }
    st.ntu = cur;
    u64 const scan = kx_ld64(src + cur);
    u32 const hash = kx_hash_short(scan, hBits, P.mml), tag = hash & 0xFFu;
    u32 const relRow = (hash >> 8) << P.rowLog;
    bool const mine = (u32)lane < rowEntries;
    u32 const tg = mine ? (u32)tagTable[relRow + (u32)lane] : 0u;
    u32 const head = kx_bcast(tg, 0) & rowMask;
    bool const hit = mine && lane != 0 && tg == tag;
    u32 const idx = hit ? hashTable[relRow + (u32)lane] : 0u;
    u64 const hitM = kx_ballot(hit), emptyM = kx_ballot(hit && idx < 2u);
    // in the order the row is walked: slot (head + k) & mask is the k-th
    u32 const k = ((u32)lane - head) & rowMask;
    u64 const full = rowEntries == 64u ? ~0ull : ((1ull << rowEntries) - 1ull);
    u64 const hitR = head ? ((hitM >> head) | (hitM << (rowEntries - head))) & full : hitM;
    u64 const emptyR = head ? ((emptyM >> head) | (emptyM << (rowEntries - head))) & full : emptyM;
    u32 const stopK = emptyR ? (u32)kx_ctz64(emptyR) : 64u;          // an empty entry ends the walk
    u32 const rank = kx_popc64(hitR & ((1ull << k) - 1ull));
    bool const cand = hit && k < stopK && rank < nbAttempts;
    u32 len = 0;
    if (cand) {
        u32 const cp = idx - 2u; u32 const room = iend - cur;
        u64 const x = scan ^ kx_ld64(src + cp);
        if (x) len = (u32)(kx_ctz64(x) >> 3);
        else {
            len = 8;
            while (len < room) {
                u64 const y = kx_ld64_clamped(src, (int)(cur + len), (int)iend) ^ kx_ld64_clamped(src, (int)(cp + len), (int)iend);
                if (y) { len += (u32)(kx_ctz64(y) >> 3); break; }
                len += 8u;
            }
        }
        if (len > room) len = room;
    }
    // the longest wins, the one walked first among equals
    u32 key = (cand && len > 3u) ? (len << 6) | (63u - rank) : 0u, who = cand ? idx - 2u : 0u;
    for (int o = 32; o >= 1; o >>= 1) {
        u32 const tk = kx_shfl(key, lane ^ o), tw = kx_shfl(who, lane ^ o);
        if (tk > key) { key = tk; who = tw; }
    }
    // cur enters its row (every lane has read the row by now)
    if (lane == 0) {
        u32 const h0 = head ? head : 1u;
        u32 const pos = (h0 - 1u + rowMask - 1u) % rowMask + 1u;
        tagTable[relRow] = (u8)pos; tagTable[relRow + pos] = (u8)tag; hashTable[relRow + pos] = cur + 2u;
    }
    kx_lockstep();
    st.ntu = cur + 1u;
    mlOut = key ? key >> 6 : 3u; offOut = key ? cur - who : 0u;
}

// ZSTD_compressBlock_lazy_generic over the block [b0, b0 + bs) of a slice (positions of the slice; the frame began at 0).  rep: in / out.
KX_DEV void kzlb_parse_block(const u8* src, u32 b0, u32 bs, u32* hashTable, u8* tagTable, const KLazyBigPar& P, KLazyBigLds& l2, KLazyBigState& st,
                             u32 rep0, u32 rep1, KSeq* seqs, u32 seq_cap, KSliceMeta* metaOut, int lane)
{
    u32 const iend = b0 + bs, depth = P.strat - 3u;
    KSliceMeta mm; mm.nbSeq = 0; mm.litSize = 0; mm.lastLL = bs; mm.longType = 0; mm.longPos = 0; mm.status = 0; mm.pad[0] = rep0; mm.pad[1] = rep1;
    u32 ip = b0, anchor = b0, off1 = rep0, off2 = rep1, saved1 = 0, saved2 = 0;
    if (ip == 0) ip = 1;
    { u32 const maxRep = ip; if (off2 > maxRep) { saved2 = off2; off2 = 0; } if (off1 > maxRep) { saved1 = off1; off1 = 0; } }
    // limited update after a very long match (ZSTD_compressBlock_internal)
    if (b0 > st.ntu + 384u) { u32 const gap = b0 - st.ntu - 384u; st.ntu = b0 - (gap < 192u ? gap : 192u); }
    bool skipping = false;
    u32 nseq = 0, nlit = 0, longType = 0, longPos = 0, guard = 0;
    auto store = [&](u32 ll, u32 offBase, u32 ml) {
        u32 const mlb = ml - 3u;
        if (ll > 0xFFFFu) { longType = 1; longPos = nseq; }
        if (mlb > 0xFFFFu) { longType = 2; longPos = nseq; }
        if (lane == 0 && nseq < seq_cap) { KSeq q; q.offBase = offBase; q.litLength = (u16)ll; q.mlBase = (u16)mlb; seqs[nseq] = q; }
        nseq++; nlit += ll;
    };
    if (bs > 16u) {
        u32 const ilimit = iend - 16u;
        while (ip < ilimit) {
            if (++guard > 400000u) { mm.status = 2; break; }
            u32 matchLength = 0, offBase = 1, start = ip + 1u;
            bool stored = false;
            if (off1 > 0 && kx_ld32(src + ip + 1u - off1) == kx_ld32(src + ip + 1u)) {
                matchLength = kzl_count_wave(src, ip + 5u, ip + 5u - off1, iend, lane) + 4u;
                if (depth == 0) stored = true;
            }
            if (!stored) {
                u32 ml2, of2; kzlb_find(src, hashTable, tagTable, P, l2, st, skipping, ip, iend, lane, ml2, of2);
                if (ml2 > matchLength) { matchLength = ml2; start = ip; offBase = of2 + 3u; }
                if (matchLength < 4u) {
                    u32 const step = ((ip - anchor) >> 8) + 1u;
                    ip += step;
                    skipping = step > 8u;
                    continue;
                }
                if (depth >= 1u)
                while (ip < ilimit) {
                    ip++;
                    if (off1 > 0 && kx_ld32(src + ip) == kx_ld32(src + ip - off1)) {
                        u32 const mlRep = kzl_count_wave(src, ip + 4u, ip + 4u - off1, iend, lane) + 4u;
                        int const gain2 = (int)(mlRep * 3u), gain1 = (int)(matchLength * 3u - kx_hb32(offBase) + 1u);
                        if (mlRep >= 4u && gain2 > gain1) { matchLength = mlRep; offBase = 1; start = ip; }
                    }
                    {
                        u32 ml3, of3; kzlb_find(src, hashTable, tagTable, P, l2, st, skipping, ip, iend, lane, ml3, of3);
                        int const gain2 = (int)(ml3 * 4u - kx_hb32(ml3 > 3u ? of3 + 3u : 999999999u)), gain1 = (int)(matchLength * 4u - kx_hb32(offBase) + 4u);
                        if (ml3 >= 4u && gain2 > gain1) { matchLength = ml3; offBase = of3 + 3u; start = ip; continue; }
                    }
                    if (depth == 2u && ip < ilimit) {
                        ip++;
                        if (off1 > 0 && kx_ld32(src + ip) == kx_ld32(src + ip - off1)) {
                            u32 const mlRep = kzl_count_wave(src, ip + 4u, ip + 4u - off1, iend, lane) + 4u;
                            int const gain2 = (int)(mlRep * 4u), gain1 = (int)(matchLength * 4u - kx_hb32(offBase) + 1u);
                            if (mlRep >= 4u && gain2 > gain1) { matchLength = mlRep; offBase = 1; start = ip; }
                        }
                        {
                            u32 ml3, of3; kzlb_find(src, hashTable, tagTable, P, l2, st, skipping, ip, iend, lane, ml3, of3);
                            int const gain2 = (int)(ml3 * 4u - kx_hb32(ml3 > 3u ? of3 + 3u : 999999999u)), gain1 = (int)(matchLength * 4u - kx_hb32(offBase) + 7u);
                            if (ml3 >= 4u && gain2 > gain1) { matchLength = ml3; offBase = of3 + 3u; start = ip; continue; }
                        }
                    }
                    break;
                }
                if (offBase > 3u) {
                    // catch up: bytes before the match that agree too (not before the anchor, not before the slice's first byte)
                    u32 const off = offBase - 3u;
                    u32 const lim1 = start - anchor, lim2 = start - off;          // start - off > prefixLowest = 0
                    u32 const maxBack = lim1 < lim2 ? lim1 : lim2;
                    u32 back = 0;
                    for (u32 done = 0; done < maxBack; done += 64u) {
                        u32 const kk = done + (u32)lane;
                        bool const ne = kk >= maxBack || src[start - 1u - kk] != src[start - off - 1u - kk];
                        u64 const stop = kx_ballot(ne);
                        if (stop) { back = done + (u32)kx_ctz64(stop); break; }
                        back = done + 64u;
                    }
                    if (back > maxBack) back = maxBack;
                    start -= back; matchLength += back;
                    off2 = off1; off1 = off;
                }
            }
            store(start - anchor, offBase, matchLength);
            anchor = ip = start + matchLength;
            skipping = false;
            while (ip <= ilimit && off2 > 0 && kx_ld32(src + ip) == kx_ld32(src + ip - off2)) {
                u32 const ml = kzl_count_wave(src, ip + 4u, ip + 4u - off2, iend, lane) + 4u;
                { u32 const t = off2; off2 = off1; off1 = t; }
                store(0u, 1u, ml);
                ip += ml; anchor = ip;
            }
        }
    }
    saved2 = (saved1 != 0 && off1 != 0) ? saved1 : saved2;
    mm.pad[0] = off1 ? off1 : saved1; mm.pad[1] = off2 ? off2 : saved2;
    mm.nbSeq = nseq; mm.litSize = nlit; mm.lastLL = iend - anchor; mm.longType = longType; mm.longPos = longPos;
    if (nseq > seq_cap) mm.status = 2;
    if (lane == 0) *metaOut = mm;
}

// One wave per slice: clear the slice's tables, then parse and frame step alternate until the frame is closed.  Slices this path does not
// take (k_zstd_lazy_big_init left their blockSize 0: 128 KiB or less -- the one-block kernels have written their frames --, above 2 MiB:
// refused) are passed over.
// MODES: a.e.stream may be any KXF_* mode -- streams (every length from 1 byte on: the unknown-size parameters) and the reference driver's
// staged frames (input taken in chunks of 128 KiB: kx_frame_window_step).  Without it: KXF_ONE_SHOT, the kernel of the one-shot batch call.
template <bool MODES = false>
KX_DEV void zstd_lazy_big_body(const KLazyBigArgs& a)
{
    KX_SHARED KEntropyLds lds;
    KX_SHARED KLazyBigLds l2;
    int const lane = kx_lane();
    for (u32 it = kx_block(); it < a.e.n_slices; it += kx_nblocks()) {
        u32 const slice = kx_xcd_chunk(it, a.e.n_slices);
        if (a.e.fstate[slice].blockSize == 0) continue;                      // (uniform)
        u32 const n = a.e.in_len[slice];
        KLazyBigPar const P = MODES ? kx_lazy_big_params_mode(a.level, n, a.e.stream) : kx_lazy_big_params_one_shot(a.level, n);
        if (P.strat == 0) continue;                                          // (cannot happen: the init kernel applies the same rule)
        const u8* const src = a.e.src + a.e.in_off[slice];
        u8* const slot = a.tables + (u64)slice * a.slot_bytes;
        u32* const hashTable = (u32*)slot; u8* const tagTable = slot + ((size_t)4 << P.H);
        {
            // both tables start empty (a batch before this one, at whatever level, has left its entries): 5 << H bytes, 16 per lane and step
            size_t const bytes = (size_t)5 << P.H;
            for (size_t o = (size_t)lane * 16u; o < bytes; o += 1024u) kx_st128(slot + o, 0ull, 0ull);
        }
        kx_sync();
        KLazyBigState st; st.ntu = 0;
        KLazyFrame lz; lz.strat = P.strat; lz.windowLog = P.W; lz.prev = a.prev + slice; lz.split = l2.split;
        KSeq* const seqs = a.seqs_w + (size_t)slice * a.e.seq_cap;
        for (u32 guard = 0; guard < KX_LAZY_BIG_MAX / 8192u + 64u; guard++) {
            KFrameState const fs = a.e.fstate[slice];
            if (fs.blockSize == 0) break;
            if (fs.blockSize >= 7u) kzlb_parse_block(src, fs.ipos, fs.blockSize, hashTable, tagTable, P, l2, st, fs.rep[0], fs.rep[1], seqs, a.e.seq_cap, a.meta_w + slice, lane);
            kx_sync();
            zstd_frame_block<true, MODES>(a.e, lds, slice, lane, &lz);
            kx_sync();
        }
    }
}

// k_zstd_frame_init's sibling for a batch at levels 5 .. 10 on a context for slices above 128 KiB: the frame state of the slices this
// path takes; blockSize 0 for the others; a slice above 2 MiB is refused (out_len 0, the status bit).
// mode: KFrameArgs.stream.  Streams and staged frames take their input in chunks of 128 KiB (chunkEnd, as k_zstd_frame_init sets it for
// levels <= 4); a stream is taken at every length -- an empty one is its header and an empty last block, which the caller writes.
KX_DEV void zstd_lazy_big_init_slice(u32 len, KFrameState& s, KSeqPrev& pv, bool& refused, u32 mode = KXF_ONE_SHOT)
{
    s.ipos = 0; s.opos = 0; s.blockSize = 0; s.first = 1; s.rep[0] = 1; s.rep[1] = 4; s.rep[2] = 8; s.hufValid = 0; s.hufSel = 0; s.savings = 0;
    s.lowLimit = 2; s.dictLimit = 2; s.bufPos = 0; s.extBase = 0; s.wflags = 0;
    s.chunkEnd = (mode != KXF_ONE_SHOT && len > KX_BLOCK_MAX) ? KX_BLOCK_MAX : len;
    pv.mode[0] = 0; pv.mode[1] = 0; pv.mode[2] = 0;
    refused = len > KX_LAZY_BIG_MAX;
    bool const streaming = mode == KXF_STREAM || mode == KXF_STREAM_EMPTY_END;
    if (len > KX_BLOCK_MAX && !refused) s.blockSize = KX_BLOCK_MAX;
    else if (streaming && !refused) s.blockSize = len;
}
// the empty stream at levels 5 .. 10: no content size, the level's window descriptor, an empty last block (9 bytes)
KX_DEV u32 zstd_lazy_big_empty_stream(u8* d, u32 level, u32 fflags = 0)
{
    kx_st32(d, 0xFD2FB528u); d[4] = (u8)((fflags & KXH_CHECKSUM) ? 1u << 2 : 0u); d[5] = (u8)((kx_lazy_big_params_stream(level, 0).W - 10u) << 3); d[6] = 1; d[7] = 0; d[8] = 0;
    return 9u;
}
