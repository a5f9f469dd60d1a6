// zstd_match_fast_dict.h -- the LZ stage of zstd levels 1, 2 and the negative levels (strategy "fast": one hash table) when the
// context holds a dictionary (reference: ZstdCompressor(level, dictionary) -> ZSTD_CCtx_setParameter + ZSTD_CCtx_loadDictionary,
// jni/Wrapper.cpp:29-56, then the one-shot ZSTD_compressStream2 at :112).  Slices of one block (at most 128 KiB).
//
// libzstd 1.5.7 turns the dictionary into a CDict (one table sized for the dictionary, built once: here by the host,
// zstd_cdict_host.h cdict_fill_fast) and then parses every input with one of two variants of the fast parser:
//   * input <= 8 KiB (attachDictSizeCutoffs[ZSTD_fast]): the CDict stays attached; its tagged table is consulted beside the
//     working table (ZSTD_compressBlock_fast_dictMatchState_generic: one position per step, the repcode tried at the next byte,
//     the step growing by one after every 256 bytes without a match);
//   * input  > 8 KiB: the CDict's table is copied into the working table first and the dictionary becomes an older segment
//     (ZSTD_compressBlock_fast_extDict_generic: the loop of zstd_match_fast.h's zstd_match_fast_ext_body -- pairs of positions, the
//     repcode tried one step ahead, the pair distance growing after 128 bytes without a match).  Here the copy is never made: a
//     working-table entry that is not from this slice falls back to the shared CDict table with its tag stripped, which is the
//     same thing and keeps the dictionary's table read-only, shared by all slices and cache resident (at most 128 KiB, read
//     through L2: a copy in LDS would cost a workgroup a fill per launch and most of a compute unit's LDS for a parser whose
//     step is one dependent load).
// Negative levels: row 0 of libzstd's tables with targetLength = -level, which is the distance between the searched positions.
// Index space, the virtual string dictionary ++ input and the team conventions are zstd_match_dict.h's: dictionary = indices
// [2, 2 + D), input from 2 + D; lane 0 of a team walks, the team extends matches; all cross-lane primitives are called from
// wave-uniform control flow.
#pragma once
#include "zstd_match_dict.h"

struct KFastDictArgs {
    KMatchArgs m;                     // slices, sequences, meta, per-team working table + epochs, work counter
    const u8* dict; u32 dict_size;    // D: 8 .. KX_MAX_DICT (a formatted dictionary's content part)
    u32 rep0 = 1, rep1 = 4;           // the repeat offsets a frame starts with (a formatted dictionary brings its own)
    const u32* dictH;                 // CDict table: entries index << 8 | tag, 1 << dHashLog of them
    u32 dWindowLog, dHashLog, dMinMatch;      // the CDict's parameters (ZSTD_getCParams for the dictionary alone at the level's row)
    u32 step = 1;                     // targetLength + !targetLength: 1 at levels 1 and 2, -level at a negative level
};
#define KX_FAST_ATTACH_MAX (8u * 1024u)        /* attachDictSizeCutoffs[ZSTD_fast] */

// a working-table slot as the copied-table variant sees it: this slice's entry, else what the copy would have put there
KX_DEV u32 kfd_slot(const u32* H, const u32* dictH, u32 h, u32 tag)
{
    u32 const e = H[h];
    return ((e & KX_TAG_MASK) == tag) ? (e & KX_IDX_MASK) : (dictH[h] >> 8);
}

enum { KFD_IDLE = 0, KFD_DMS = 1, KFD_START = 2, KFD_PAIR = 3, KFD_REPLOOP = 4, KFD_MATCH = 5, KFD_CLEANUP = 6, KFD_DONE = 7 };

template <int G>
KX_DEV void zstd_match_fast_dict_body(const KFastDictArgs& d)
{
    const KMatchArgs& a = d.m;
    auto const [lane, k, tbase, tmask, team] = kx_team<G>(0);
    u32* const H = kx_team_tables(a, team);
    int const D = (int)d.dict_size;
    u32 const P = 2u + (u32)D;                            // index of the input's first byte (prefixStartIndex; dictStartIndex is 2)

    int state = KFD_IDLE;
    KV v; v.dict = d.dict; v.D = D; v.src = a.src; v.n = 0;
    int n = 0, ilimit = 0; u32 slice = 0; bool attach = false;
    int ip0 = 0, ip1 = 0, anchor = 0; u32 off1 = 1, off2 = 4; u32 tag = 0, hlog = 13, mls = 5;
    int step = 1, gap = 1, nextStep = 0; u32 hash0 = 0, hash1 = 0, idx = 0;        // (copied-table variant) gap = distance from the pair to the next one
    u32 guard = 0, status = 0;
    KSeqSink sink = { a.seqs };
    // pending match (virtual positions); m_cur0: the searched position whose successor is inserted behind the match, -1: none;
    // m_ip1 / m_hash1: the pair's other position (copied-table variant), inserted when the match has not swallowed it
    int m_start = 0, m_mv = 0, m_low = 0, m_cur0 = 0, m_ip1 = -1; u32 m_len0 = 0, m_off = 0, m_hash1 = 0; bool m_back = false;

#define KFD_SLOT(h_) kfd_slot(H, d.dictH, h_, tag)

    for (;;) {
        // ================= next slice ==================================
        if (kx_any(state == KFD_IDLE)) {
            KClaim const cl = kx_team_claim<true>(state == KFD_IDLE && k == 0, tbase, a.counter, a.n_slices, a.team_epoch + team);
            u32 const s = cl.s;
            if (state == KFD_IDLE) {
                if (s >= a.n_slices) state = KFD_DONE;
                else {
                    slice = s;
                    v.src = a.src + a.in_off[s]; n = (int)a.in_len[s]; v.n = n;
                    sink.reset(a.seqs + (size_t)s * a.seq_cap);
                    attach = n <= (int)KX_FAST_ATTACH_MAX;
                    hlog = d.dHashLog; mls = d.dMinMatch;
                    if (attach) {
                        // working table resized for the input alone (ZSTD_adjustCParams_internal, attach mode)
                        u32 const srcLog = (n < 64) ? 6u : kx_hb32((u32)n - 1u) + 1u;
                        u32 const W = d.dWindowLog < srcLog ? d.dWindowLog : srcLog;
                        if (hlog > W + 1) hlog = W + 1;
                    }
                    guard = 0; status = 0;
                    tag = kx_team_tag<G>(k, cl.ep, H, KX_TBL_ENTRIES);
                    anchor = 0; ip0 = 0; ilimit = n - 8; off1 = d.rep0; off2 = d.rep1;
                    if (attach) {
                        step = (int)d.step; ip1 = step; nextStep = 256;
                        state = (n < 8 || ip1 > ilimit) ? KFD_CLEANUP : KFD_DMS;
                    } else {
                        // repeat offsets that reach the dictionary's first byte or beyond are set aside for the block (maxRep = D)
                        if (off2 >= (u32)D) off2 = 0;
                        if (off1 >= (u32)D) off1 = 0;
                        state = KFD_START;
                    }
                }
            }
        }
        if (kx_all(state == KFD_DONE)) break;

        // ================= attached CDict: one search position (lane 0 of the team decides) ==========
        if (kx_any(state == KFD_DMS)) {
            bool const srch = state == KFD_DMS;
            u32 kind = 0;                // 0 none, 1 rep at ip0 + 1, 2 dictionary candidate at ip0, 3 candidate of this slice at ip0
            u32 mIdx = 0;                // index of the match start
            if (srch && k == 0) {
                u64 const w0 = kv_ld64(v, D + ip0);
                u32 const h0 = kx_hash_short_any(w0, hlog, mls), hd = kx_hash_short_any(w0, d.dHashLog + 8, mls);
                u32 const curr = P + (u32)ip0;
                // both tables' slots are requested together, then the candidates' bytes; the decisions keep libzstd's order
                u32 const e = H[h0], x = d.dictH[hd >> 8];
                u32 const mi = ((e & KX_TAG_MASK) == tag) ? (e & KX_IDX_MASK) : 0u;
                bool const dTag = (x & 0xFFu) == (hd & 0xFFu); u32 const dIdx = x >> 8;
                u32 const repIndex = curr + 1u - off1;
                // ZSTD_index_overlap_check + the lower bound (libzstd only asserts it, it always holds)
                bool const repOk = ((u32)((P - 1u) - repIndex) >= 3u) && off1 <= curr - 1u;
                bool const dOk = dTag && dIdx > 2u, mOk = mi >= P;
                u32 const cR = kv_ld32(v, repOk ? (int)repIndex - 2 : 0);
                u32 const cD = kv_ld32(v, dOk ? (int)dIdx - 2 : 0);
                u32 const cM = kv_ld32(v, mOk ? (int)mi - 2 : 0);
                H[h0] = tag | curr;
                if (repOk && cR == (u32)(w0 >> 8)) { kind = 1; mIdx = repIndex; }
                else if (dOk && cD == (u32)w0 && mi <= P) { kind = 2; mIdx = dIdx; }      // (the dictionary's candidate only where this slice has none)
                else if (mOk && cM == (u32)w0) { kind = 3; mIdx = mi; }
            }
            kind = kx_shfl(kind, tbase); mIdx = kx_shfl(mIdx, tbase);
            if (srch) {
                guard++;
                if (kind == 0) {
                    if (ip1 >= nextStep) { step++; nextStep += 256; }
                    ip0 = ip1; ip1 += step;
                    if (ip1 > ilimit) state = KFD_CLEANUP;
                    if (guard > 2u * (u32)n + 64u) { status = 1; state = KFD_CLEANUP; }
                } else {
                    m_cur0 = ip0; m_ip1 = -1;
                    m_mv = (int)mIdx - 2;
                    m_low = (kind == 3) ? D : 0;
                    if (kind == 1) { m_start = ip0 + 1; m_off = 0; m_back = false; }
                    else { m_start = ip0; m_off = (P + (u32)ip0) - mIdx; m_back = true; }
                    m_len0 = 4;
                    state = KFD_MATCH;
                }
            }
        }

        // ================= copied table: "_start", a new run of pairs =====================
        if (kx_any(state == KFD_START)) {
            if (state == KFD_START) {
                step = (int)d.step + 1; gap = step; nextStep = ip0 + 128;
                if (n < 8 || ip0 + step + 1 >= ilimit) state = KFD_CLEANUP;             // (ip3 = ip0 + step + 1)
                else {
                    u32 h0 = 0, h1 = 0, e = 0;
                    if (k == 0) {
                        h0 = kx_hash_short_any(kv_ld64(v, D + ip0), hlog, mls);
                        h1 = kx_hash_short_any(kv_ld64(v, D + ip0 + 1), hlog, mls);
                        e = KFD_SLOT(h0);
                    }
                    hash0 = h0; hash1 = h1; idx = e;             // lane 0's copies are the ones used
                    state = KFD_PAIR;
                }
            }
        }

        // ================= copied table: one pair (lane 0 of the team walks it, in libzstd's order) ===========
        if (kx_any(state == KFD_PAIR)) {
            bool const pr = state == KFD_PAIR;
            u32 kind = 0;            // 0 no hit, 1 repcode at ip2, 2 candidate of the pair's first position, 3 of its second
            int n_ip0 = ip0, n_step = step, n_gap = gap, n_next = nextStep, n_cur = 0, n_ip1 = 0; u32 n_idx = 0, n_h0 = hash0, n_h1 = hash1, n_rep = 0;
            if (pr && k == 0) {
                int const i1p = ip0 + 1, ip2 = ip0 + gap, ip3 = ip2 + 1;
                u64 const w2 = kv_ld64(v, D + ip2);
                u32 const s0 = kv_ld32(v, D + ip0), s1 = kv_ld32(v, D + i1p);
                u32 const repIndex = P + (u32)ip2 - off1;
                bool const repOk = ((u32)(P - repIndex) >= 4u) && off1 > 0;
                u32 const rval = repOk ? kv_ld32(v, (int)repIndex - 2) : ((u32)w2 ^ 1u);
                u32 const c0 = idx >= 2u ? kv_ld32(v, (int)idx - 2) : (s0 ^ 1u);
                n_cur = ip0; n_ip1 = i1p;
                H[hash0] = tag | (P + (u32)ip0);
                if ((u32)w2 == rval) { kind = 1; n_ip0 = ip2; n_rep = repIndex; }
                else if (c0 == s0) { kind = 2; n_idx = idx; }
                else {
                    u32 const i1 = KFD_SLOT(hash1);
                    u32 const h2 = kx_hash_short_any(w2, hlog, mls);
                    n_cur = i1p; n_ip1 = ip2;
                    H[hash1] = tag | (P + (u32)i1p);
                    u32 const c1 = i1 >= 2u ? kv_ld32(v, (int)i1 - 2) : (s1 ^ 1u);
                    if (c1 == s1) { kind = 3; n_ip0 = i1p; n_idx = i1; n_h0 = hash1; n_h1 = h2; }
                    else {
                        u32 const i2 = KFD_SLOT(h2);
                        u32 const h3 = kx_hash_short_any(kv_ld64(v, D + ip3), hlog, mls);
                        n_idx = i2; n_h0 = h2; n_h1 = h3;
                        n_ip0 = ip2;                              // the next pair: (ip2, ip3); its successor lies `step` behind it
                        n_gap = step;
                        if (ip2 + step >= nextStep) { n_step = step + 1; n_next = nextStep + 128; }
                    }
                }
            }
            kind = kx_shfl(kind, tbase); n_ip0 = (int)kx_shfl((u32)n_ip0, tbase); n_step = (int)kx_shfl((u32)n_step, tbase);
            n_next = (int)kx_shfl((u32)n_next, tbase); n_cur = (int)kx_shfl((u32)n_cur, tbase); n_idx = kx_shfl(n_idx, tbase);
            n_gap = (int)kx_shfl((u32)n_gap, tbase);
            n_ip1 = (int)kx_shfl((u32)n_ip1, tbase); n_h0 = kx_shfl(n_h0, tbase); n_h1 = kx_shfl(n_h1, tbase); n_rep = kx_shfl(n_rep, tbase);
            if (pr) {
                guard++;
                if (kind == 0) {
                    ip0 = n_ip0; idx = n_idx; hash0 = n_h0; hash1 = n_h1; gap = n_gap; step = n_step; nextStep = n_next;
                    if (!(ip0 + 1 + gap < ilimit)) state = KFD_CLEANUP;               // while (ip3 < ilimit), ip3 = ip1 + step
                    if (guard > 2u * (u32)n + 64u) { status = 1; state = KFD_CLEANUP; }
                } else {
                    m_cur0 = n_cur; m_ip1 = n_ip1; m_hash1 = kind == 3 ? n_h1 : hash1;
                    if (kind == 1) {
                        int const mp = (int)n_rep - 2;
                        bool const b1 = kv_byte(v, D + n_ip0 - 1) == kv_byte(v, mp - 1);      // (mp >= 1: offsets that reach index 2 were set aside)
                        m_start = n_ip0 - (b1 ? 1 : 0); m_mv = mp - (b1 ? 1 : 0); m_len0 = 4u + (b1 ? 1u : 0u); m_back = false; m_off = 0; m_low = 0;
                    } else {
                        m_start = n_ip0; m_mv = (int)n_idx - 2; m_len0 = 4; m_back = true;
                        m_off = (P + (u32)m_start) - n_idx;
                        m_low = n_idx < P ? 0 : D;                   // lowMatchPtr: the start of the match's own segment
                    }
                    state = KFD_MATCH;
                }
            }
        }

        // ================= immediate repcode (both variants) =================================
        if (kx_any(state == KFD_REPLOOP)) {
            bool const inrep = state == KFD_REPLOOP;
            bool hit = false; int rv = 0;
            if (inrep && ip0 <= ilimit) {
                u32 const current2 = P + (u32)ip0;
                u32 const repIndex2 = current2 - off2;
                // (attached: repcodes are never 0 and libzstd only asserts the lower bound)
                bool const ok = ((u32)((P - 1u) - repIndex2) >= 3u) && off2 > 0 && off2 <= current2 - 2u;
                rv = (int)repIndex2 - 2;
                if (ok) hit = kv_ld32(v, rv) == kv_ld32(v, D + ip0);
            }
            if (inrep) {
                if (hit) {
                    if (k == 0) H[kx_hash_short_any(kv_ld64(v, D + ip0), hlog, mls)] = tag | (P + (u32)ip0);
                    u32 const t = off2; off2 = off1; off1 = t;
                    m_start = ip0; m_mv = rv; m_low = 0; m_len0 = 4; m_back = false; m_off = 0; m_cur0 = -1; m_ip1 = -1;
                    state = KFD_MATCH;
                } else if (attach) {
                    step = (int)d.step; ip1 = ip0 + step; nextStep = ip0 + 256;
                    state = (ip1 > ilimit) ? KFD_CLEANUP : KFD_DMS;
                } else state = KFD_START;
            }
        }

        // ================= take the match ====================================
        if (kx_any(state == KFD_MATCH)) {
            bool const mt = state == KFD_MATCH;
            u32 lenA = kv_team_extend<G>(mt, v, D + n, D + m_start, m_mv, m_len0, k, tbase, tmask);
            int const mb = (m_start - anchor < m_mv - m_low) ? m_start - anchor : m_mv - m_low;
            u32 const back = kv_team_backward<G>(mt && m_back, v, D + m_start, m_mv, mb, k, tbase, tmask);
            if (mt) {
                u32 offBase = 1;
                if (m_back) { m_start -= (int)back; lenA += back; off2 = off1; off1 = m_off; offBase = m_off + 3; }
                int const ll = m_start - anchor;
                sink.push<G>(k, offBase, ll, lenA - 3);
                ip0 = m_start + (int)lenA; anchor = ip0;
                if (m_cur0 >= 0 && k == 0) {
                    // the pair's other position, if the match has not swallowed it; then the fill: the searched position + 2 and ip0 - 2
                    if (m_ip1 >= 0 && m_ip1 < ip0) H[m_hash1] = tag | (P + (u32)m_ip1);
                    if (ip0 <= ilimit) {
                        H[kx_hash_short_any(kv_ld64(v, D + m_cur0 + 2), hlog, mls)] = tag | (P + (u32)m_cur0 + 2u);
                        H[kx_hash_short_any(kv_ld64(v, D + ip0 - 2), hlog, mls)] = tag | (P + (u32)ip0 - 2u);
                    }
                }
                if (++guard > 2u * (u32)n + 64u) { status = 2; state = KFD_CLEANUP; }
                else if (ip0 <= ilimit) state = KFD_REPLOOP;
                else if (attach) state = KFD_CLEANUP;                  // (ip1 = ip0 + step lies beyond ilimit too)
                else state = KFD_START;
            }
        }

        // ================= finish the slice ==================================
        if (kx_any(state == KFD_CLEANUP)) {
            if (state == KFD_CLEANUP) {
                sink.flush<G>(k);
                if (k == 0) {
                    KSliceMeta mm = sink.meta((u32)(n - anchor), status);
                    a.meta[slice] = mm;
                }
                state = KFD_IDLE;
            }
        }
    }
#undef KFD_SLOT
}
