// zstd_team.h -- what every team parser of the zstd compress side shares (zstd_match*.h): a wave is split into 64/G
// teams of G lanes, each team owns one slice at a time.  None of this depends on which parse it is:
//
//  * KTeam / kx_team: who this lane is inside its team;
//  * kx_team_claim / kx_team_tag: the next slice from the work queue, the epoch of the team's tables;
//  * KSeqSink: the sequences of a slice on their way to memory in whole 16-byte pieces, and the slice's record.
//
// Plain inline functions and small structs: the parsers keep their state machines and loops and call into this.  Which
// claimed slice a body takes or skips, its literal copy, its runaway guards and its record's padding words stay with
// the body.  All cross-lane primitives are called from wave-uniform control flow.
#pragma once
#include "zstd_common.h"
#include "kx_agent.h"

// ---- the lane inside its team ------------------------------------------
// k: index inside the team; tbase: the wave lane of the team's lane 0; tmask: G ones; team: the team's index in the
// launch, which selects its tables and epoch (block_base: KMatchArgs.block_base, 0 where a launch owns all teams)
template <int G>
struct KTeam { int lane, k, tbase; u64 tmask; u32 team; };

template <int G>
KX_DEV KTeam<G> kx_team(u32 block_base)
{
    KTeam<G> t;
    t.lane = kx_lane();
    t.k = t.lane & (G - 1);
    t.tbase = t.lane - t.k;
    t.tmask = (G == 64) ? ~0ull : ((1ull << G) - 1ull);
    t.team = (kx_block() + block_base) * (64 / G) + (u32)(t.lane / G);
    return t;
}

// ---- the slice claim ----------------------------------------------------
// The next slice index of the work queue for every team whose lane 0 says `claim` (idle and k == 0), broadcast to the
// team; a value >= n_slices says the queue is empty.  EPOCH (one-block bodies, tables per team): the team's epoch is
// stepped for a slice that exists; ep comes back 0 when it wrapped ("clear the tables, restart at 1": kx_team_tag).
struct KClaim { u32 s, ep; };

template <bool EPOCH>
KX_DEV KClaim kx_team_claim(bool claim, int tbase, u32* counter, u32 n_slices, u32* epoch)
{
    KClaim c; c.s = 0; c.ep = 0;
    if (claim) {
        c.s = kx_atomic_add(counter, 1u);
        if (EPOCH && c.s < n_slices) {
            u32 ep = *epoch + 1;
            if (ep > KX_EPOCH_MAX) ep = 0;
            *epoch = ep ? ep : 1u;
            c.ep = ep;
        }
    }
    c.s = kx_shfl(c.s, tbase);
    if (EPOCH) c.ep = kx_shfl(c.ep, tbase);
    return c;
}

// The tag of this slice's table entries; a wrapped epoch first clears the team's `entries` words.
template <int G>
KX_DEV u32 kx_team_tag(int k, u32 ep, u32* tbl, u32 entries)
{
    if (ep == 0) {
        for (u32 i = (u32)k; i < entries; i += G) tbl[i] = 0;
        ep = 1;
    }
    return ep << KX_TAG_SHIFT;
}

// ---- the sequence sink --------------------------------------------------
// Sequences wait in registers (two per lane) until the team can store whole 16-byte pieces of a line; uniform across
// the team's lanes except sq0 / sq1.
// wt: the stores go through the L2 at once (kx_st64_agent), for a launch that reads the slice while this one still runs (the
// parse's completion records, zstd_match.h); uniform across the wave
struct KSeqSink {
    KSeq* seqs; u64 sq0, sq1; u32 nseq, nlit, longType, longPos; bool wt = false;

    KX_MEMBER void reset(KSeq* s) { seqs = s; nseq = 0; nlit = 0; longType = 0; longPos = 0; }

    template <int G>
    KX_MEMBER void push(int k, u32 offBase, int ll, u32 mlBase)
    {
        u64 const q = (u64)offBase | ((u64)(u16)ll << 32) | ((u64)(u16)mlBase << 48);   // KSeq
        u32 const slot = nseq & (2u * G - 1u);
        if ((u32)k == (slot >> 1)) { if (slot & 1u) sq1 = q; else sq0 = q; }
        if (slot == 2u * G - 1u) {
            KSeq* const p = seqs + (nseq - slot) + 2u * (u32)k;
            if (wt) { kx_st64_agent((u64*)p, sq0); kx_st64_agent((u64*)p + 1, sq1); } else kx_st128(p, sq0, sq1);
        }
        if (ll > 0xFFFF) { longType = 1; longPos = nseq; }
        if (mlBase > 0xFFFF) { longType = 2; longPos = nseq; }
        nseq++; nlit += (u32)ll;
    }

    // the sequences still in registers
    template <int G>
    KX_MEMBER void flush(int k) const
    {
        u32 const cnt = nseq & (2u * G - 1u);
        u64* const sp = (u64*)(seqs + (nseq - cnt));
        if (2u * (u32)k < cnt) { if (wt) kx_st64_agent(sp + 2 * k, sq0); else sp[2 * k] = sq0; }
        if (2u * (u32)k + 1u < cnt) { if (wt) kx_st64_agent(sp + 2 * k + 1, sq1); else sp[2 * k + 1] = sq1; }
    }

    // the slice's record; the padding words are the body's (repcodes of a block, timestamps)
    KX_MEMBER KSliceMeta meta(u32 lastLL, u32 status) const
    {
        KSliceMeta mm;
        mm.nbSeq = nseq; mm.litSize = nlit; mm.lastLL = lastLL;
        mm.longType = longType; mm.longPos = longPos; mm.status = status; mm.pad[0] = 0; mm.pad[1] = 0;
        return mm;
    }
};
