// zstd_launch.h -- the host side's description of a zstd compress launch: workspace capacities, a view of a batch over a workspace,
// and the argument structs built from it.  The library (kmp_batch.hip) and the CPU emulator harness (tests/emu/emu_zstd.cpp) both
// launch through this file, so nothing here needs the HIP runtime: plain structs and host functions over the kernels' own headers.
#pragma once
#include "zstd_entropy.h"           // (brings zstd_match.h, zstd_match_ext.h, zstd_match_fast.h)
#include "zstd_match_dict.h"
#include "zstd_match_fast_dict.h"
#include "zstd_lazy.h"
#include "zstd_lazy_big.h"
#include "zstd_seekable.h"          // (the XXH64 body of a batch whose frames carry checksums)
#include <type_traits>

// The parsers are templates on their team width (lanes per slice): f(std::integral_constant<int, G>()) for G = 2 .. 64 (else 64)
template <class F> static void by_team_width(int G, F const& f)
{
    switch (G) {
    case 2:  f(std::integral_constant<int, 2>()); break;
    case 4:  f(std::integral_constant<int, 4>()); break;
    case 8:  f(std::integral_constant<int, 8>()); break;
    case 16: f(std::integral_constant<int, 16>()); break;
    case 32: f(std::integral_constant<int, 32>()); break;
    default: f(std::integral_constant<int, 64>()); break;
    }
}

// What a slice's part of the workspace holds, from the largest block parsed there: sequences, literals (+ the wide copies' overrun),
// words of Huffman stream staging; pos_cap: the positions of a slice in the workspace of levels 5 .. 10
struct KWorkCaps { u32 seq_cap, lit_cap, scratch_words, pos_cap; };
inline KWorkCaps kx_work_caps(u32 block_cap)
{
    KWorkCaps w;
    w.seq_cap = (block_cap / 4 + 8 + 15) & ~15u; w.lit_cap = block_cap + 64; w.scratch_words = block_cap / 4 + 64; w.pos_cap = (block_cap + 63u) & ~63u;
    return w;
}

// A batch over a workspace: the caller's arrays (in_len: the lengths the kernels may trust) and the per-slice workspace arrays.
struct KBatchView {
    const u8* src; const u64* in_off; const u32* in_len; u8* dst; const u64* out_off; u32* out_len; u32 n;
    KSeq* seqs; u8* lits; KSliceMeta* meta; u32* scratch; KWorkCaps cap;
    // the frame flags the batch was queued with (KXH_*: every argument struct below that writes frames takes them from here) and, with
    // KXH_CHECKSUM, one word per slice that the batch's XXH64 pass fills (kx_frame_xxh_args) before any frame is closed
    u32 fflags = 0; u32* cks = nullptr;
    // the slices [first, first + count): the one place where the per-slice strides are applied (src and dst are addressed by the offsets)
    KBatchView sub(u32 first, u32 count) const
    {
        KBatchView v = *this;
        v.in_off += first; v.in_len += first; v.out_off += first; v.out_len += first; v.n = count;
        v.seqs += (size_t)first * cap.seq_cap; v.lits += (size_t)first * cap.lit_cap; v.meta += first; v.scratch += (size_t)first * cap.scratch_words;
        if (v.cks) v.cks += first;
        return v;
    }
};

// The team tables a one-block parse runs over: one piece, or the four pieces of a spread set (tseg, tseg_n == 4); level4: that level's
// double-fast row, whose tables are larger
struct KTeamTables { u32* tables; u32* epochs; u32* const* tseg; u32 tseg_n; bool level4; };
inline KTeamTables kx_one_piece(u32* tables, u32* epochs, bool level4 = false) { KTeamTables t = { tables, epochs, nullptr, 1, level4 }; return t; }

// counter: the launch's work queue head; block_base: KMatchArgs.block_base
inline KMatchArgs kx_match_args(KBatchView const& v, KTeamTables const& t, u32* counter, u32 flags, u32 block_base = 0)
{
    KMatchArgs m;
    m.src = v.src; m.in_off = v.in_off; m.in_len = v.in_len; m.n_slices = v.n;
    m.seqs = v.seqs; m.seq_cap = v.cap.seq_cap; m.lits = v.lits; m.lit_cap = v.cap.lit_cap; m.meta = v.meta;
    m.tables = t.tables; m.team_epoch = t.epochs; m.tseg_n = t.tseg_n; for (int i = 0; i < 4; i++) m.tseg[i] = t.tseg ? t.tseg[i] : nullptr;
    m.counter = counter; m.flags = flags; m.fstate = nullptr; m.big_tables = nullptr; m.block_base = block_base;
    if (t.level4) { m.tbl_stride = KX_TBL4_ENTRIES; m.tbl_long = KX_TBL4_LONG; m.level = 4; }
    return m;
}
// ... in block mode (frames of several blocks): the slices' states and their own tables
inline KMatchArgs kx_match_args_blk(KBatchView const& v, KTeamTables const& t, u32* counter, bool streaming, bool wide, const KFrameState* fstate, u32* big_tables, bool level4)
{
    KMatchArgs m = kx_match_args(v, t, counter, KXM_NT_STORES | (streaming ? KXM_STREAM_PARAMS : 0u) | (wide ? KXM_WIDE : 0u));
    m.fstate = fstate; m.big_tables = big_tables;
    if (level4) { m.level = 4; m.big_stride = KX_BIG4_ENTRIES; m.big_long = KX_BIG4_LONG; }
    return m;
}
// levels 1, 2 and the negative ones (strategy "fast"); negative: row 0 of libzstd's table, a step of 1 - level
inline KFastArgs kx_fast_args(KBatchView const& v, KTeamTables const& t, u32* counter, int level)
{
    KFastArgs g;
    g.m = kx_match_args(v, t, counter, KXM_NT_STORES | KXM_NO_LITS);
    g.level = level < 0 ? 0u : (u32)level; g.step0 = level < 0 ? (u32)(1 - level) : 2u;
    return g;
}
// the parse against a dictionary's content (CDict tables L / S with the parameters W, H, C, M); rep: the repeat offsets a frame starts with
inline KDictArgs kx_dict_args(KBatchView const& v, KTeamTables const& t, u32* counter, const u8* content, u32 content_size,
                              const u32* L, const u32* S, u32 W, u32 H, u32 C, u32 M, u32 rep0, u32 rep1)
{
    KDictArgs g;
    g.m = kx_match_args(v, t, counter, KXM_NT_STORES | KXM_NO_LITS);
    g.dict = content; g.dict_size = content_size; g.dictL = L; g.dictS = S; g.rep0 = rep0; g.rep1 = rep1;
    g.dWindowLog = W; g.dHashLog = H; g.dChainLog = C; g.dMinMatch = M;
    return g;
}
// ... at levels 1, 2 and the negative ones (strategy "fast": one CDict table H with the parameters W, Hlog, M of the level's row)
inline KFastDictArgs kx_fast_dict_args(KBatchView const& v, KTeamTables const& t, u32* counter, const u8* content, u32 content_size,
                                       const u32* H, u32 W, u32 Hlog, u32 M, u32 rep0, u32 rep1, int level)
{
    KFastDictArgs g;
    g.m = kx_match_args(v, t, counter, KXM_NT_STORES | KXM_NO_LITS);
    g.dict = content; g.dict_size = content_size; g.dictH = H; g.rep0 = rep0; g.rep1 = rep1;
    g.dWindowLog = W; g.dHashLog = Hlog; g.dMinMatch = M;
    g.step = level < 0 ? (u32)(-level) : 1u;             // targetLength + !targetLength
    return g;
}
// which CDict a level asks for: 3 (and 0) double-fast, 1, 2, or -1 for every negative level (row 0; the step is no part of the tables)
inline int kx_dict_level_class(int level) { return level < 0 ? -1 : level == 0 ? 3 : level; }
// levels 5 .. 10 (and level 4's slices up to 16 KiB): rec / wr hold pos_cap positions for each of the view's slices
inline KLazyArgs kx_lazy_args(KBatchView const& v, KLazyRec* rec, u32* wr, u32 pos_cap, int level)
{
    KLazyArgs g;
    g.src = v.src; g.in_off = v.in_off; g.in_len = v.in_len; g.n_slices = v.n;
    g.rec = rec; g.wr = wr; g.pos_cap = pos_cap;
    g.seqs = v.seqs; g.seq_cap = v.cap.seq_cap; g.meta = v.meta; g.level = (u32)level;
    return g;
}

// KEntropyArgs.flags: behind the level-3 parser (match_flags: what that launch got), behind the fast parser, behind the lazy levels'
inline u32 kx_entropy_flags_dfast(u32 match_flags, bool level4) { return ((match_flags & KXM_NO_LITS) ? KXE_GATHER_LITS : 0u) | (level4 ? 4u << KXE_LEVEL_SHIFT : 0u); }
inline u32 kx_entropy_flags_fast(bool negative) { return KXE_GATHER_LITS | KXE_STRATEGY_FAST | (negative ? KXE_RAW_LITS : 0u); }
inline u32 kx_entropy_flags_lazy(int level) { return KXE_GATHER_LITS | ((u32)level << KXE_LEVEL_SHIFT); }
// dict_total: the whole dictionary's bytes when the batch was parsed against one (raw or formatted), else 0
inline KEntropyArgs kx_entropy_args(KBatchView const& v, u32 flags, const KDictPrior* prior = nullptr, u32 dict_total = 0)
{
    KEntropyArgs e;
    e.src = v.src; e.in_off = v.in_off; e.in_len = v.in_len; e.n_slices = v.n;
    e.seqs = v.seqs; e.seq_cap = v.cap.seq_cap; e.lits = v.lits; e.lit_cap = v.cap.lit_cap; e.meta = v.meta;
    e.scratch = v.scratch; e.scratch_words = v.cap.scratch_words;
    e.dst = v.dst; e.out_off = v.out_off; e.out_len = v.out_len; e.prior = prior; e.flags = flags;
    e.fflags = v.fflags; e.cks = v.cks; e.dict_total = dict_total;
    return e;
}

// The XXH64 pass of a batch with KXH_CHECKSUM, in front of its first frame writer: zstd_seekable.h's quad-per-piece body over the view's
// slices, the low 32 bits (seed 0) of slice i to v.cks[i].  A quad walks its slice alone, so one slice of 1 GiB takes as long as a
// batch of them: the frames this library writes end at 2 MiB a block chain, where that is a fraction of the parse.
inline KSeekXxhArgs kx_frame_xxh_args(KBatchView const& v)
{
    KSeekXxhArgs x = { v.src, v.in_off, v.in_len, v.n, v.cks, nullptr, nullptr };
    return x;
}
// its grid of four-wave workgroups: a wave takes 16 slices a trip (the shape the seekable container launches the body with)
inline u32 kx_frame_xxh_blocks(u32 n) { u32 const b = (n + 63u) / 64u; return b < 1u ? 1u : b > 8192u ? 8192u : b; }

// Entropy sweeps beside a one-block parse (zstd_compress_dfast): the parse leaves a completion record per slice and counts them
// (KMatchArgs.done / done_count); a sweep is the entropy launch with KXE_SWEEP, which codes the slices that are done and not yet
// coded.  done, coded: one word per slice; count: one word; all zeroed before the parse is launched.
struct KSweepRecords { u32* done; u32* coded; u32* count; };
enum { KX_MAX_SWEEPS = 16 };
inline void kx_match_records(KMatchArgs& m, KSweepRecords const& r) { m.done = r.done; m.done_count = r.count; }
// swept: where the sweep counts the slices it codes, or null
inline KEntropyArgs kx_entropy_sweep_args(KEntropyArgs e, KSweepRecords const& r, u32* swept) { e.flags |= KXE_SWEEP; e.done = r.done; e.coded = r.coded; e.swept = swept; return e; }
// The counts of finished slices at which the K - 1 sweeps beside the parse start: T_j = j n / K, j = 1 .. K - 1, without those that are 0
// and without duplicates (K > n), ascending; every one satisfies 0 < T <= n, so the parse reaches it.  Returns how many (< KX_MAX_SWEEPS).
inline u32 kx_sweep_thresholds(u32 n, u32 K, u32* T)
{
    if (K > KX_MAX_SWEEPS) K = KX_MAX_SWEEPS;
    u32 cnt = 0;
    for (u32 j = 1; j < K; j++) {
        u32 const t = (u32)((u64)j * n / K);
        if (t == 0 || t > n || (cnt && T[cnt - 1] == t)) continue;
        T[cnt++] = t;
    }
    return cnt;
}

// Frames of several blocks.  strategy: 0 level 3 / 4 (double-fast), 1 level 1 and the negative levels (fast; fast_step0 = 1 - level for
// those, else 0), 2 level 2 (fast, but double-fast for 128 KiB < size <= 256 KiB when the size is known).  level -> these three:
struct KBigLevel { u32 strategy, fast_step0; bool level4; };
inline KBigLevel kx_big_level(int level)
{
    KBigLevel b = { (level == 3 || level == 4) ? 0u : level < 0 ? 1u : (u32)level, level < 0 ? (u32)(1 - level) : 0u, level == 4 };
    return b;
}
// a streaming frame's window descriptor byte (0: one-shot frames write their own header)
inline u32 kx_big_window_byte(u32 stream, u32 strategy) { return (stream == KXF_STREAM || stream == KXF_STREAM_EMPTY_END) ? (strategy == 1u ? 0x48u : strategy == 2u ? 0x50u : 0x58u) : 0u; }
// tail_or_chunk: KFrameArgs.tail_direct, or with KXF_REFERENCE its out_chunk (the mode says which it is)
inline KFrameArgs kx_frame_args(KBatchView const& v, KFrameState* fstate, u32* hufct, u32* remaining, u32* status_word, u32 stream, KBigLevel const& b, u32 tail_or_chunk)
{
    KFrameArgs e;
    e.src = v.src; e.in_off = v.in_off; e.in_len = v.in_len; e.n_slices = v.n;
    e.seqs = v.seqs; e.seq_cap = v.cap.seq_cap; e.lits = v.lits; e.lit_cap = v.cap.lit_cap; e.meta = v.meta;
    e.scratch = v.scratch; e.scratch_words = v.cap.scratch_words;
    e.dst = v.dst; e.out_off = v.out_off; e.out_len = v.out_len;
    e.fstate = fstate; e.hufct = hufct; e.remaining = remaining; e.status_word = status_word;
    e.stream = stream; e.strategy = b.strategy ? 1u : 0u; e.level2 = b.strategy == 2u ? 1u : 0u; e.cls = KXC_ALL;
    e.fast_step0 = b.strategy == 1u ? b.fast_step0 : 0u;
    e.tail_direct = stream == KXF_REFERENCE ? 0u : tail_or_chunk; e.out_chunk = stream == KXF_REFERENCE ? tail_or_chunk : 0u;
    e.fflags = v.fflags; e.cks = v.cks;
    return e;
}
// Levels 5 .. 10 over frames of several blocks (zstd_lazy_big.h): the view's slices over table slots of slot_bytes each and their
// previous-table records; hash_log_max: kx_lazy_big_hash_log_max of the largest slice the slots must hold
inline u64 kx_lazy_big_slot_bytes(u32 hash_log_max) { return (u64)5 << hash_log_max; }
// stream: KFrameArgs.stream (KXF_ONE_SHOT: the one-shot batch call; the other modes go through zstd_lazy_big_body<true>); out_chunk: KXF_REFERENCE's
inline KLazyBigArgs kx_lazy_big_args(KBatchView const& v, KFrameState* fstate, u32* hufct, u32* remaining, u32* status_word, u8* tables, u64 slot_bytes, KSeqPrev* prev, int level,
                                     u32 stream = KXF_ONE_SHOT, u32 out_chunk = 0)
{
    KLazyBigArgs g;
    KBigLevel const none = { 0u, 0u, false };
    g.e = kx_frame_args(v, fstate, hufct, remaining, status_word, stream, none, stream == KXF_REFERENCE ? out_chunk : 0u);
    g.level = (u32)level; g.tables = tables; g.slot_bytes = slot_bytes; g.prev = prev; g.seqs_w = v.seqs; g.meta_w = v.meta;
    return g;
}
// the table slot a batch in that mode needs on a context for slices of up to slice_cap bytes
inline u64 kx_lazy_big_slot_bytes_mode(u32 slice_cap, int level, u32 stream)
{
    bool const streaming = stream == KXF_STREAM || stream == KXF_STREAM_EMPTY_END;
    return kx_lazy_big_slot_bytes(streaming ? kx_lazy_big_hash_log_stream(level) : kx_lazy_big_hash_log_max(slice_cap));
}
// the block-chain kernels' arguments (a wave walks a slice's chain of blocks); counters: one work queue head per workgroup
inline KBigArgs kx_big_args(KMatchArgs const& m, KFrameArgs const& e, u32* counters, u32 spw) { KBigArgs g; g.m = m; g.e = e; g.counters = counters; g.spw = spw; return g; }
// Level 2 with the sizes known goes through both kernels: the slices of its double-fast row (KXC_L2_DFAST, zstd_big_body<G>) first, then the
// others (KXC_L2_FAST, zstd_big_body<G, true>).  match_flags: what kx_match_args_blk set
inline void kx_big_set_class(KBigArgs& g, u32 match_flags, u32 cls)
{
    g.e.cls = cls; g.e.strategy = cls == KXC_L2_DFAST ? 0u : 1u;
    g.m.flags = match_flags | (cls << KXM_CLASS_SHIFT) | (cls == KXC_L2_DFAST ? KXM_L2_DFAST : 0u);
}
