// TEST INFRASTRUCTURE: runs the product kernel bodies on the CPU wave emulator.  Workspace sizes, batch views and the kernels' argument
// structs come from the product's own launch description (zstd_launch.h); what is restated here is the sequence of launches only.
#include "kx_wave.h"
#include "emu_core.h"
#include "zstd_launch.h"
#include <stdlib.h>
#include <vector>

namespace {
bool env_on(const char* name) { return getenv(name) && atoi(getenv(name)) != 0; }
bool team_width_ok(int G) { return G == 2 || G == 4 || G == 8 || G == 16 || G == 32 || G == 64; }
// a context's workspace for n slices of up to block_cap bytes, full of junk no kernel may rely on
struct Work {
    KWorkCaps cap; std::vector<KSeq> seqs; std::vector<u8> lits; std::vector<KSliceMeta> meta; std::vector<u32> scratch;
    Work(u32 n, u32 block_cap) : cap(kx_work_caps(block_cap)), seqs((size_t)n * cap.seq_cap), lits((size_t)n * cap.lit_cap, 0xEE), meta(n), scratch((size_t)n * cap.scratch_words, 0xA5A5A5A5u) {}
    KBatchView view(const u8* src, const u64* in_off, const u32* in_len, u32 n, u8* dst, const u64* out_off, u32* out_len)
    { KBatchView v = { src, in_off, in_len, dst, out_off, out_len, n, seqs.data(), lits.data(), meta.data(), scratch.data(), cap }; return v; }
};
// team tables for a launch of nblocks waves: stale junk with epoch 0 in every entry, every team at start_epoch
struct Teams {
    std::vector<u32> tables, epoch; bool level4;
    Teams(u32 nblocks, int G, u32 start_epoch, bool l4 = false) : tables((size_t)nblocks * (64 / G) * (l4 ? KX_TBL4_ENTRIES : KX_TBL_ENTRIES), 0xDEADBEEFu & 0x0003FFFFu), epoch(nblocks * (64 / G), start_epoch), level4(l4) {}
    KTeamTables get() { return kx_one_piece(tables.data(), epoch.data(), level4); }
};
bool any_status(const KSliceMeta* meta, u32 n) { for (u32 i = 0; i < n; i++) if (meta[i].status) return true; return false; }
// the level-3 parse of a view's slices: zstd_match.h, or the split-phase parser (ring = bytes of a team's window in LDS)
int run_match(KBatchView const& v, KTeamTables const& t, int G, u32 nblocks, u32 flags)
{
    if (!team_width_ok(G)) return -2;
    u32 counter = 0;
    KMatchArgs const a = kx_match_args(v, t, &counter, flags);
    kxemu::failed = 0;
    by_team_width(G, [&](auto w) { kxemu::launch(nblocks, [&]() { zstd_match_body<decltype(w)::value>(a); }); });
    return kxemu::failed ? -1 : 0;
}
}

extern "C" __attribute__((visibility("default")))
int emu_zstd_match(const u8* src, const u64* in_off, const u32* in_len, u32 n, int G, u32 nblocks,
                   KSeq* seqs, u32 seq_cap, u8* lits, u32 lit_cap, KSliceMeta* meta, u32 start_epoch)
{
    if (!team_width_ok(G)) return -2;
    Teams teams(nblocks, G, start_epoch, getenv("KXEMU_LEVEL") && atoi(getenv("KXEMU_LEVEL")) == 4);      // level 4's double-fast row: larger tables
    KBatchView const v = { src, in_off, in_len, nullptr, nullptr, nullptr, n, seqs, lits, meta, nullptr, { seq_cap, lit_cap, 0, 0 } };
    return run_match(v, teams.get(), G, nblocks, getenv("KXEMU_MATCH_FLAGS") ? (u32)atoi(getenv("KXEMU_MATCH_FLAGS")) & KXM_ADAPTIVE : 0u);
}

#include "zstd_match2.h"
static int run_match2(KBatchView const& v, KTeamTables const& t, int G, u32 nblocks, u32 flags)
{
    int const ring = getenv("KXEMU_RING") ? atoi(getenv("KXEMU_RING")) : 256;
    u32 counter = 0;
    KMatchArgs const a = kx_match_args(v, t, &counter, flags);
    kxemu::failed = 0;
    switch (G * 1000 + ring) {
    case 2256:  kxemu::launch(nblocks, [&]() { zstd_match2_body<2, 256>(a); }); break;
    case 4256:  kxemu::launch(nblocks, [&]() { zstd_match2_body<4, 256>(a); }); break;
    case 4512:  kxemu::launch(nblocks, [&]() { zstd_match2_body<4, 512>(a); }); break;
    case 8512:  kxemu::launch(nblocks, [&]() { zstd_match2_body<8, 512>(a); }); break;
    default: return -2;
    }
    return kxemu::failed ? -1 : 0;
}
// The split-phase parser (zstd_match2.h): same interface, same results.
extern "C" __attribute__((visibility("default")))
int emu_zstd_match2(const u8* src, const u64* in_off, const u32* in_len, u32 n, int G, u32 nblocks,
                    KSeq* seqs, u32 seq_cap, u8* lits, u32 lit_cap, KSliceMeta* meta, u32 start_epoch)
{
    if (G != 2 && G != 4 && G != 8) return -2;
    Teams teams(nblocks, G, start_epoch);
    KBatchView const v = { src, in_off, in_len, nullptr, nullptr, nullptr, n, seqs, lits, meta, nullptr, { seq_cap, lit_cap, 0, 0 } };
    return run_match2(v, teams.get(), G, nblocks, 0u);
}

// Full compress pipeline (match kernel + entropy kernel) on the emulator: zstd_compress_dfast's steps.  A batch of two slices or more goes
// through in two chunks over the one workspace, as the product's large batches do; there the entropy launch of the first chunk runs beside
// the parse of the second, here behind it.
extern "C" __attribute__((visibility("default")))
int emu_zstd_compress(const u8* src, const u64* in_off, const u32* in_len, u32 n, int G, u32 nblocks,
                      u8* dst, const u64* out_off, u32* out_len, u32 slice_cap)
{
    if (!team_width_ok(G)) return -2;
    Work w(n, slice_cap);
    KBatchView const v = w.view(src, in_off, in_len, n, dst, out_off, out_len);
    bool const l4 = getenv("KXEMU_LEVEL") && atoi(getenv("KXEMU_LEVEL")) == 4;
    Teams teams(nblocks, G, 7, l4);
    // KXEMU_FUSE=1: k_zstd_l3_fused's body (the entropy stage inside the parse kernel's waves)
    if (env_on("KXEMU_FUSE") && (G == 4 || G == 8)) {
        u32 counter = 0;
        KMatchArgs const a = kx_match_args(v, kx_one_piece(teams.tables.data(), teams.epoch.data()), &counter, 0u);
        KEntropyArgs const e = kx_entropy_args(v, kx_entropy_flags_dfast(a.flags, false));
        kxemu::failed = 0;
        if (G == 4) kxemu::launch(nblocks, [&]() { zstd_l3_fused_body<4>(a, e); });
        else kxemu::launch(nblocks, [&]() { zstd_l3_fused_body<8>(a, e); });
        if (kxemu::failed) return -1;
        return any_status(v.meta, n) ? -3 : 0;
    }
    // KXEMU_MATCH_V2=1: the split-phase parser (zstd_match2.h; it copies no literals, the entropy kernel gathers them)
    bool const v2 = env_on("KXEMU_MATCH_V2");
    u32 const match_flags = (v2 ? KXM_NO_LITS : 0u) | (getenv("KXEMU_MATCH_FLAGS") ? (u32)atoi(getenv("KXEMU_MATCH_FLAGS")) & KXM_ADAPTIVE : 0u);
    u32 const starts[3] = { 0, n >= 2 ? n / 2 : n, n };
    for (u32 ci = 0; ci < 2; ci++) {
        KBatchView const cv = v.sub(starts[ci], starts[ci + 1] - starts[ci]);
        if (cv.n == 0) continue;
        int const r = v2 ? run_match2(cv, teams.get(), G, nblocks, match_flags) : run_match(cv, teams.get(), G, nblocks, match_flags);
        if (r) return r;
    }
    if (any_status(v.meta, n)) return -3;
    kxemu::failed = 0;
    for (u32 ci = 0; ci < 2; ci++) {
        KBatchView const cv = v.sub(starts[ci], starts[ci + 1] - starts[ci]);
        if (cv.n == 0) continue;
        KEntropyArgs const e = kx_entropy_args(cv, kx_entropy_flags_dfast(match_flags, l4));
        kxemu::launch(nblocks, [&]() { zstd_entropy_body(e); });
    }
    return kxemu::failed ? -1 : 0;
}

// Levels 1 and 2 (strategy fast) and the negative ones: fast match kernel + entropy kernel on the emulator.
extern "C" __attribute__((visibility("default")))
int emu_zstd_compress_level(const u8* src, const u64* in_off, const u32* in_len, u32 n, int G, u32 nblocks,
                            u8* dst, const u64* out_off, u32* out_len, u32 slice_cap, int level)
{
    if (!team_width_ok(G)) return -2;
    Work w(n, slice_cap);
    KBatchView const v = w.view(src, in_off, in_len, n, dst, out_off, out_len);
    Teams teams(nblocks, G, 7);
    u32 counter = 0;
    KFastArgs const g = kx_fast_args(v, teams.get(), &counter, level);
    kxemu::failed = 0;
    by_team_width(G, [&](auto tw) { kxemu::launch(nblocks, [&]() { zstd_match_fast_body<decltype(tw)::value>(g); }); });
    if (kxemu::failed) return -1;
    if (any_status(v.meta, n)) return -3;
    KEntropyArgs const e = kx_entropy_args(v, kx_entropy_flags_fast(level < 0));
    kxemu::launch(nblocks, [&]() { zstd_entropy_body(e); });
    return kxemu::failed ? -1 : 0;
}

#include "zstd_cdict_host.h"
// Compress with a dictionary (raw content, or zstd's format): the host code's steps of kmp_zstd_compress_batch_dict, the dictionary
// match kernel + the entropy kernel on the emulator.
extern "C" __attribute__((visibility("default")))
int emu_zstd_compress_dict(const u8* src, const u64* in_off, const u32* in_len, u32 n, int G, u32 nblocks,
                           u8* dst, const u64* out_off, u32* out_len, u32 slice_cap, const u8* dict, u32 dict_size)
{
    if (!team_width_ok(G)) return -2;
    Work w(n, slice_cap);
    KBatchView const v = w.view(src, in_off, in_len, n, dst, out_off, out_len);
    Teams teams(nblocks, G, 7);
    u32 counter = 0, W, C, H, M;
    KDictPrior prior; size_t content_off = 0;
    int const formatted = cdict_parse_formatted(dict, dict_size, &prior, &content_off);
    if (formatted < 0) return -4;
    cdict_params(dict_size, &W, &C, &H, &M);
    dict += content_off; dict_size -= (u32)content_off;
    std::vector<u32> tl, ts;
    cdict_fill(tl, H, ts, C, M, dict, dict_size);
    KDictArgs const g = kx_dict_args(v, teams.get(), &counter, dict, dict_size, tl.data(), ts.data(), W, H, C, M, formatted ? prior.rep[0] : 1u, formatted ? prior.rep[1] : 4u);
    kxemu::failed = 0;
    by_team_width(G, [&](auto tw) { kxemu::launch(nblocks, [&]() { zstd_match_dict_body<decltype(tw)::value>(g); }); });
    if (kxemu::failed) return -1;
    if (any_status(v.meta, n)) return -3;
    KEntropyArgs const e = kx_entropy_args(v, KXE_GATHER_LITS, formatted ? &prior : nullptr);
    if (formatted) kxemu::launch(nblocks, [&]() { zstd_entropy_body<true>(e); });
    else kxemu::launch(nblocks, [&]() { zstd_entropy_body(e); });
    return kxemu::failed ? -1 : 0;
}

// Levels 5 .. 10 (greedy / lazy / lazy2): sort body (workgroups of four waves), parse body, entropy body -- zstd_compress_lazy's steps.
extern "C" __attribute__((visibility("default")))
int emu_zstd_compress_lazy(const u8* src, const u64* in_off, const u32* in_len, u32 n, u32 nblocks,
                           u8* dst, const u64* out_off, u32* out_len, u32 slice_cap, int level)
{
    Work w(n, slice_cap);
    KBatchView const v = w.view(src, in_off, in_len, n, dst, out_off, out_len);
    std::vector<u32> wr((size_t)n * w.cap.pos_cap, 0xCCCCCCCCu); std::vector<KLazyRec> rec((size_t)n * w.cap.pos_cap);
    memset(rec.data(), 0xBB, rec.size() * sizeof(KLazyRec));
    for (u32 i = 0; i < n; i++) { memset(&w.meta[i], 0, sizeof(w.meta[i])); w.meta[i].lastLL = in_len[i]; w.meta[i].status = 3; }      // (level 4: what the double-fast kernel's slices look like to this harness: not served here)
    KLazyArgs const g = kx_lazy_args(v, rec.data(), wr.data(), w.cap.pos_cap, level);
    kxemu::failed = 0;
    kxemu::launch_block(nblocks, 4, [&]() { zstd_lazy_sort_body(g); });
    if (kxemu::failed) return -1;
    if (slice_cap <= 65536u) kxemu::launch(nblocks, [&]() { zstd_lazy_body<2048>(g); }); else kxemu::launch(nblocks, [&]() { zstd_lazy_body<4096>(g); });
    if (kxemu::failed) return -2;
    for (u32 i = 0; i < n; i++) if (w.meta[i].status == 2) return -3;
    KEntropyArgs const e = kx_entropy_args(v, kx_entropy_flags_lazy(level));
    kxemu::launch(nblocks, [&]() { zstd_entropy_body(e); });
    if (kxemu::failed) return -4;
    for (u32 i = 0; i < n; i++) if (w.meta[i].status == 3) out_len[i] = 0;          // (k_len_guard_finish: another strategy at this size)
    return 0;
}

// Frames of several blocks (slices above 128 KiB): zstd_compress_big's steps (kmp_batch.hip) on the emulator.
extern "C" __attribute__((visibility("default")))
int emu_zstd_compress_big_ex2(const u8* src, const u64* in_off, const u32* in_len, u32 n, int G, u32 nblocks,
                              u8* dst, const u64* out_off, u32* out_len, u32* rounds_out, u32 stream_and_strategy, u32 tail_or_chunk, u32 wide);
extern "C" __attribute__((visibility("default")))
int emu_zstd_compress_big_ex(const u8* src, const u64* in_off, const u32* in_len, u32 n, int G, u32 nblocks,
                             u8* dst, const u64* out_off, u32* out_len, u32* rounds_out, u32 stream_and_strategy)
{ return emu_zstd_compress_big_ex2(src, in_off, in_len, n, G, nblocks, dst, out_off, out_len, rounds_out, stream_and_strategy, 0, 0); }
extern "C" __attribute__((visibility("default")))
int emu_zstd_compress_big(const u8* src, const u64* in_off, const u32* in_len, u32 n, int G, u32 nblocks,
                          u8* dst, const u64* out_off, u32* out_len, u32* rounds_out)
{ return emu_zstd_compress_big_ex(src, in_off, in_len, n, G, nblocks, dst, out_off, out_len, rounds_out, 0); }
// stream (low byte): KFrameArgs.stream; the next byte: zstd_compress_big's strategy (1: level 1, 2: level 2), or 4: level 4's double-fast rows
// (the level-3 kernels, larger tables); bits 16 ..: a negative level's step (1 - level), with strategy 1.  tail_or_chunk: tail_direct of a
// stream, out_chunk of the one-shot driver (KXF_REFERENCE); wide: table entries without check bits (what contexts for slices of 4 MiB and more use)
extern "C" __attribute__((visibility("default")))
int emu_zstd_compress_big_ex2(const u8* src, const u64* in_off, const u32* in_len, u32 n, int G, u32 nblocks,
                              u8* dst, const u64* out_off, u32* out_len, u32* rounds_out, u32 stream_and_strategy, u32 tail_or_chunk, u32 wide)
{
    if (!team_width_ok(G)) return -2;
    u32 const stream = stream_and_strategy & 0xFFu, sbyte = (stream_and_strategy >> 8) & 0xFFu;
    KBigLevel const b = { sbyte == 4u ? 0u : sbyte, sbyte == 1u ? stream_and_strategy >> 16 : 0u, sbyte == 4u };
    bool const streaming = stream == KXF_STREAM || stream == KXF_STREAM_EMPTY_END;
    Work w(n, 128u * 1024u);
    KBatchView const v = w.view(src, in_off, in_len, n, dst, out_off, out_len);
    std::vector<KFrameState> fstate(n);
    std::vector<u32> hufct((size_t)n * 512, 0xDEADBEEFu);
    std::vector<u32> big_tables((size_t)n * (b.level4 ? KX_BIG4_ENTRIES : KX_BIG_TBL_ENTRIES), 0u);
    u32 remaining = 0, counter = 0;
    for (u32 i = 0; i < n; i++) {           // (k_zstd_frame_init)
        KFrameState s; memset(&s, 0, sizeof(s));
        s.blockSize = in_len[i] < KX_BLOCK_MAX ? in_len[i] : KX_BLOCK_MAX; s.first = 1; s.rep[0] = 1; s.rep[1] = 4; s.rep[2] = 8;
        s.lowLimit = 2; s.dictLimit = 2; s.chunkEnd = (stream != KXF_ONE_SHOT && in_len[i] > KX_BLOCK_MAX) ? KX_BLOCK_MAX : in_len[i];
        if (b.level4 && !streaming && !kx_l4_served(in_len[i])) { s.blockSize = 0; s.chunkEnd = 0; fstate[i] = s; out_len[i] = 0; continue; }      // (refused size class)
        fstate[i] = s;
        if (in_len[i] == 0) { u8* d = dst + out_off[i]; u32 const magic = 0xFD2FB528u, wd = kx_big_window_byte(stream, b.strategy); memcpy(d, &magic, 4); d[4] = wd ? 0x00 : 0x20; d[5] = (u8)wd; d[6] = 1; d[7] = 0; d[8] = 0; out_len[i] = 9; }
        else remaining++;
    }
    KMatchArgs const m = kx_match_args_blk(v, kx_one_piece(nullptr, nullptr), &counter, streaming, wide != 0, fstate.data(), big_tables.data(), b.level4);
    KFrameArgs const e = kx_frame_args(v, fstate.data(), hufct.data(), &remaining, nullptr, stream, b, tail_or_chunk);
    if (b.strategy && rounds_out) return -6;
    if (!rounds_out) {
        // product path: one wave per slice walks its chain of blocks
        std::vector<u32> counters(nblocks, 0u);
        KBigArgs g = kx_big_args(m, e, counters.data(), (n > 2 && 64 / G >= 2) ? 2 : 1);
        kxemu::failed = 0;
        if (b.strategy == 2u && !streaming) {
            // level 2, sizes known: the slices of its double-fast row first, the others through the fast parser below
            kx_big_set_class(g, m.flags, KXC_L2_DFAST);
            by_team_width(G, [&](auto tw) { kxemu::launch(nblocks, [&]() { zstd_big_body<decltype(tw)::value>(g); }); });
            if (kxemu::failed) return -1;
            for (auto& x : counters) x = 0;
            kx_big_set_class(g, m.flags, KXC_L2_FAST);
        }
        if (b.strategy) by_team_width(G, [&](auto tw) { kxemu::launch(nblocks, [&]() { zstd_big_body<decltype(tw)::value, true>(g); }); });
        else by_team_width(G, [&](auto tw) { kxemu::launch(nblocks, [&]() { zstd_big_body<decltype(tw)::value>(g); }); });
        if (kxemu::failed) return -1;
        for (u32 i = 0; i < n; i++) if (fstate[i].blockSize != 0) return -5;
        return 0;
    }
    // the block rounds as separate launches (the ablation build's KMP_BIG_ROUNDS=1)
    u32 rounds = 0;
    while (remaining != 0) {
        if (++rounds > 20000) return -4;
        counter = 0; kxemu::failed = 0;
        by_team_width(G, [&](auto tw) { kxemu::launch(nblocks, [&]() { zstd_match_body<decltype(tw)::value, true>(m); }); });
        if (kxemu::failed) return -1;
        // the blocks libzstd parses with the extDict variant (behind a wrap of its staging buffer)
        counter = 0;
        by_team_width(G, [&](auto tw) { kxemu::launch(nblocks, [&]() { zstd_match_ext_body<decltype(tw)::value>(m); }); });
        if (kxemu::failed) return -1;
        for (u32 i = 0; i < n; i++) if (fstate[i].blockSize >= 8 && w.meta[i].status) return -3;
        kxemu::launch(nblocks, [&]() { zstd_frame_body(e); });
        if (kxemu::failed) return -1;
    }
    *rounds_out = rounds;
    return 0;
}

#include "zstd_decode.h"
#include "zstd_predecode.h"
extern "C" __attribute__((visibility("default")))
int emu_zstd_decompress_dict(const u8* src, const u64* in_off, const u32* in_len, u32 n, u32 nblocks,
                             u8* dst, const u64* out_off, const u32* out_cap, u32* out_len, u32* status, u32 lit_cap,
                             const u8* dict, u32 dict_size);
extern "C" __attribute__((visibility("default")))
int emu_zstd_decompress(const u8* src, const u64* in_off, const u32* in_len, u32 n, u32 nblocks,
                        u8* dst, const u64* out_off, const u32* out_cap, u32* out_len, u32* status, u32 lit_cap)
{ return emu_zstd_decompress_dict(src, in_off, in_len, n, nblocks, dst, out_off, out_cap, out_len, status, lit_cap, nullptr, 0); }
extern "C" __attribute__((visibility("default")))
int emu_zstd_decompress_dict(const u8* src, const u64* in_off, const u32* in_len, u32 n, u32 nblocks,
                             u8* dst, const u64* out_off, const u32* out_cap, u32* out_len, u32* status, u32 lit_cap,
                             const u8* dict, u32 dict_size)
{
    std::vector<u8> lits((size_t)n * lit_cap, 0xEE);
    KDecodeArgs d;
    d.src = src; d.in_off = in_off; d.in_len = in_len; d.n_slices = n;
    d.dst = dst; d.out_off = out_off; d.out_cap = out_cap; d.out_len = out_len; d.status = status;
    d.lits = lits.data(); d.lit_cap = lit_cap; d.flags = 0; d.dict = dict; d.dict_size = dict ? dict_size : 0;
    // (a formatted dictionary: the host code's steps of zstd_decompress_impl)
    KDictDPrior dprior; u32 start_rep[3] = { 1, 4, 8 };
    if (dict && dict_size >= 8) {
        size_t off = 0;
        int const formatted = cdict_parse_formatted(dict, dict_size, nullptr, &off, &dprior);
        if (formatted < 0) return -7;
        if (formatted) { d.dict = dict + off; d.dict_size = dict_size - (u32)off; d.dprior = &dprior; d.dict_id = dprior.dictID; start_rep[0] = dprior.rep[0]; start_rep[1] = dprior.rep[1]; start_rep[2] = dprior.rep[2]; }
    }
    // sequences decoded ahead, one lane per frame (what the product does); KXEMU_NO_PRE=1: everything in the decode body
    u32 const seq_cap = lit_cap / 3u + 64u, blk_cap = lit_cap / 8192u + 16u;
    std::vector<u64> stage; std::vector<KPreBlk> pblk; std::vector<u32> nblk;
    d.pre_stage = nullptr; d.pre_seq_cap = 0; d.pre_blk = nullptr; d.pre_blk_cap = 0; d.pre_nblk = nullptr;
    kxemu::failed = 0;
    // as the product: the pre-decoders take their entries in order of sequence count (the product sorts batches of 1024 and more;
    // here every batch of 4 and more, so that the CPU suite covers the mapping)
    std::vector<u32> skey(n, 0u), sperm(n, 0u), shist(KXP_SORT_BUCKETS, 0u);
    bool const sorted = n >= 4 && !getenv("KXEMU_NO_PRE");
    if (sorted) {
        KSeqSortArgs sa;
        sa.src = src; sa.in_off = in_off; sa.in_len = in_len; sa.n_slices = n; sa.key = skey.data(); sa.hist = shist.data(); sa.perm = sperm.data(); sa.len_shift = 0;
        kxemu::launch_block((n + 255) / 256, 4, [&]() { zstd_seq_count_body(sa); });
        kxemu::launch_block(1, 4, [&]() { zstd_seq_rank_body(sa); });
        kxemu::launch_block((n + 255) / 256, 4, [&]() { zstd_seq_perm_body(sa); });
        if (kxemu::failed) return -5;
    }
    if (!getenv("KXEMU_NO_PRE")) {
        stage.assign((size_t)n * seq_cap, 0xCDCDCDCDCDCDCDCDull); pblk.resize((size_t)n * blk_cap); nblk.assign(n, 0u);
        KPreArgs p;
        p.src = src; p.in_off = in_off; p.in_len = in_len; p.n_slices = n;
        p.stage = stage.data(); p.seq_cap = seq_cap; p.blk = pblk.data(); p.blk_cap = blk_cap; p.nblk = nblk.data(); p.perm = sorted ? sperm.data() : nullptr;
        p.rep[0] = start_rep[0]; p.rep[1] = start_rep[1]; p.rep[2] = start_rep[2];
        kxemu::launch((n + KXP_FRAMES - 1) / KXP_FRAMES, [&]() { zstd_seq_predecode_body(p); });
        if (kxemu::failed) return -2;
        d.pre_stage = stage.data(); d.pre_seq_cap = seq_cap; d.pre_blk = pblk.data(); d.pre_blk_cap = blk_cap; d.pre_nblk = nblk.data();
    }
    std::vector<u8> plits; std::vector<KPreLit> plrec; std::vector<u32> nlit;
    d.pre_lits = nullptr; d.pre_lit_cap = 0; d.pre_lit = nullptr; d.pre_nlit = nullptr; d.pre_blk_cap = blk_cap;
    if (!getenv("KXEMU_NO_PRE")) {
        u32 const plcap = lit_cap + 64u;
        plits.assign((size_t)n * plcap, 0xABu); plrec.resize((size_t)n * blk_cap); nlit.assign(n, 0u);
        KLitArgs p;
        p.src = src; p.in_off = in_off; p.in_len = in_len; p.n_slices = n;
        p.lits = plits.data(); p.lit_cap = plcap; p.rec = plrec.data(); p.blk_cap = blk_cap; p.nrec = nlit.data(); p.perm = sorted ? sperm.data() : nullptr;
        kxemu::launch((n + KXL_FRAMES - 1) / KXL_FRAMES, [&]() { zstd_lit_predecode_body(p); });
        if (kxemu::failed) return -3;
        d.pre_lits = plits.data(); d.pre_lit_cap = plcap; d.pre_lit = plrec.data(); d.pre_nlit = nlit.data();
    }
    kxemu::launch(nblocks, [&]() { zstd_decode_body(d); });
    return kxemu::failed ? -1 : 0;
}

// the counting sort that orders the pre-decoders' lane slots by sequence count (zstd_predecode.h): count, rank, perm
extern "C" __attribute__((visibility("default")))
int emu_seq_sort_by(const u8* src, const u64* in_off, const u32* in_len, u32 n, u32* key, u32* perm, u32 len_shift);
extern "C" __attribute__((visibility("default")))
int emu_seq_sort(const u8* src, const u64* in_off, const u32* in_len, u32 n, u32* key, u32* perm) { return emu_seq_sort_by(src, in_off, in_len, n, key, perm, 0); }
// len_shift != 0: keyed by the entry's size (what inflate's pre-decoder is given)
extern "C" __attribute__((visibility("default")))
int emu_seq_sort_by(const u8* src, const u64* in_off, const u32* in_len, u32 n, u32* key, u32* perm, u32 len_shift)
{
    std::vector<u32> hist(KXP_SORT_BUCKETS, 0u);
    KSeqSortArgs sa;
    sa.src = src; sa.in_off = in_off; sa.in_len = in_len; sa.n_slices = n; sa.key = key; sa.hist = hist.data(); sa.perm = perm; sa.len_shift = len_shift;
    kxemu::failed = 0;
    kxemu::launch_block((n + 255) / 256, 4, [&]() { zstd_seq_count_body(sa); });
    if (kxemu::failed) return -1;
    kxemu::launch_block(1, 4, [&]() { zstd_seq_rank_body(sa); });
    if (kxemu::failed) return -2;
    kxemu::launch_block((n + 255) / 256, 4, [&]() { zstd_seq_perm_body(sa); });
    return kxemu::failed ? -3 : 0;
}

#include "deflate_match.h"
#include "deflate_lazy.h"
#include "deflate_encode.h"
// raw DEFLATE level 6 pipeline (chains -> best -> parse -> encode) on the emulator
extern "C" __attribute__((visibility("default")))
int emu_deflate_level(const u8* src, const u64* in_off, const u32* in_len, u32 n, u8* dst, const u64* out_off, u32* out_len,
                      u16* link_out, KdBest* best_out, u32 format, int level);
extern "C" __attribute__((visibility("default")))
int emu_deflate(const u8* src, const u64* in_off, const u32* in_len, u32 n, u8* dst, const u64* out_off, u32* out_len,
                u16* link_out, KdBest* best_out, u32 format)
{ return emu_deflate_level(src, in_off, in_len, n, dst, out_off, out_len, link_out, best_out, format, 6); }
extern "C" __attribute__((visibility("default")))
int emu_deflate_params(const u8* src, const u64* in_off, const u32* in_len, u32 n, u8* dst, const u64* out_off, u32* out_len,
                       u16* link_out, KdBest* best_out, u32 format, int level, int window_bits, int mem_level, int old_kernels);
extern "C" __attribute__((visibility("default")))
int emu_deflate_level(const u8* src, const u64* in_off, const u32* in_len, u32 n, u8* dst, const u64* out_off, u32* out_len,
                      u16* link_out, KdBest* best_out, u32 format, int level)
{ return emu_deflate_params(src, in_off, in_len, n, dst, out_off, out_len, link_out, best_out, format, level, 15, 8, 0); }
// ... with deflateInit2's windowBits / memLevel; old_kernels: the chain / all-positions search / lane-per-slice parse also for slices up to 64 KiB
extern "C" __attribute__((visibility("default")))
int emu_deflate_params(const u8* src, const u64* in_off, const u32* in_len, u32 n, u8* dst, const u64* out_off, u32* out_len,
                       u16* link_out, KdBest* best_out, u32 format, int level, int window_bits, int mem_level, int old_kernels)
{
    u32 maxlen = 65536u;
    for (u32 i = 0; i < n; i++) if (in_len[i] > maxlen) maxlen = in_len[i];
    u32 const pos_cap = (maxlen + 63u) & ~63u, blk_cap = kd_block_cap(pos_cap, 1u << (mem_level + 6));
    std::vector<u16> link((size_t)n * pos_cap, 0xEEEE);
    std::vector<KdBest> best((size_t)n * pos_cap * 2);
    std::vector<u32> syms((size_t)n * pos_cap, 0xDDDDDDDDu);
    std::vector<u32> wrv((size_t)n * pos_cap, 0xCCCCCCCCu);
    std::vector<KdSliceMeta> meta(n);
    std::vector<KdBlockInfo> blocks((size_t)n * blk_cap);
    KdArgs a;
    a.wr = wrv.data();
    a.src = src; a.in_off = in_off; a.in_len = in_len; a.n_slices = n;
    a.pos_cap = pos_cap; a.blk_cap = blk_cap; a.blocks = blocks.data();
    a.link = link.data(); a.best = best.data(); a.syms = syms.data(); a.meta = meta.data();
    a.dst = dst; a.out_off = out_off; a.out_len = out_len; a.flags = 0; a.format = format;
    kd_level_config(a, level, window_bits, mem_level);
    kxemu::failed = 0;
    if (level >= 1 && level <= 3) {
        memset((void*)best.data(), 0, (size_t)n * (a.hmask + 1u) * 4u);
        kxemu::launch((n + 63) / 64, [&]() { deflate_fast_body(a); });
        if (kxemu::failed) return -3;
        kxemu::launch(n < 3 ? n : 3, [&]() { deflate_encode_body(a); });
        return kxemu::failed ? -4 : 0;
    }
    // slices up to 64 KiB: the sort + wave-wide lazy parse of deflate_lazy.h (what the product runs there), unless the caller wants the
    // chain links / per-position records of the older kernels back (link_out / best_out) -- the tests keep both pipelines honest
    if (pos_cap > 65536u && !link_out && !best_out && !old_kernels) {
        // slices above 64 KiB: segment by segment, as deflate_batch_impl does (the search arrays hold one 64 KiB span per slice)
        std::vector<u16> rankv((size_t)n * 65536u, 0xBBBB);
        std::vector<u32> statev((size_t)n * KDL_STATE_WORDS, 0xAAAAAAAAu);
        a.seg_rank = rankv.data(); a.seg_state = statev.data();
        u32 const segs = (maxlen - KDL_SEG_SPAN + KDL_SEG_STEP - 1u) / KDL_SEG_STEP + 1u;
        for (u32 seg = 0; seg < segs; seg++) {
            a.seg = seg;
            if (a.hmask > 0x7FFFu) kxemu::launch_block(n < 2 ? n : 2, 4, [&]() { deflate_sort_body<16, true>(a); });
            else kxemu::launch_block(n < 2 ? n : 2, 4, [&]() { deflate_sort_body<15, true>(a); });
            if (kxemu::failed) return -1;
            kxemu::launch(n < 3 ? n : 3, [&]() { deflate_lazy_body<true>(a); });
            if (kxemu::failed) return -3;
        }
        kxemu::launch(n < 3 ? n : 3, [&]() { deflate_encode_body(a); });
        return kxemu::failed ? -4 : 0;
    }
    if (pos_cap <= 65536u && !link_out && !best_out && !old_kernels) {
        if (a.hmask > 0x7FFFu) kxemu::launch_block(n < 2 ? n : 2, 4, [&]() { deflate_sort_body<16>(a); });
        else kxemu::launch_block(n < 2 ? n : 2, 4, [&]() { deflate_sort_body<15>(a); });
        if (kxemu::failed) return -1;
        kxemu::launch(n < 3 ? n : 3, [&]() { deflate_lazy_body<false>(a); });
        if (kxemu::failed) return -3;
        kxemu::launch(n < 3 ? n : 3, [&]() { deflate_encode_body(a); });
        return kxemu::failed ? -4 : 0;
    }
    if (pos_cap <= 65536u) kxemu::launch_block(n < 2 ? n : 2, 4, [&]() { deflate_chains_body<u16>(a); });
    else kxemu::launch_block(n < 2 ? n : 2, 4, [&]() { deflate_chains_body<u32>(a); });
    if (kxemu::failed) return -1;
    kxemu::launch_block(n < 2 ? n : 2, 16, [&]() { deflate_best_body(a); });
    if (kxemu::failed) return -2;
    // the parse over the records: a wave per slice (what the product runs), or the earlier lane per slice (old_kernels == 2)
    if (old_kernels == 2) kxemu::launch((n + 63) / 64, [&]() { deflate_parse_body(a); });
    else kxemu::launch(n < 3 ? n : 3, [&]() { deflate_parse_wave_body(a); });
    if (kxemu::failed) return -3;
    kxemu::launch(n < 3 ? n : 3, [&]() { deflate_encode_body(a); });
    if (kxemu::failed) return -4;
    if (link_out) memcpy(link_out, link.data(), link.size() * 2);
    if (best_out) memcpy(best_out, best.data(), (size_t)n * pos_cap * sizeof(KdBest));
    return 0;
}

#include "deflate_predecode.h"
// the two-kernel inflate (lane-per-stream pre-decoder, then the executor / inflate_stream for what it did not cover);
// covered_out[i] = 1 where the pre-decoder's staging was executed.  stage_bytes: the size the staging is made for
// (max_slice_bytes of a context)
extern "C" __attribute__((visibility("default")))
int emu_inflate_pre(const u8* src, const u64* in_off, const u32* in_len, u32 n, u8* dst, const u64* out_off, const u32* out_cap,
                    u32* out_len, int* status, u32 format, u32 stage_bytes, u32* covered_out)
{
    u32 const seq_cap = stage_bytes / 3u + 64u, lit_cap = stage_bytes + 64u;
    std::vector<u64> stage((size_t)n * seq_cap, 0xDDDDDDDDDDDDDDDDull);
    std::vector<u8> lits((size_t)n * lit_cap, 0xEE);
    std::vector<u32> nseq(n, 0x12345678u), nlit(n, 0x12345678u);
    KipArgs p;
    p.src = src; p.in_off = in_off; p.in_len = in_len; p.n_slices = n; p.out_cap = out_cap; p.format = format;
    p.stage = stage.data(); p.seq_cap = seq_cap; p.lits = lits.data(); p.lit_cap = lit_cap; p.nseq = nseq.data(); p.nlit = nlit.data();
    std::vector<u32> perm(n), skey(n);                      // the host's order: by compressed size, largest first
    { u32 sh = 1; while ((stage_bytes >> sh) >= KXP_SORT_BUCKETS) sh++; if (emu_seq_sort_by(src, in_off, in_len, n, skey.data(), perm.data(), sh) != 0) return -3; }
    p.perm = perm.data();
    kxemu::failed = 0;
    kxemu::launch((n + KIP_STREAMS - 1) / KIP_STREAMS, [&]() { inflate_predecode_body(p); });
    if (kxemu::failed) return -1;
    for (u32 i = 0; i < n; i++) if (covered_out) covered_out[i] = nseq[i] >> 31;
    KieArgs e;
    e.i.src = src; e.i.in_off = in_off; e.i.in_len = in_len; e.i.n_slices = n;
    e.i.dst = dst; e.i.out_off = out_off; e.i.out_cap = out_cap; e.i.out_len = out_len; e.i.status = status; e.i.format = format;
    e.stage = stage.data(); e.seq_cap = seq_cap; e.lits = lits.data(); e.lit_cap = lit_cap; e.nseq = nseq.data(); e.nlit = nlit.data();
    kxemu::launch(n < 3 ? n : 3, [&]() { inflate_exec_body(e); });
    return kxemu::failed ? -2 : 0;
}

extern "C" __attribute__((visibility("default")))
int emu_inflate(const u8* src, const u64* in_off, const u32* in_len, u32 n, u8* dst, const u64* out_off, const u32* out_cap,
                u32* out_len, int* status, u32 format)
{
    KiArgs a;
    a.src = src; a.in_off = in_off; a.in_len = in_len; a.n_slices = n;
    a.dst = dst; a.out_off = out_off; a.out_cap = out_cap; a.out_len = out_len; a.status = status; a.format = format;
    kxemu::failed = 0;
    kxemu::launch(n < 3 ? n : 3, [&]() { inflate_body(a); });
    return kxemu::failed ? -1 : 0;
}

// kx_xcd_chunk (zstd_common.h): the slice a virtual workgroup index takes
extern "C" __attribute__((visibility("default")))
unsigned emu_xcd_chunk(unsigned it, unsigned n) { return kx_xcd_chunk(it, n); }

