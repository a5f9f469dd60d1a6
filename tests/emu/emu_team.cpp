// TEST INFRASTRUCTURE: the shared team pieces of the zstd parsers (kompressor_amd/csrc/zstd_team.h) on the CPU wave emulator: KSeqSink
// driven directly, and the parse bodies alone (no entropy stage) for the slice records they leave.  Built into a library of its own
// (tests/helpers_team.py) together with emu_core.cpp.
#include "kx_wave.h"
#include "emu_core.h"
#include "zstd_launch.h"
#include "zstd_cdict_host.h"
#include <vector>

namespace {
template <int G>
void sink_body(KSeq* seqs, const u32* in, u32 n, KSliceMeta* meta)
{
    auto const [lane, k, tbase, tmask, team] = kx_team<G>(0);
    // every team of the wave sees the same pushes and owns a region of its own: `per` entries, an even count, so that every region
    // starts on a 16-byte boundary as a slice's sequences do
    u32 const per = (n + 2 * G + 8 + 1) & ~1u;
    KSeqSink sink = { nullptr };
    sink.reset(seqs + (size_t)team * per);
    for (u32 i = 0; i < n; i++) sink.push<G>(k, in[3 * i], (int)in[3 * i + 1], in[3 * i + 2]);
    sink.flush<G>(k);
    if (lane == 0) *meta = sink.meta(77u, 5u);
    (void)tbase; (void)tmask;
}
}

// in: n triples (offBase, ll, mlBase).  seqs: 16-byte aligned, 64 / G regions of n + 2 G + 8 entries rounded up to an even count,
// prefilled by the caller.
extern "C" __attribute__((visibility("default")))
int emu_team_sink(int G, KSeq* seqs, const u32* in, u32 n, KSliceMeta* meta)
{
    kxemu::failed = 0;
    switch (G) {
    case 2:  kxemu::launch(1, [&]() { sink_body<2>(seqs, in, n, meta); }); break;
    case 8:  kxemu::launch(1, [&]() { sink_body<8>(seqs, in, n, meta); }); break;
    case 64: kxemu::launch(1, [&]() { sink_body<64>(seqs, in, n, meta); }); break;
    default: return -2;
    }
    return kxemu::failed ? -1 : 0;
}

// The parse body of a level alone -> the slices' records.  level 3 or 1; dict != nullptr: the two dictionary bodies (raw content).
extern "C" __attribute__((visibility("default")))
int emu_team_parse_meta(const u8* src, const u64* in_off, const u32* in_len, u32 n, int G, u32 nblocks, u32 slice_cap,
                        const u8* dict, u32 dict_size, int level, KSliceMeta* meta)
{
    if (G != 4 && G != 8) return -2;
    KWorkCaps const cap = kx_work_caps(slice_cap);
    std::vector<KSeq> seqs((size_t)n * cap.seq_cap); std::vector<u8> lits((size_t)n * cap.lit_cap, 0xEE);
    KBatchView const v = { src, in_off, in_len, nullptr, nullptr, nullptr, n, seqs.data(), lits.data(), meta, nullptr, cap };
    u32 const teams = nblocks * (64u / (u32)G);
    // team tables: stale entries of epoch 0 (tag and check bits zero, a junk index), every team at epoch 7
    u32 const stale = 0xDEADBEEFu & KX_IDX_MASK;
    std::vector<u32> tables((size_t)teams * KX_TBL_ENTRIES, stale), epochs(teams, 7u);
    KTeamTables const t = kx_one_piece(tables.data(), epochs.data());
    u32 counter = 0, W, C, H, M;
    kxemu::failed = 0;
    if (!dict && level == 3) {
        KMatchArgs const a = kx_match_args(v, t, &counter, 0u);
        by_team_width(G, [&](auto w) { kxemu::launch(nblocks, [&]() { zstd_match_body<decltype(w)::value>(a); }); });
    } else if (!dict) {
        KFastArgs const g = kx_fast_args(v, t, &counter, level);
        by_team_width(G, [&](auto w) { kxemu::launch(nblocks, [&]() { zstd_match_fast_body<decltype(w)::value>(g); }); });
    } else if (level == 3) {
        cdict_params(dict_size, &W, &C, &H, &M);
        std::vector<u32> tl, ts;
        cdict_fill(tl, H, ts, C, M, dict, dict_size);
        KDictArgs const g = kx_dict_args(v, t, &counter, dict, dict_size, tl.data(), ts.data(), W, H, C, M, 1u, 4u);
        by_team_width(G, [&](auto w) { kxemu::launch(nblocks, [&]() { zstd_match_dict_body<decltype(w)::value>(g); }); });
    } else {
        cdict_params(dict_size, &W, &C, &H, &M, level);
        std::vector<u32> th;
        cdict_fill_fast(th, H, C, M, dict, dict_size);
        KFastDictArgs const g = kx_fast_dict_args(v, t, &counter, dict, dict_size, th.data(), W, H, M, 1u, 4u, level);
        by_team_width(G, [&](auto w) { kxemu::launch(nblocks, [&]() { zstd_match_fast_dict_body<decltype(w)::value>(g); }); });
    }
    return kxemu::failed ? -1 : 0;
}
