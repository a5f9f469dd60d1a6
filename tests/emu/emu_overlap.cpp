// TEST INFRASTRUCTURE: the entropy sweeps beside the level-3 parse (kmp_batch.hip zstd_compress_dfast's overlapped path) on the CPU wave
// emulator: the parse body with its completion records, then the entropy body with KXE_SWEEP over `done` sets the caller reveals in
// an order of its choosing, then the final sweep.  Arguments and thresholds come from the product's launch description
// (zstd_launch.h).  Built into a library of its own (tests/test_emu_overlap.py) together with emu_core.cpp.
#include "kx_wave.h"
#include "emu_core.h"
#include "zstd_launch.h"
#include <vector>

namespace {
struct Work {
    KWorkCaps cap; std::vector<KSeq> seqs; std::vector<u8> lits; std::vector<KSliceMeta> meta; std::vector<u32> scratch;
    Work(u32 n, u32 block_cap) : cap(kx_work_caps(block_cap)), seqs((size_t)n * cap.seq_cap), lits((size_t)n * cap.lit_cap, 0xEE), meta(n), scratch((size_t)n * cap.scratch_words, 0xA5A5A5A5u) {}
};
}

// The parse (team width 4) leaves done[i] and *done_count; level4 != 0: level 4's double-fast row, which refuses slices of up to 16 KiB
// (their records carry status 3).  Then, unless dst is null: for every cut c of `cuts` (ascending counts) the slices order[0 .. c) are
// revealed as done and a sweep runs; at the end everything the parse marked is revealed and the final sweep runs.  swept: ncuts + 1
// counts of slices coded.  status: the slices' record status words (n).
extern "C" __attribute__((visibility("default")))
int emu_overlap_compress(const u8* src, const u64* in_off, const u32* in_len, u32 n, u32 nblocks, u32 slice_cap, int level4,
                         u32* done, u32* done_count, u32* status,
                         u8* dst, const u64* out_off, u32* out_len, const u32* order, const u32* cuts, u32 ncuts, u32* swept)
{
    Work w(n, slice_cap);
    KBatchView const v = { src, in_off, in_len, dst, out_off, out_len, n, w.seqs.data(), w.lits.data(), w.meta.data(), w.scratch.data(), w.cap };
    u32 const teams = nblocks * 16u;
    std::vector<u32> tables((size_t)teams * (level4 ? KX_TBL4_ENTRIES : KX_TBL_ENTRIES), 0xDEADBEEFu & 0x0003FFFFu), epochs(teams, 7u);
    std::vector<u32> coded(n, 0u), visible(n, 0u);
    for (u32 i = 0; i < n; i++) done[i] = 0;
    *done_count = 0;
    u32 counter = 0;
    KMatchArgs m = kx_match_args(v, kx_one_piece(tables.data(), epochs.data(), level4 != 0), &counter, KXM_NT_STORES | KXM_NO_LITS);
    KSweepRecords const parse_rec = { done, coded.data(), done_count };
    kx_match_records(m, parse_rec);
    kxemu::failed = 0;
    kxemu::launch(nblocks, [&]() { zstd_match_body<4>(m); });
    if (kxemu::failed) return -1;
    for (u32 i = 0; i < n; i++) status[i] = w.meta[i].status;
    if (!dst) return 0;
    KEntropyArgs const e = kx_entropy_args(v, kx_entropy_flags_dfast(m.flags, level4 != 0));
    KSweepRecords const rec = { visible.data(), coded.data(), done_count };
    u32 shown = 0;
    for (u32 j = 0; j <= ncuts; j++) {
        if (j < ncuts) { for (; shown < cuts[j] && shown < n; shown++) visible[order[shown]] = done[order[shown]]; }
        else for (u32 i = 0; i < n; i++) visible[i] = done[i];
        swept[j] = 0;
        KEntropyArgs const s = kx_entropy_sweep_args(e, rec, swept + j);
        kxemu::launch(nblocks, [&]() { zstd_entropy_body(s); });
        if (kxemu::failed) return -1;
    }
    for (u32 i = 0; i < n; i++) if (!coded[i]) return -4;
    return 0;
}

// kx_sweep_thresholds: the counts the host's stream waits use
extern "C" __attribute__((visibility("default")))
u32 emu_overlap_thresholds(u32 n, u32 K, u32* T) { return kx_sweep_thresholds(n, K, T); }
