// TEST INFRASTRUCTURE: zstd levels 1, 2 and the negative ones with a dictionary (kmp_batch.hip kmp_zstd_compress_batch_dict_level's
// steps) on the CPU wave emulator: the host's CDict of strategy "fast", zstd_match_fast_dict.h's body, the entropy body.  Built into a
// library of its own (tests/helpers_dict_levels.py) together with emu_core.cpp.
#include "kx_wave.h"
#include "emu_core.h"
#include "zstd_launch.h"
#include "zstd_cdict_host.h"
#include <stdlib.h>
#include <vector>

// status_out: 1 when a parser guard tripped.  Returns 0, -1 a kernel body failed, -2 bad team width, -4 damaged formatted dictionary
extern "C" __attribute__((visibility("default")))
int emu_zstd_compress_dict_level(const u8* src, const u64* in_off, const u32* in_len, u32 n, int G, u32 nblocks,
                                 u8* dst, const u64* out_off, u32* out_len, u32 slice_cap, const u8* dict, u32 dict_size, int level, u32* status_out)
{
    if (!(G == 2 || G == 4 || G == 8 || G == 16 || G == 32 || G == 64)) return -2;
    if (!(level == 1 || level == 2 || (level < 0 && level >= -131072))) return -5;
    KWorkCaps const cap = kx_work_caps(slice_cap);
    std::vector<KSeq> seqs((size_t)n * cap.seq_cap); std::vector<u8> lits((size_t)n * cap.lit_cap, 0xEE); std::vector<KSliceMeta> meta(n);
    memset((void*)meta.data(), 0x6B, meta.size() * sizeof(KSliceMeta));          // (what an earlier batch might have left)
    std::vector<u32> scratch((size_t)n * cap.scratch_words, 0xA5A5A5A5u);
    KBatchView const v = { src, in_off, in_len, dst, out_off, out_len, n, seqs.data(), lits.data(), meta.data(), scratch.data(), cap };
    // team tables: stale entries of epoch 0, every team at epoch 7
    u32 const teams = nblocks * (64u / (u32)G);
    std::vector<u32> tables((size_t)teams * KX_TBL_ENTRIES, 0xDEADBEEFu & 0x0003FFFFu), epochs(teams, 7u);
    u32 counter = 0, W, C, H, M;
    KDictPrior prior; size_t content_off = 0;
    int const formatted = cdict_parse_formatted(dict, dict_size, &prior, &content_off);
    if (formatted < 0) return -4;
    cdict_params(dict_size, &W, &C, &H, &M, level);
    dict += content_off; dict_size -= (u32)content_off;
    std::vector<u32> t;
    cdict_fill_fast(t, H, C, M, dict, dict_size);
    KFastDictArgs const g = kx_fast_dict_args(v, kx_one_piece(tables.data(), epochs.data()), &counter, dict, dict_size, t.data(), W, H, M,
                                              formatted ? prior.rep[0] : 1u, formatted ? prior.rep[1] : 4u, level);
    kxemu::failed = 0;
    by_team_width(G, [&](auto tw) { kxemu::launch(nblocks, [&]() { zstd_match_fast_dict_body<decltype(tw)::value>(g); }); });
    if (kxemu::failed) return -1;
    u32 status = 0;
    for (u32 i = 0; i < n; i++) if (in_len[i] >= 8 && meta[i].status) status = 1;
    if (status_out) *status_out = status;
    KEntropyArgs const e = kx_entropy_args(v, kx_entropy_flags_fast(level < 0), formatted ? &prior : nullptr);
    if (formatted) kxemu::launch(nblocks, [&]() { zstd_entropy_body<true>(e); });
    else kxemu::launch(nblocks, [&]() { zstd_entropy_body(e); });
    return kxemu::failed ? -1 : 0;
}

// the host's CDict parameters at a level: windowLog, chainLog, hashLog, minMatch
extern "C" __attribute__((visibility("default")))
void emu_dict_level_params(u32 dict_size, int level, u32* out4) { cdict_params(dict_size, &out4[0], &out4[1], &out4[2], &out4[3], level); }
