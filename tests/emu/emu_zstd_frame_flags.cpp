// TEST INFRASTRUCTURE: the frame flags (kmp_batch_set_frame_flags) on the CPU wave emulator: a batch view with the flags and its checksum
// words, the XXH64 pass of a batch with KXH_CHECKSUM, then the level's parse and frame writers with the argument structs zstd_launch.h
// builds from that view -- the steps of kmp_batch.hip's compress paths.  Built into a library of its own (tests/helpers_frame_flags.py)
// together with emu_core.cpp.
#include "kx_wave.h"
#include "emu_core.h"
#include "zstd_launch.h"
#include "zstd_cdict_host.h"
#include <stdlib.h>
#include <vector>

namespace {
bool any_status(const KSliceMeta* meta, const u32* in_len, u32 n) { for (u32 i = 0; i < n; i++) if (in_len[i] >= 8 && meta[i].status) return true; return false; }

// k_zstd_frame_init
void frame_init(KBatchView const& v, KFrameState* fstate, u32* remaining, u32 wd, bool chunked)
{
    for (u32 i = 0; i < v.n; i++) {
        KFrameState s; memset(&s, 0, sizeof(s));
        u32 const len = v.in_len[i];
        s.blockSize = len < KX_BLOCK_MAX ? len : KX_BLOCK_MAX; s.first = 1; s.rep[0] = 1; s.rep[1] = 4; s.rep[2] = 8;
        s.lowLimit = 2; s.dictLimit = 2; s.chunkEnd = (chunked && len > KX_BLOCK_MAX) ? KX_BLOCK_MAX : len;
        fstate[i] = s;
        if (len == 0) {
            u8* d = v.dst + v.out_off[i];
            if (wd) { kx_st32(d, 0xFD2FB528u); d[4] = (u8)((v.fflags & KXH_CHECKSUM) ? 1u << 2 : 0u); d[5] = (u8)wd; }
            else kx_write_frame_header(d, 0, kx_window_log_src(0), v.fflags);
            d[6] = 1; d[7] = 0; d[8] = 0; v.out_len[i] = kx_frame_end(d, 9, v.fflags, v.cks, i);
        } else (*remaining)++;
    }
}
}

// level: 3, 1, 2, a negative one, or 5 .. 8; with a dictionary (dict_size != 0): 3, 1, 2 or a negative one, slices up to 128 KiB.
// slice_cap above 128 KiB: the paths of a context for frames of several blocks (every slice through the block chain; levels 5 .. 8: the
// one-block kernels, then zstd_lazy_big.h's chain).  stream: KFrameArgs.stream, on those paths at levels up to 3.
// Returns 0, -1 a kernel body failed, -2 bad arguments, -3 a parser guard, -4 damaged dictionary, -5 a frame left open
extern "C" __attribute__((visibility("default")))
int emu_zstd_compress_flags(const u8* src, const u64* in_off, const u32* in_len, u32 n, int G, u32 nblocks,
                            u8* dst, const u64* out_off, u32* out_len, u32 slice_cap, const u8* dict, u32 dict_size, int level, u32 fflags, u32 stream)
{
    if (!(G == 2 || G == 4 || G == 8 || G == 16 || G == 32 || G == 64)) return -2;
    bool const big = slice_cap > KX_BLOCK_MAX, fast = level == 1 || level == 2 || level < 0, lazy = level >= 5 && level <= 8;
    if (!(level == 3 || fast || lazy) || (dict_size && (big || lazy)) || (stream && (!big || lazy))) return -2;
    KWorkCaps const cap = kx_work_caps(big ? KX_BLOCK_MAX : slice_cap);
    std::vector<KSeq> seqs((size_t)n * cap.seq_cap); std::vector<u8> lits((size_t)n * cap.lit_cap, 0xEE); std::vector<KSliceMeta> meta(n);
    memset((void*)meta.data(), 0, meta.size() * sizeof(KSliceMeta));
    std::vector<u32> scratch((size_t)n * cap.scratch_words, 0xA5A5A5A5u), cks(n, 0xDEADBEEFu);
    KBatchView v = { src, in_off, in_len, dst, out_off, out_len, n, seqs.data(), lits.data(), meta.data(), scratch.data(), cap };
    v.fflags = fflags; v.cks = (fflags & KXH_CHECKSUM) ? cks.data() : nullptr;          // (batch_view)
    kxemu::failed = 0;
    if (v.cks) {                                                                         // (frame_checksums)
        KSeekXxhArgs const x = kx_frame_xxh_args(v);
        kxemu::launch_block(kx_frame_xxh_blocks(n) < nblocks ? kx_frame_xxh_blocks(n) : nblocks, 4, [&]() { seekable_xxh64_body(x); });
        if (kxemu::failed) return -1;
    }
    u32 const teams = nblocks * (64u / (u32)G);
    std::vector<u32> tables((size_t)teams * KX_TBL_ENTRIES, 0xDEADBEEFu & 0x0003FFFFu), epochs(teams, 7u);
    KTeamTables const tt = kx_one_piece(tables.data(), epochs.data());
    u32 counter = 0;

    if (dict_size) {
        // zstd_compress_dict
        u32 W, C, H, M;
        KDictPrior prior; size_t content_off = 0;
        int const formatted = cdict_parse_formatted(dict, dict_size, &prior, &content_off);
        if (formatted < 0) return -4;
        int const cls = kx_dict_level_class(level);
        cdict_params(dict_size, &W, &C, &H, &M, cls);
        const u8* const content = dict + content_off; u32 const content_size = dict_size - (u32)content_off;
        std::vector<u32> tl, ts;
        u32 eflags = KXE_GATHER_LITS;
        if (cls == 3) {
            cdict_fill(tl, H, ts, C, M, content, content_size);
            KDictArgs const g = kx_dict_args(v, tt, &counter, content, content_size, tl.data(), ts.data(), W, H, C, M, formatted ? prior.rep[0] : 1u, formatted ? prior.rep[1] : 4u);
            by_team_width(G, [&](auto tw) { kxemu::launch(nblocks, [&]() { zstd_match_dict_body<decltype(tw)::value>(g); }); });
        } else {
            cdict_fill_fast(tl, H, C, M, content, content_size);
            KFastDictArgs const g = kx_fast_dict_args(v, tt, &counter, content, content_size, tl.data(), W, H, M, formatted ? prior.rep[0] : 1u, formatted ? prior.rep[1] : 4u, level);
            by_team_width(G, [&](auto tw) { kxemu::launch(nblocks, [&]() { zstd_match_fast_dict_body<decltype(tw)::value>(g); }); });
            eflags = kx_entropy_flags_fast(level < 0);
        }
        if (kxemu::failed) return -1;
        if (any_status(meta.data(), in_len, n)) return -3;
        KEntropyArgs const e = kx_entropy_args(v, eflags, formatted ? &prior : nullptr, dict_size);
        if (formatted) kxemu::launch(nblocks, [&]() { zstd_entropy_body<true>(e); });
        else kxemu::launch(nblocks, [&]() { zstd_entropy_body(e); });
        return kxemu::failed ? -1 : 0;
    }

    if (!big && !lazy) {
        // zstd_compress_dfast / the "fast" levels of kmp_zstd_compress_batch_level
        u32 eflags;
        if (fast) {
            KFastArgs const g = kx_fast_args(v, tt, &counter, level);
            by_team_width(G, [&](auto tw) { kxemu::launch(nblocks, [&]() { zstd_match_fast_body<decltype(tw)::value>(g); }); });
            eflags = kx_entropy_flags_fast(level < 0);
        } else {
            KMatchArgs const m = kx_match_args(v, tt, &counter, 0u);
            by_team_width(G, [&](auto tw) { kxemu::launch(nblocks, [&]() { zstd_match_body<decltype(tw)::value>(m); }); });
            eflags = kx_entropy_flags_dfast(m.flags, false);
        }
        if (kxemu::failed) return -1;
        if (any_status(meta.data(), in_len, n)) return -3;
        KEntropyArgs const e = kx_entropy_args(v, eflags);
        kxemu::launch(nblocks, [&]() { zstd_entropy_body(e); });
        return kxemu::failed ? -1 : 0;
    }

    std::vector<KFrameState> fstate(n); std::vector<u32> hufct((size_t)n * 512, 0xDEADBEEFu);
    u32 remaining = 0, status = 0;
    if (lazy) {
        // zstd_compress_lazy / zstd_compress_lazy_big: the one-block slices (the longer ones read as empty there), then the chains
        std::vector<u32> small_len(n);
        for (u32 i = 0; i < n; i++) small_len[i] = in_len[i] > KX_BLOCK_MAX ? 0u : in_len[i];
        KBatchView sv = v; sv.in_len = small_len.data();
        {
            std::vector<KLazyRec> rec((size_t)n * cap.pos_cap); std::vector<u32> wr((size_t)n * cap.pos_cap, 0xDEADBEEFu);
            KLazyArgs const g = kx_lazy_args(sv, rec.data(), wr.data(), cap.pos_cap, level);
            kxemu::launch_block(nblocks, 4, [&]() { zstd_lazy_sort_body(g); });
            if (kxemu::failed) return -1;
            if (cap.pos_cap <= 65536u) kxemu::launch(nblocks, [&]() { zstd_lazy_body<2048>(g); }); else kxemu::launch(nblocks, [&]() { zstd_lazy_body<4096>(g); });
            if (kxemu::failed) return -1;
            KEntropyArgs const e = kx_entropy_args(sv, kx_entropy_flags_lazy(level));
            kxemu::launch(nblocks, [&]() { zstd_entropy_body(e); });
            if (kxemu::failed) return -1;
        }
        if (!big) return any_status(meta.data(), in_len, n) ? -3 : 0;
        u64 const slot_bytes = kx_lazy_big_slot_bytes(kx_lazy_big_hash_log_max(slice_cap));
        std::vector<u8> ltab((size_t)n * slot_bytes, 0x5Au);
        std::vector<KSeqPrev> prev(n); memset((void*)prev.data(), 0x7F, prev.size() * sizeof(KSeqPrev));
        for (u32 i = 0; i < n; i++) {           // (k_zstd_lazy_big_init)
            bool refused;
            zstd_lazy_big_init_slice(in_len[i], fstate[i], prev[i], refused);
            if (refused) return -2;
            if (fstate[i].blockSize) remaining++;
        }
        KLazyBigArgs const g = kx_lazy_big_args(v, fstate.data(), hufct.data(), &remaining, &status, ltab.data(), slot_bytes, prev.data(), level);
        kxemu::launch(nblocks, [&]() { zstd_lazy_big_body(g); });
        if (kxemu::failed) return -1;
    } else {
        // zstd_compress_big
        KBigLevel const b = kx_big_level(level);
        bool const streaming = stream == KXF_STREAM || stream == KXF_STREAM_EMPTY_END;
        std::vector<u32> big_tables((size_t)n * KX_BIG_TBL_ENTRIES, 0u);
        frame_init(v, fstate.data(), &remaining, kx_big_window_byte(stream, b.strategy), stream != KXF_ONE_SHOT);
        KMatchArgs const m = kx_match_args_blk(v, kx_one_piece(nullptr, nullptr), &counter, streaming, false, fstate.data(), big_tables.data(), false);
        KFrameArgs const e = kx_frame_args(v, fstate.data(), hufct.data(), &remaining, &status, stream, b, 0);
        std::vector<u32> counters(nblocks, 0u);
        KBigArgs g = kx_big_args(m, e, counters.data(), (n > 2 && 64 / G >= 2) ? 2 : 1);
        if (b.strategy == 2u && !streaming) {
            kx_big_set_class(g, m.flags, KXC_L2_DFAST);
            by_team_width(G, [&](auto tw) { kxemu::launch(nblocks, [&]() { zstd_big_body<decltype(tw)::value>(g); }); });
            if (kxemu::failed) return -1;
            for (auto& x : counters) x = 0;
            kx_big_set_class(g, m.flags, KXC_L2_FAST);
        }
        if (b.strategy) by_team_width(G, [&](auto tw) { kxemu::launch(nblocks, [&]() { zstd_big_body<decltype(tw)::value, true>(g); }); });
        else by_team_width(G, [&](auto tw) { kxemu::launch(nblocks, [&]() { zstd_big_body<decltype(tw)::value>(g); }); });
        if (kxemu::failed) return -1;
    }
    for (u32 i = 0; i < n; i++) if (fstate[i].blockSize != 0) return -5;
    return (remaining != 0 || (status & 2u)) ? -5 : 0;
}
