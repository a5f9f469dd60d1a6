// TEST INFRASTRUCTURE: the kernel bodies of the BGZF container (kompressor_amd/csrc/bgzf.h) on the CPU wave emulator: plan, wrap,
// finish, the verify pass, the serial walk as the kernel runs it, and the parallel open -- the same sequence of launches as
// bgzf_open_impl (kmp_bgzf.hip) makes, with the candidate cap as an argument.  Built into a library of its own (tests/helpers_bgzf.py)
// together with emu_core.cpp; the blocks' DEFLATE streams come from the kernels of the main emulator library.
#include "kx_wave.h"
#include "emu_core.h"
#include "zstd_seekable.h"
#include "bgzf.h"

#include <vector>

#define EMU_API extern "C" __attribute__((visibility("default")))

// every entry point: 0, or -1 when the emulator reported a failure (diverged lanes, a barrier not reached)
EMU_API int emu_bgzf_plan(u64 src_size, u32 block_bytes, u32 n, u64 stride, u64* in_off, u32* in_len, u64* out_off, u32 nblocks)
{
    KSeekPlanArgs const a = { src_size, block_bytes, n, stride, in_off, in_len, out_off };
    kxemu::failed = 0;
    kxemu::launch_block(nblocks, 4, [&]() { seekable_plan_body(a); });
    return kxemu::failed ? -1 : 0;
}
EMU_API int emu_bgzf_wrap(const u8* src, const u64* in_off, const u32* in_len, u8* frames, const u64* out_off, u32* out_len, u32 n, u32 nblocks)
{
    KBgzfWrapArgs const a = { src, in_off, in_len, frames, out_off, out_len, n };
    kxemu::failed = 0;
    kxemu::launch_block(nblocks, 1, [&]() { bgzf_wrap_body(a); });
    return kxemu::failed ? -1 : 0;
}
EMU_API int emu_bgzf_finish(u8* dst, const u64* dense_off, const u32* out_len, u32 n, u32 flags, const u32* ctx_status, u64* result, int waves)
{
    KBgzfFinishArgs const a = { dst, dense_off, out_len, n, flags, ctx_status, result };
    kxemu::failed = 0;
    kxemu::launch_block(1, waves, [&]() { bgzf_finish_body(a); });
    return kxemu::failed ? -1 : 0;
}
EMU_API int emu_bgzf_verify(const u8* blob, const u64* in_off, const u32* in_len, const u8* dst, const u64* out_off, const u32* out_len, const u32* out_cap,
                            int32_t* status, u32 n, u32 verify, u32 nblocks)
{
    KBgzfVerifyArgs const a = { blob, in_off, in_len, dst, out_off, out_len, out_cap, status, n, verify };
    kxemu::failed = 0;
    kxemu::launch_block(nblocks, 1, [&]() { bgzf_verify_body(a); });
    return kxemu::failed ? -1 : 0;
}
// k_bgzf_walk; in_off null: the stat and the prefix arrays alone
EMU_API int emu_bgzf_walk(const u8* blob, u64 size, kmp_bgzf_stat* stat, u64* member_off, u64* content_off, u64 cap, u64* in_off, u32* in_len, u32* out_cap)
{
    KBgzfArrays const arr = { in_off, in_len, out_cap };
    kxemu::failed = 0;
    kxemu::launch_block(1, 1, [&]() { bgzf_walk_body(blob, size, stat, member_off, content_off, cap, arr); });
    return kxemu::failed ? -1 : 0;
}
// the head test alone (compiled for the host), for the tests that compare it with the restatement position by position
EMU_API int emu_bgzf_head(const u8* blob, u64 size, u64 p, u32* out4)
{
    KBgzfHead h = { 0, 0, 0, 0 };
    int const st = kx_bgzf_head(blob, size, p, &h);
    out4[0] = h.total; out4[1] = h.xlen; out4[2] = h.isize; out4[3] = h.extra;
    return st;
}

// ---- the parallel open --------------------------------------------------------------------------------------------------------------
template <class T> struct Guarded {                 // a buffer of exactly n entries between canaries
    std::vector<u8> mem; size_t n;
    explicit Guarded(size_t count) : mem(count * sizeof(T) + 128, 0xA5), n(count) {}
    T* p() { return (T*)(mem.data() + 64); }
    bool intact() const
    {
        for (size_t i = 0; i < 64; i++) if (mem[i] != 0xA5 || mem[mem.size() - 1 - i] != 0xA5) return false;
        return true;
    }
};

static u32 scan_tiles(const u8* blob, u64 size, u64 ntiles, u32* tiles, const u32* base, KBgzfCand* cand, u32 nblocks)
{
    KBgzfScanArgs const a = { blob, size, ntiles, tiles, base, cand };
    kxemu::launch_block(nblocks, 4, [&]() { bgzf_scan_body(a); });
    return 0;
}

// first: the candidates alone (the first host wait); -1: the emulator failed
EMU_API int64_t emu_bgzf_count(const u8* blob, u64 size, u32 nblocks, int waves)
{
    u64 const ntiles = (size + KBZ_TILE - 1u) / KBZ_TILE;
    Guarded<u32> tiles(ntiles + 1);
    kxemu::failed = 0;
    scan_tiles(blob, size, ntiles, tiles.p(), nullptr, nullptr, nblocks);
    kxemu::launch_block(1, waves, [&]() { bgzf_prefix_body(tiles.p(), ntiles); });
    if (kxemu::failed || !tiles.intact()) return -1;
    return tiles.p()[ntiles];
}
// The open as bgzf_open_impl runs it.  The output arrays hold room + 1 entries, room = what emu_bgzf_count said (or, on the walk's path,
// the members the first walk found: the caller sizes them by either).  info[0] = 1 parallel / 2 the serial walk; info[1] = candidates;
// info[2] = doubling levels.  Returns 0, -1 (the emulator failed), -2 (a canary of the open's own tables is gone), -3 (room too small).
EMU_API int emu_bgzf_open(const u8* blob, u64 size, u32 max_candidates, kmp_bgzf_stat* stat, u64* member_off, u64* content_off, u64* in_off, u32* in_len,
                          u32* out_cap, u64 room, u32* info, u32 nblocks, int waves)
{
    kxemu::failed = 0;
    KBgzfArrays const arr = { in_off, in_len, out_cap };
    info[0] = 0; info[1] = 0; info[2] = 0;
    auto walk = [&]() {
        info[0] = 2;
        KBgzfArrays const none = { nullptr, nullptr, nullptr };
        kxemu::launch_block(1, 1, [&]() { bgzf_walk_body(blob, size, stat, nullptr, nullptr, 0, none); });
        if (kxemu::failed) return -1;
        if (stat->status != 0) return 0;
        if (stat->blocks > room) return -3;
        kxemu::launch_block(1, 1, [&]() { bgzf_walk_body(blob, size, stat, member_off, content_off, (u64)stat->blocks + 1u, arr); });
        return kxemu::failed ? -1 : 0;
    };
    if (size == 0 || max_candidates == 0) return walk();
    u64 const ntiles = (size + KBZ_TILE - 1u) / KBZ_TILE;
    Guarded<u32> tiles(ntiles + 1);
    scan_tiles(blob, size, ntiles, tiles.p(), nullptr, nullptr, nblocks);
    kxemu::launch_block(1, waves, [&]() { bgzf_prefix_body(tiles.p(), ntiles); });
    if (kxemu::failed) return -1;
    u32 const n = tiles.p()[ntiles];
    info[1] = n;
    if (n > max_candidates) return walk();
    if (n > room) return -3;
    info[0] = 1;
    u32 levels = 0;
    while (levels < 32u && (1ull << levels) < n) levels++;
    info[2] = levels;
    Guarded<KBgzfCand> cand(n); Guarded<u32> jump((size_t)n * (levels ? levels : 1u)), mark(n);
    if (n) {
        scan_tiles(blob, size, ntiles, tiles.p(), tiles.p(), cand.p(), nblocks + 1u);
        KBgzfLinkArgs const lk = { cand.p(), n, size, jump.p(), mark.p() };
        kxemu::launch_block(nblocks, 4, [&]() { bgzf_link_body(lk); });
        for (u32 k = 1; k < levels; k++)
            kxemu::launch_block(nblocks, 4, [&]() { bgzf_double_body(jump.p() + (size_t)(k - 1u) * n, jump.p() + (size_t)k * n, n); });
        for (u32 k = levels; k-- > 0;)
            kxemu::launch_block(nblocks, 4, [&]() { bgzf_mark_body(jump.p() + (size_t)k * n, mark.p(), n); });
    }
    KBgzfGatherArgs const g = { blob, size, cand.p(), jump.p(), mark.p(), n, member_off, content_off, arr, stat };
    kxemu::launch_block(1, waves, [&]() { bgzf_gather_body(g); });
    if (kxemu::failed) return -1;
    return tiles.intact() && cand.intact() && jump.intact() && mark.intact() ? 0 : -2;
}
