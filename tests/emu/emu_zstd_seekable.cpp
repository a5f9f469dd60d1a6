// TEST INFRASTRUCTURE: the kernel bodies of zstd's seekable container (kompressor_amd/csrc/zstd_seekable.h) on the CPU wave emulator:
// plan, XXH64 (summing and verifying), table, and the table's validation.  Built into a library of its own (tests/helpers_seekable.py)
// together with emu_core.cpp; the chunks' frames come from the compress kernels of the main emulator library.
#include "kx_wave.h"
#include "emu_core.h"
#include "zstd_seekable.h"

#define EMU_API extern "C" __attribute__((visibility("default")))

// every entry point: 0, or -1 when the emulator reported a failure (diverged lanes, a barrier not reached)
EMU_API int emu_seekable_plan(u64 src_size, u32 frame_bytes, u32 n, u64 stride, u64* in_off, u32* in_len, u64* out_off, u32 nblocks)
{
    KSeekPlanArgs const a = { src_size, frame_bytes, n, stride, in_off, in_len, out_off };
    kxemu::failed = 0;
    kxemu::launch_block(nblocks, 4, [&]() { seekable_plan_body(a); });
    return kxemu::failed ? -1 : 0;
}
// cks != null: the checksums of n pieces; else the verifying form (expect: 12-byte entries, status: updated in place)
EMU_API int emu_seekable_xxh64(const u8* src, const u64* off, const u32* len, u32 n, u32* cks, const u8* expect, u32* status, u32 nblocks, int waves)
{
    KSeekXxhArgs const a = { src, off, len, n, cks, expect, status };
    kxemu::failed = 0;
    kxemu::launch_block(nblocks, waves, [&]() { seekable_xxh64_body(a); });
    return kxemu::failed ? -1 : 0;
}
// one workgroup, as the library launches it
EMU_API int emu_seekable_table(u8* dst, const u64* dense_off, const u32* clen, const u32* dlen, const u32* cks, u32 n, u32 flags,
                               const u32* ctx_status, u64* result, int waves)
{
    KSeekTableArgs const a = { dst, dense_off, clen, dlen, cks, n, flags, ctx_status, result };
    kxemu::failed = 0;
    kxemu::launch_block(1, waves, [&]() { seekable_table_body(a); });
    return kxemu::failed ? -1 : 0;
}
EMU_API int emu_seekable_index(const u8* blob, u64 size, kmp_seekable_stat* out)
{
    kxemu::failed = 0;
    kxemu::launch_block(1, 1, [&]() { seekable_index_body(blob, size, out); });
    return kxemu::failed ? -1 : 0;
}
