// TEST INFRASTRUCTURE: the bodies of k_zstd_frame_info and k_batch_layout (kompressor_amd/csrc/zstd_frame_info.h) on the CPU wave
// emulator.  Built into a library of its own (tests/helpers_frame_info.py) together with emu_core.cpp.
#include "kx_wave.h"
#include "emu_core.h"
#include "zstd_frame_info.h"

// n entries src[in_off[i] .. + in_len[i]) -> info[i]; the grid is nblocks workgroups of `waves` waves (grid-stride over n).
// Returns 0, -1 when the emulator reported a failure.
extern "C" __attribute__((visibility("default")))
int emu_zstd_frame_info(const u8* src, const u64* in_off, const u32* in_len, u32 n, u32 nblocks, int waves, kmp_zstd_frame_info* info)
{
    KFrameInfoArgs const a = { src, in_off, in_len, n, info };
    kxemu::failed = 0;
    kxemu::launch_block(nblocks, waves, [&]() { zstd_frame_info_body(a); });
    return kxemu::failed ? -1 : 0;
}

// the layout kernel as the library launches it: one workgroup of KFI_LAYOUT_WAVES waves
extern "C" __attribute__((visibility("default")))
int emu_batch_layout(const kmp_zstd_frame_info* info, u32 n, u32 align, u64* out_off, u32* out_cap, u64* total)
{
    KLayoutArgs const a = { info, n, align, out_off, out_cap, total };
    kxemu::failed = 0;
    kxemu::launch_block(1, KFI_LAYOUT_WAVES, [&]() { batch_layout_body(a); });
    return kxemu::failed ? -1 : 0;
}
