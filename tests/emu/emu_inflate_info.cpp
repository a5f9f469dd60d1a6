// TEST INFRASTRUCTURE: the body of k_inflate_size (kompressor_amd/csrc/deflate_info.h) on the CPU wave emulator.  Built into a
// library of its own (tests/helpers_inflate_info.py) together with emu_core.cpp.
#include "kx_wave.h"
#include "emu_core.h"
#include "deflate_info.h"

// n entries src[in_off[i] .. + in_len[i]) -> info[i], as the library launches the kernel: KIP_STREAMS entries per one-wave workgroup.
// Returns 0, -1 when the emulator reported a failure.
extern "C" __attribute__((visibility("default")))
int emu_inflate_info(const u8* src, const u64* in_off, const u32* in_len, u32 n, u32 format, kmp_inflate_info* info)
{
    KisArgs a;
    a.src = src; a.in_off = in_off; a.in_len = in_len; a.n_slices = n; a.info = info; a.format = format;
    kxemu::failed = 0;
    kxemu::launch((n + KIP_STREAMS - 1) / KIP_STREAMS, [&]() { inflate_size_body(a); });
    return kxemu::failed ? -1 : 0;
}
