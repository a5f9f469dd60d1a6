// TEST INFRASTRUCTURE: a stand-alone program around inflate_size_body (kompressor_amd/csrc/deflate_info.h) on the wave emulator, built
// by tests/helpers_inflate_info.py with g++ -fsanitize=address,undefined together with emu_core.cpp.  It reads the cases the test wrote
// (u32 count; per entry u32 length, u32 format, the bytes, the expected 32-byte kmp_inflate_info), copies each entry into a heap block
// of exactly its length -- a read past its end or in front of its start is a sanitizer error --, walks the entries of each format as one
// batch and compares the answers.  Exit 0: every entry walked and equal.
#include "kx_wave.h"
#include "emu_core.h"
#include "deflate_info.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t n = 0, bad = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    std::vector<u8*> block(n); std::vector<u32> len(n), fmt(n); std::vector<kmp_inflate_info> want(n);
    for (uint32_t i = 0; i < n; i++) {
        if (fread(&len[i], 4, 1, f) != 1 || fread(&fmt[i], 4, 1, f) != 1 || fmt[i] > 3) return 2;
        block[i] = (u8*)malloc(len[i]);                     // (exactly the entry: length 0 gives a block with no byte to read)
        if (len[i] && fread(block[i], 1, len[i], f) != len[i]) return 2;
        if (fread(&want[i], sizeof want[i], 1, f) != 1) return 2;
    }
    fclose(f);
    const u8* base = nullptr;                               // the lowest block: every offset from it is positive
    for (uint32_t i = 0; i < n; i++) if (!base || block[i] < base) base = block[i];
    for (u32 format = 0; format < 4; format++) {
        std::vector<u64> off; std::vector<u32> ln, who;
        for (uint32_t i = 0; i < n; i++) if (fmt[i] == format) { off.push_back((u64)(block[i] - base)); ln.push_back(len[i]); who.push_back(i); }
        if (who.empty()) continue;
        std::vector<kmp_inflate_info> got(who.size());
        memset(got.data(), 0xEE, got.size() * sizeof got[0]);
        KisArgs a;
        a.src = base; a.in_off = off.data(); a.in_len = ln.data(); a.n_slices = (u32)who.size(); a.info = got.data(); a.format = format;
        kxemu::failed = 0;
        kxemu::launch((a.n_slices + KIP_STREAMS - 1) / KIP_STREAMS, [&]() { inflate_size_body(a); });
        if (kxemu::failed) { fprintf(stderr, "the emulator reported a failure (format %u)\n", format); return 3; }
        for (size_t k = 0; k < who.size(); k++) if (memcmp(&got[k], &want[who[k]], sizeof got[k]) != 0) {
            kmp_inflate_info const& g = got[k]; kmp_inflate_info const& w = want[who[k]];
            fprintf(stderr, "entry %u (%u bytes, format %u): content %llu status %d blocks %u flags %u window_bits %u, expected %llu %d %u %u %u\n", who[k], ln[k], format,
                    (unsigned long long)g.content, g.status, g.blocks, g.flags, g.window_bits, (unsigned long long)w.content, w.status, w.blocks, w.flags, w.window_bits);
            bad++;
        }
    }
    for (uint32_t i = 0; i < n; i++) free(block[i]);
    printf("%u entries, %u differ\n", n, bad);
    return bad ? 1 : 0;
}
