// TEST INFRASTRUCTURE: a stand-alone program around the emulator's decode entry point (emu_zstd_decompress: the sort, both pre-decoders
// and k_zstd_decode's body), built by tests/test_emu_handmade.py with g++ -fsanitize=address,undefined together with emu_core.cpp and
// emu_zstd.cpp.  It reads the cases the test wrote (u32 count; per case u32 length, u32 capacity, u32 the library's status, u32 the
// library's output length (for the two entries the decoder is held to refuse though the library accepts them, that refusal), u32 lenient, the bytes), copies each entry into a heap block of exactly its length and decodes it into a heap
// block of exactly its capacity, alone (KXEMU_NO_PRE) and behind the pre-decoders: a read or write outside either block, or an index
// outside an LDS array (the tables hostile descriptions fill: weights[256], keepNorm[3][64]), is a sanitizer error.  Exit 0: nothing
// found, and every entry accepted exactly where the library accepts it, with the library's length.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

extern "C" int emu_zstd_decompress(const uint8_t* src, const uint64_t* in_off, const uint32_t* in_len, uint32_t n, uint32_t nblocks,
                                   uint8_t* dst, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, uint32_t* status, uint32_t lit_cap);

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t n = 0, bad = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t h[5];
        if (fread(h, 4, 5, f) != 5) return 2;
        uint32_t const len = h[0], cap = h[1], want = h[2], want_len = h[3], lenient = h[4];
        uint8_t* const p = (uint8_t*)malloc(len);          // (exactly the entry)
        uint8_t* const out = (uint8_t*)malloc(cap);        // (exactly the capacity)
        if (len && fread(p, 1, len, f) != len) return 2;
        for (int pre = 0; pre < 2; pre++) {
            if (pre) unsetenv("KXEMU_NO_PRE"); else setenv("KXEMU_NO_PRE", "1", 1);
            uint64_t const zero = 0; uint32_t out_len = 0xEEEEEEEEu, status = 0xEEEEEEEEu;
            int const r = emu_zstd_decompress(p, &zero, &len, 1, 1, out, &zero, &cap, &out_len, &status, 128 * 1024 + 64);
            bool const ok = r == 0 && (want ? status != 0 && out_len == 0 : (status == 0 && out_len == want_len) || (lenient && status != 0 && out_len == 0));
            if (!ok) { fprintf(stderr, "entry %u (%u bytes, capacity %u, %s): emulator %d, status %u, length %u; the library: %u, %u\n", i, len, cap,
                               pre ? "pre-decoders" : "alone", r, status, out_len, want, want_len); bad++; }
        }
        free(p); free(out);
    }
    fclose(f);
    printf("%u entries, %u findings\n", n, bad);
    return bad ? 1 : 0;
}
