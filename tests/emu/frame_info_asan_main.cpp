// TEST INFRASTRUCTURE: a stand-alone program around kx_frame_info (kompressor_amd/csrc/zstd_frame_info.h), built by
// tests/helpers_frame_info.py with g++ -fsanitize=address,undefined.  It reads the cases the test wrote (u32 count; per entry u32
// length, the bytes, the expected 32-byte kmp_zstd_frame_info), copies each entry into a heap block of exactly its length -- a read
// past its end or in front of its start is a sanitizer error -- and compares the answers.  Exit 0: every entry parsed and equal.
#include "zstd_frame_info.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t n = 0, bad = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t len = 0;
        kmp_zstd_frame_info want, got;
        if (fread(&len, 4, 1, f) != 1) return 2;
        uint8_t* const p = (uint8_t*)malloc(len);          // (exactly the entry: length 0 gives a block with no byte to read)
        if (len && fread(p, 1, len, f) != len) return 2;
        if (fread(&want, sizeof want, 1, f) != 1) return 2;
        memset(&got, 0xEE, sizeof got);
        kx_frame_info(p, len, &got);
        if (memcmp(&got, &want, sizeof got) != 0) {
            fprintf(stderr, "entry %u (%u bytes): content %llu bound %llu status %u frames %u dict_id %u flags %u, expected %llu %llu %u %u %u %u\n", i, len,
                    (unsigned long long)got.content, (unsigned long long)got.bound, got.status, got.frames, got.dict_id, got.flags,
                    (unsigned long long)want.content, (unsigned long long)want.bound, want.status, want.frames, want.dict_id, want.flags);
            bad++;
        }
        free(p);
    }
    fclose(f);
    printf("%u entries, %u differ\n", n, bad);
    return bad ? 1 : 0;
}
