// TEST INFRASTRUCTURE: a stand-alone program around kx_seekable_index (kompressor_amd/csrc/zstd_seekable.h), built by
// tests/helpers_seekable.py with g++ -fsanitize=address,undefined.  It reads the cases the test wrote (u32 count; per blob u32 length, the
// bytes, the expected 40-byte kmp_seekable_stat), copies each blob into a heap block of exactly its length -- a read past its end or in
// front of its start is a sanitizer error -- and compares the answers.  Exit 0: every blob validated and equal.
#include "zstd_seekable.h"
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
        kmp_seekable_stat want, got;
        if (fread(&len, 4, 1, f) != 1) return 2;
        uint8_t* const p = (uint8_t*)malloc(len);          // (exactly the blob: length 0 gives a block with no byte to read)
        if (len && fread(p, 1, len, f) != len) return 2;
        if (fread(&want, sizeof want, 1, f) != 1) return 2;
        memset(&got, 0xEE, sizeof got);
        kx_seekable_index(p, len, &got);
        if (memcmp(&got, &want, sizeof got) != 0) {
            fprintf(stderr, "blob %u (%u bytes): status %u frames %u content %llu table_off %llu, expected %u %u %llu %llu\n", i, len, got.status, got.frames,
                    (unsigned long long)got.content, (unsigned long long)got.table_off, want.status, want.frames,
                    (unsigned long long)want.content, (unsigned long long)want.table_off);
            bad++;
        }
        free(p);
    }
    fclose(f);
    printf("%u blobs, %u differ\n", n, bad);
    return bad ? 1 : 0;
}
