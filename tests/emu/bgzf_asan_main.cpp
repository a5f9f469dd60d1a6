// TEST INFRASTRUCTURE: a stand-alone program around kx_bgzf_head and kx_bgzf_walk (kompressor_amd/csrc/bgzf.h), built by
// tests/helpers_bgzf.py with g++ -fsanitize=address,undefined.  It reads the cases the test wrote (u32 count; per blob u32 length, the
// bytes, the expected 32-byte kmp_bgzf_stat), copies each blob into a heap block of exactly its length -- a read past its end or in
// front of its start is a sanitizer error --, runs the head test at EVERY position of the blob (what the parallel open's scan may do),
// then the walk twice as kmp_bgzf_index_host does, the second time into prefix arrays of exactly blocks + 1 entries, and compares the
// answers.  Exit 0: every blob walked and equal.
#include "bgzf.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t n = 0, bad = 0;
    unsigned long long heads = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t len = 0;
        kmp_bgzf_stat want, got, again;
        if (fread(&len, 4, 1, f) != 1) return 2;
        uint8_t* const p = (uint8_t*)malloc(len);          // (exactly the blob: length 0 gives a block with no byte to read)
        if (len && fread(p, 1, len, f) != len) return 2;
        if (fread(&want, sizeof want, 1, f) != 1) return 2;
        for (uint64_t at = 0; at <= len; at++) { KBgzfHead h; if (kx_bgzf_head(p, len, at, &h) == 0) heads++; }
        memset(&got, 0xEE, sizeof got); memset(&again, 0xEE, sizeof again);
        kx_bgzf_walk(p, len, &got, NULL, NULL, 0);
        if (got.status == 0) {
            uint64_t* const mo = (uint64_t*)malloc(((size_t)got.blocks + 1) * 8);
            uint64_t* const co = (uint64_t*)malloc(((size_t)got.blocks + 1) * 8);
            kx_bgzf_walk(p, len, &again, mo, co, (uint64_t)got.blocks + 1);
            if (memcmp(&got, &again, sizeof got) != 0 || mo[got.blocks] != len || co[got.blocks] != got.content || mo[0] != 0 || co[0] != 0) {
                fprintf(stderr, "blob %u: the second walk differs from the first\n", i);
                bad++;
            }
            free(mo); free(co);
        }
        if (memcmp(&got, &want, sizeof got) != 0) {
            fprintf(stderr, "blob %u (%u bytes): status %d blocks %u content %llu flags %u, expected %d %u %llu %u\n", i, len, got.status, got.blocks,
                    (unsigned long long)got.content, got.flags, want.status, want.blocks, (unsigned long long)want.content, want.flags);
            bad++;
        }
        free(p);
    }
    fclose(f);
    printf("%u blobs, %u differ, %llu valid heads\n", n, bad, heads);
    return bad ? 1 : 0;
}
