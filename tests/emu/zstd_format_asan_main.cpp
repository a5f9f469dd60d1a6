// TEST INFRASTRUCTURE: a stand-alone program around the two section readers of kompressor_amd/csrc/zstd_format.h, built by
// tests/test_emu_decode_status.py with g++ -fsanitize=address,undefined.  Input: u32 count; per body u32 length, the bytes (bodies of
// compressed blocks).  For every body and EVERY prefix length L the prefix is copied into a heap block of exactly L bytes -- a read
// at or beyond the bound is a sanitizer error -- and zf_literals(p, L) and zf_sequences(p, pos, L) are called: the latter where the
// literals section ends (once that is known) and at every position within 4 bytes of the bound.  Once a reader has said that the
// header fits (the count is there; the modes byte is there), a longer prefix may not change a field.  Exit 0: no finding.
#include "zstd_format.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static bool same(const ZfLiterals& a, const ZfLiterals& b) { return memcmp(&a, &b, sizeof a) == 0; }

// the fields a longer prefix may still change: none once the modes byte is there (or the count is 0); have_modes, modes and next before
static bool grew(const ZfSequences& was, const ZfSequences& now)
{
    if (!was.have_count) return true;
    if (!now.have_count || now.count != was.count) return false;
    if (was.have_modes || was.count == 0) return memcmp(&was, &now, sizeof was) == 0;
    return now.have_modes ? now.next == was.next + 1 : memcmp(&was, &now, sizeof was) == 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s bodies.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t n = 0, bad = 0;
    unsigned long long calls = 0;
    if (fread(&n, 4, 1, f) != 1) return 2;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t len = 0;
        if (fread(&len, 4, 1, f) != 1) return 2;
        std::vector<uint8_t> body(len);
        if (len && fread(body.data(), 1, len, f) != len) return 2;
        ZfLiterals lit0; memset(&lit0, 0, sizeof lit0);
        ZfSequences at_end; memset(&at_end, 0, sizeof at_end);
        std::vector<ZfSequences> near(len + 1);                 // what zf_sequences said at each position, at the last bound tried
        memset(near.data(), 0, near.size() * sizeof(ZfSequences));
        for (uint32_t L = 0; L <= len; L++) {
            uint8_t* const p = (uint8_t*)malloc(L);             // (exactly the prefix: length 0 gives a block with no byte to read)
            if (L) memcpy(p, body.data(), L);
            ZfLiterals const lit = zf_literals(p, L); calls++;
            if (lit0.fits && !same(lit0, lit)) { fprintf(stderr, "body %u: the literals header changed at prefix %u\n", i, L); bad++; }
            if (lit.fits && lit.header > L) { fprintf(stderr, "body %u: a literals header of %u bytes fits %u\n", i, lit.header, L); bad++; }
            if (!lit0.fits) lit0 = lit;
            if (lit0.fits && lit0.section <= L) {
                ZfSequences const s = zf_sequences(p, lit0.section, L); calls++;
                if (!grew(at_end, s) || s.next > L) { fprintf(stderr, "body %u: the sequences header behind the literals changed at prefix %u\n", i, L); bad++; }
                at_end = s;
            }
            for (uint32_t pos = L > 4 ? L - 4 : 0; pos <= L; pos++) {
                ZfSequences const s = zf_sequences(p, pos, L); calls++;
                if (!grew(near[pos], s) || s.next > L || s.next < pos) { fprintf(stderr, "body %u: the sequences header at %u changed at prefix %u\n", i, pos, L); bad++; }
                near[pos] = s;
            }
            free(p);
        }
    }
    fclose(f);
    printf("%u bodies, %u findings, %llu calls\n", n, bad, calls);
    return bad ? 1 : 0;
}
