// TEST INFRASTRUCTURE: zstd levels 5 .. 10 as streams and as the reference driver's staged frames (kmp_batch.hip zstd_compress_lazy_big's
// steps with a mode) on the CPU wave emulator.  Built into a library of its own (tests/helpers_lazy_stream.py) together with emu_core.cpp.
#include "kx_wave.h"
#include "emu_core.h"
#include "zstd_launch.h"
#include <stdlib.h>
#include <vector>

// mode: KFrameArgs.stream (1 stream, 2 stream closed by a call without data, 3 the reference's one-shot driver; out_chunk: its output slices,
// 0 = max(8192, n / 10)).  status_out: the context's status word (KMP_STATUS_* bits); out_len 0 = refused.  piece: table slots (slices in
// flight), 0 = all.  slot_bytes_out: what a table slot was sized to.
extern "C" __attribute__((visibility("default")))
int emu_zstd_compress_lazy_stream(const u8* src, const u64* in_off, const u32* in_len, u32 n, u32 nblocks,
                                  u8* dst, const u64* out_off, u32* out_len, u32 slice_cap, int level, u32 mode, u32 out_chunk, u32 piece,
                                  u32* status_out, u64* slot_bytes_out)
{
    if (mode < KXF_STREAM || mode > KXF_REFERENCE) return -2;
    bool const streaming = mode != KXF_REFERENCE;
    u32 const block_cap = 128u * 1024u;
    KWorkCaps const cap = kx_work_caps(block_cap);
    std::vector<KSeq> seqs((size_t)n * cap.seq_cap); std::vector<u8> lits((size_t)n * cap.lit_cap, 0xEE); std::vector<KSliceMeta> meta(n);
    memset((void*)meta.data(), 0x6B, meta.size() * sizeof(KSliceMeta));          // (what an earlier batch might have left)
    std::vector<u32> scratch((size_t)n * cap.scratch_words, 0xA5A5A5A5u);
    KBatchView const v = { src, in_off, in_len, dst, out_off, out_len, n, seqs.data(), lits.data(), meta.data(), scratch.data(), cap };
    u32 status = 0, remaining = 0;
    if (!streaming) {
        // staged = in place up to 128 KiB: the one-block slices go through the kernels of zstd_lazy.h and the entropy kernel
        std::vector<u32> small_len(n);
        for (u32 i = 0; i < n; i++) small_len[i] = in_len[i] > KX_BLOCK_MAX ? 0u : in_len[i];
        KBatchView sv = v; sv.in_len = small_len.data();
        std::vector<KLazyRec> rec((size_t)n * cap.pos_cap); std::vector<u32> wr((size_t)n * cap.pos_cap, 0xDEADBEEFu);
        KLazyArgs const g = kx_lazy_args(sv, rec.data(), wr.data(), cap.pos_cap, level);
        kxemu::failed = 0;
        kxemu::launch_block(nblocks, 4, [&]() { zstd_lazy_sort_body(g); });
        if (kxemu::failed) return -1;
        kxemu::launch(nblocks, [&]() { zstd_lazy_body<4096>(g); });
        if (kxemu::failed) return -1;
        KEntropyArgs const e = kx_entropy_args(sv, kx_entropy_flags_lazy(level));
        kxemu::launch(nblocks, [&]() { zstd_entropy_body(e); });
        if (kxemu::failed) return -1;
    }
    // the chains of blocks, piece by piece over table slots full of what an earlier batch might have left
    u32 const slots = piece ? piece : (n ? n : 1u);
    u64 const slot_bytes = kx_lazy_big_slot_bytes_mode(slice_cap, level, mode);
    if (slot_bytes_out) *slot_bytes_out = slot_bytes;
    std::vector<u8> tables((size_t)slots * slot_bytes, 0x5Au);
    std::vector<KSeqPrev> prev(slots); memset((void*)prev.data(), 0x7F, prev.size() * sizeof(KSeqPrev));
    std::vector<KFrameState> fstate(n); std::vector<u32> hufct((size_t)n * 512, 0xDEADBEEFu);
    kxemu::failed = 0;
    for (u32 first = 0; first < n; first += slots) {
        u32 const m = n - first < slots ? n - first : slots;
        KBatchView const pv = v.sub(first, m);
        for (u32 i = 0; i < m; i++) {           // (k_zstd_lazy_big_init_modes)
            bool refused;
            zstd_lazy_big_init_slice(pv.in_len[i], fstate[first + i], prev[i], refused, mode);
            if (refused) { pv.out_len[i] = 0; status |= 4u; }
            else if (fstate[first + i].blockSize) remaining++;
            else if (streaming) pv.out_len[i] = zstd_lazy_big_empty_stream(pv.dst + pv.out_off[i], (u32)level);
        }
        KLazyBigArgs const g = kx_lazy_big_args(pv, fstate.data() + first, hufct.data() + (size_t)first * 512u, &remaining, &status, tables.data(), slot_bytes, prev.data(), level, mode, out_chunk);
        kxemu::launch(nblocks, [&]() { zstd_lazy_big_body<true>(g); });
        if (kxemu::failed) return -1;
    }
    for (u32 i = 0; i < n; i++) if (fstate[i].blockSize != 0) return -5;
    if (remaining != 0) return -6;
    // (k_len_guard_finish: a stream batch hands it no per-slice records -- a tripped guard is in the status word already)
    if (!streaming) for (u32 i = 0; i < n; i++) {
        if (meta[i].status == 3u) { out_len[i] = 0; status |= 4u; }
        else if (in_len[i] >= 8 && meta[i].status != 0) { out_len[i] = 0; status |= 2u; }
    }
    if (status_out) *status_out = status;
    return 0;
}

// the kernels' restatement of libzstd's parameters in a mode: windowLog, hashLog, searchLog, minMatch, strategy (0: not served)
extern "C" __attribute__((visibility("default")))
void emu_lazy_stream_params(int level, u32 n, u32 mode, u32* out5)
{
    KLazyBigPar const p = kx_lazy_big_params_mode((u32)level, n, mode);
    out5[0] = p.W; out5[1] = p.H; out5[2] = p.S; out5[3] = p.mml; out5[4] = p.strat;
}
