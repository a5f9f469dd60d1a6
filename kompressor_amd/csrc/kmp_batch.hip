// kmp_batch.hip -- the zstd half of libkompressor_hip.so's batched device API (include/kompressor_hip.h part 2): kernel entry
// points for gfx950, the batch context and its workspace, kmp_zstd_compress_batch* / kmp_zstd_decompress_batch*,
// kmp_compact_batch.  The DEFLATE half is kmp_deflate.hip, the streaming-compatible API kmp_stream.hip.
#include "kx_wave.h"
#include "zstd_match.h"
#ifdef KMP_ABLATIONS
#include "zstd_match2.h"
#endif
#include "zstd_launch.h"            // (the compress kernels' bodies and how their arguments are built)
#include "zstd_cdict_host.h"
#include "zstd_decode.h"
#include "zstd_predecode.h"
#include "zstd_frame_info.h"         // (frame inspection and the decode layout made of it)
#include "deflate_match.h"          // (KdBest & co.: the context frees the DEFLATE workspace)
#include "kmp_internal.h"

#include <mutex>
#include <new>
#include <thread>
#include <vector>

// entropy sweeps: K of a context unless KMP_ENTROPY_SWEEPS says otherwise (the ablation build), and the words in front of done[] in
// kmp_batch_ctx.sweep_rec: [0] the count the stream waits read, [1 + j] slices coded by sweep j.  K = 8: 201.9 ms a step against
// 202.3 at K = 4, 203.1 at K = 16 and 205.6 without sweeps (65 536 x 64 KiB, profiles/overlap_entropy.txt)
enum { KMP_SWEEPS_DEFAULT = 8, KMP_SWEEP_HEAD = 32 };
static_assert(KMP_SWEEP_HEAD > KX_MAX_SWEEPS + 1, "a counter per sweep, the final one included");

// --------------------------------------------------------------------------
// kernels (one 64-lane wave per workgroup everywhere)
// --------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(64) void k_zstd_match(KMatchArgs a) { zstd_match_body<G>(a); }
// Team width 4, the level-3 default: five waves' worth of registers per SIMD (<= 96 VGPRs each).  The launch itself puts four
// parse waves on a SIMD, so one wave of k_zstd_entropy (128 VGPRs) fits beside them: the entropy sweeps (zstd_compress_dfast)
template <>
__global__ __launch_bounds__(64, 5) void k_zstd_match<4>(KMatchArgs a) { zstd_match_body<4>(a); }
#ifdef KMP_ABLATIONS
// the same parse as a split-phase stage machine (zstd_match2.h): one memory round trip per outer iteration
template <int G, int R>
__global__ __launch_bounds__(64, 4) void k_zstd_match2(KMatchArgs a) { zstd_match2_body<G, R>(a); }
#endif
__global__ __launch_bounds__(64, 4) void k_zstd_entropy(KEntropyArgs a) { zstd_entropy_body(a); }
// zstd levels 5 .. 10 (greedy / lazy / lazy2: zstd_lazy.h)
__global__ __launch_bounds__(256) void k_zstd_lazy_sort(KLazyArgs a) { zstd_lazy_sort_body(a); }
template <int WORDS> __global__ __launch_bounds__(64, 2) void k_zstd_lazy(KLazyArgs a) { zstd_lazy_body<WORDS>(a); }
// ... above 128 KiB, up to 2 MiB: frames of several blocks, a wave walks a slice's chain of parse and frame step (zstd_lazy_big.h)
__global__ __launch_bounds__(64, 2) void k_zstd_lazy_big(KLazyBigArgs a) { zstd_lazy_big_body(a); }
// the lengths the one-block kernels of such a batch see: a slice above 128 KiB reads as empty there (its frame comes from k_zstd_lazy_big)
__global__ __launch_bounds__(256) void k_zstd_lazy_small_len(const u32* in_len, u32 n, u32* small_len)
{
    u32 const i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) { u32 const len = in_len[i]; small_len[i] = len > KX_BLOCK_MAX ? 0u : len; }
}
// k_zstd_frame_init's sibling: the frame states of the slices k_zstd_lazy_big takes; a slice above 2 MiB is refused (out_len 0, the status bit)
__global__ __launch_bounds__(256) void k_zstd_lazy_big_init(const u32* in_len, u32 n, KFrameState* fs, KSeqPrev* prev, u32* out_len, u32* remaining, u32* status)
{
    u32 const i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    KFrameState s; bool refused;
    zstd_lazy_big_init_slice(in_len[i], s, prev[i], refused);
    fs[i] = s;
    if (refused) { out_len[i] = 0; atomicOr(status, (u32)KMP_STATUS_LEVEL_SIZE); }
    else if (s.blockSize) atomicAdd(remaining, 1u);
}
// ... as streams or as the reference driver's staged frames (KFrameArgs.stream = KXF_STREAM / KXF_STREAM_EMPTY_END / KXF_REFERENCE): a kernel of
// its own, so that the one-shot kernel keeps its code
__global__ __launch_bounds__(64, 2) void k_zstd_lazy_big_modes(KLazyBigArgs a) { zstd_lazy_big_body<true>(a); }
// ... and its init: a stream is taken at every length (an empty one: its nine bytes are written here)
__global__ __launch_bounds__(256) void k_zstd_lazy_big_init_modes(const u32* in_len, u32 n, KFrameState* fs, KSeqPrev* prev, u8* dst, const u64* out_off, u32* out_len, u32* remaining, u32* status, u32 mode, u32 level, u32 fflags, const u32* cks)
{
    u32 const i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    KFrameState s; bool refused;
    zstd_lazy_big_init_slice(in_len[i], s, prev[i], refused, mode);
    fs[i] = s;
    if (refused) { out_len[i] = 0; atomicOr(status, (u32)KMP_STATUS_LEVEL_SIZE); }
    else if (s.blockSize) atomicAdd(remaining, 1u);
    else if (mode != KXF_REFERENCE) out_len[i] = kx_frame_end(dst + out_off[i], zstd_lazy_big_empty_stream(dst + out_off[i], level, fflags), fflags, cks, i);
}
// ... of a batch parsed against a formatted dictionary: its tables as the block's predecessor, its ID in the frame header
__global__ __launch_bounds__(64, 4) void k_zstd_entropy_prior(KEntropyArgs a) { zstd_entropy_body<true>(a); }
#ifdef KMP_ABLATIONS
// parse and entropy stage in one launch (zstd_entropy.h: zstd_l3_fused_body)
template <int G>
__global__ __launch_bounds__(64, 4) void k_zstd_l3_fused(KMatchArgs a, KEntropyArgs e) { zstd_l3_fused_body<G>(a, e); }
#endif
// levels 1 and 2 (strategy "fast")
template <int G>
__global__ __launch_bounds__(64) void k_zstd_match_fast(KFastArgs a) { zstd_match_fast_body<G>(a); }
// the parse when the context holds a raw-content dictionary
template <int G>
__global__ __launch_bounds__(64) void k_zstd_match_dict(KDictArgs a) { zstd_match_dict_body<G>(a); }
// ... at levels 1, 2 and the negative ones (strategy "fast")
template <int G>
__global__ __launch_bounds__(64) void k_zstd_match_fast_dict(KFastDictArgs a) { zstd_match_fast_dict_body<G>(a); }
#ifdef KMP_ABLATIONS
// frames of several blocks (slices above 128 KiB): one block of every unfinished slice per launch
template <int G>
__global__ __launch_bounds__(64) void k_zstd_match_blk(KMatchArgs a)
{
    zstd_match_body<G, true>(a);
    a.counter += 1;                          // second work queue: the blocks libzstd parses with the extDict variant
    zstd_match_ext_body<G>(a);
}
__global__ __launch_bounds__(64, 4) void k_zstd_frame(KFrameArgs a) { zstd_frame_body(a); }
#endif
// ... or the whole chain of blocks of a slice by one wave (no host rounds)
template <int G>
__global__ __launch_bounds__(64, 3) void k_zstd_big(KBigArgs a) { zstd_big_body<G>(a); }
template <int G>
__global__ __launch_bounds__(64, 3) void k_zstd_big_fast(KBigArgs a) { zstd_big_body<G, true>(a); }
// first block size, repcodes {1,4,8}, no Huffman table, a fresh window; an empty slice is a header and an empty raw block
// chunked: the input is taken in chunks of 128 KiB (KFrameArgs.stream != 0); wd: window descriptor byte of a streaming frame, 0 = one-shot
// level4: slices of the size classes level 4 runs as "greedy" (up to 16 KiB, 128 - 256 KiB; sizes known) get no frame here: out_len 0, and the
// status bit -- except, with level4 == 2, the class above a block, whose frames k_zstd_lazy_big writes behind this batch's chains
// fflags / cks: the batch's frame flags and checksums (zstd_common.h KXH_*), for the empty slices' frames
__global__ __launch_bounds__(256) void k_zstd_frame_init(const u32* in_len, u32 n, KFrameState* fs, u8* dst, const u64* out_off, u32* out_len, u32* remaining, u32 wd, u32 chunked, u32 level4, u32* status, u32 fflags, const u32* cks)
{
    u32 const i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    KFrameState s; u32 const len = in_len[i];
    if (level4 && !wd && !kx_l4_served(len)) {
        s.ipos = 0; s.opos = 0; s.blockSize = 0; s.first = 1; s.rep[0] = 1; s.rep[1] = 4; s.rep[2] = 8; s.hufValid = 0; s.hufSel = 0; s.savings = 0;
        s.lowLimit = 2; s.dictLimit = 2; s.bufPos = 0; s.extBase = 0; s.wflags = 0; s.chunkEnd = 0;
        // (level4 == 2, the one-shot batch call: the class above a block is not refused, k_zstd_lazy_big writes its frames behind this chain)
        fs[i] = s; out_len[i] = 0; if (status && !(level4 == 2u && len > KX_BLOCK_MAX)) atomicOr(status, (u32)KMP_STATUS_LEVEL_SIZE);
        return;
    }
    s.ipos = 0; s.opos = 0; s.blockSize = len < KX_BLOCK_MAX ? len : KX_BLOCK_MAX; s.first = 1;
    s.rep[0] = 1; s.rep[1] = 4; s.rep[2] = 8; s.hufValid = 0; s.hufSel = 0; s.savings = 0;
    s.lowLimit = 2; s.dictLimit = 2; s.bufPos = 0; s.extBase = 0; s.wflags = 0;
    s.chunkEnd = (chunked && len > KX_BLOCK_MAX) ? KX_BLOCK_MAX : len;
    fs[i] = s;
    if (len == 0) {
        u8* d = dst + out_off[i];
        if (wd) { kx_st32(d, 0xFD2FB528u); d[4] = (u8)((fflags & KXH_CHECKSUM) ? 1u << 2 : 0u); d[5] = (u8)wd; }
        else kx_write_frame_header(d, 0, kx_window_log_src(0), fflags);      // (six bytes either way: a content size of 0, or the smallest window)
        d[6] = 1; d[7] = 0; d[8] = 0; out_len[i] = kx_frame_end(d, 9, fflags, cks, i);
    }
    else atomicAdd(remaining, 1u);
}
// level 4's "greedy" class above a block (128 KiB < size <= 256 KiB), behind k_zstd_big: the frame states of those slices for
// k_zstd_lazy_big at level 4 (kx_lazy_big_params_l4); every other slice's frame is written already and k_zstd_lazy_big passes it over
__global__ __launch_bounds__(256) void k_zstd_lazy_big_init_l4(const u32* in_len, u32 n, KFrameState* fs, KSeqPrev* prev, u32* remaining)
{
    u32 const i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    KFrameState s; bool refused; u32 const len = in_len[i];
    zstd_lazy_big_init_slice(len, s, prev[i], refused);
    if (kx_lazy_big_params_l4(len).strat == 0u) s.blockSize = 0;
    fs[i] = s;
    if (s.blockSize) atomicAdd(remaining, 1u);
}
// XXH64 of every slice of a batch whose frames carry checksums (zstd_seekable.h's body, as the seekable container runs it)
__global__ __launch_bounds__(256) void k_frame_xxh64(KSeekXxhArgs a) { seekable_xxh64_body(a); }
__global__ __launch_bounds__(64, 5) void k_zstd_decode(KDecodeArgs a) { zstd_decode_body(a); }
// the sequence bitstreams decoded ahead of it, one lane per frame (FSE tables in HBM)
__global__ __launch_bounds__(4 * KXP_FRAMES) void k_zstd_seq_predecode(KPreArgs a) { zstd_seq_predecode_body(a); }
// ... and the Huffman-coded literals, one lane per stream (32 frames per workgroup of 128 threads)
__global__ __launch_bounds__(64) void k_zstd_lit_predecode(KLitArgs a) { zstd_lit_predecode_body(a); }
__global__ __launch_bounds__(256) void k_zstd_seq_count(KSeqSortArgs a) { zstd_seq_count_body(a); }
__global__ __launch_bounds__(256) void k_zstd_seq_rank(KSeqSortArgs a) { zstd_seq_rank_body(a); }
__global__ __launch_bounds__(256) void k_zstd_seq_perm(KSeqSortArgs a) { zstd_seq_perm_body(a); }
// what each entry's frames declare, a lane per entry; capacities and offsets of a decode made of it, one workgroup
__global__ __launch_bounds__(256) void k_zstd_frame_info(KFrameInfoArgs a) { zstd_frame_info_body(a); }
__global__ __launch_bounds__(64 * KFI_LAYOUT_WAVES) void k_batch_layout(KLayoutArgs a) { batch_layout_body(a); }
// exclusive prefix sum of u32 lengths into u64 offsets, single workgroup
__global__ __launch_bounds__(1024) void k_scan_lengths(const u32* len, u32 n, u64* off)
{
    __shared__ u64 part[1024];
    u32 const t = threadIdx.x;
    u32 const per = (n + 1023) / 1024;
    u32 const b = t * per, e = (b + per < n) ? b + per : n;
    u64 s = 0;
    for (u32 i = b; i < e; i++) s += len[i];
    part[t] = s;
    __syncthreads();
    for (u32 o = 1; o < 1024; o <<= 1) {
        u64 v = (t >= o) ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    u64 run = (t == 0) ? 0 : part[t - 1];
    for (u32 i = b; i < e; i++) { off[i] = run; run += len[i]; }
    if (t == 1023) off[n] = part[1023];
}
// one wave per frame, 16 B per lane per step when both sides allow it
__global__ __launch_bounds__(64) void k_compact(const u8* src, const u64* in_off, const u32* len, u32 n, u8* dst, const u64* out_off)
{
    int const lane = threadIdx.x;
    for (u32 it = blockIdx.x; it < n; it += gridDim.x) {
        u32 const i = kx_xcd_chunk(it, n);                  // (frame sizes follow the content's period too: zstd_common.h)
        const u8* s = src + in_off[i]; u8* d = dst + out_off[i]; u32 const L = len[i];
        u32 k = (u32)lane * 8u;
        for (; k + 8 <= L; k += 512u) kx_st64(d + k, kx_ld64(s + k));
        u32 const tail = L & ~7u;
        if (lane < (int)(L - tail)) d[tail + lane] = s[tail + lane];
    }
}

// Per-slice lengths live on the device, so the host cannot check them against the workspace before it launches.
// Every batch entry point therefore runs its kernels on a sanitised copy: a slice longer than the context (or the
// codec) holds is processed as an empty one, then loses its frame again (out_len = 0: a real frame is never empty) and
// raises the context's status word, which kmp_batch_status hands to the host.
__global__ __launch_bounds__(256) void k_len_guard(const u32* in_len, u32 n, u32 cap, u32* len_ok, u32* status)
{
    u32 const i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    u32 const len = in_len[i];
    len_ok[i] = len > cap ? 0u : len;
    if (len > cap) atomicOr(status, (u32)KMP_STATUS_SLICE_TOO_LARGE);
}
__global__ void k_status_take(u32* status, u32* out) { *out = atomicExch(status, 0u); }
// meta: the one-block zstd parsers' per-slice record (a tripped loop guard there also voids the frame), or null
__global__ __launch_bounds__(256) void k_len_guard_finish(const u32* in_len, u32 n, u32 cap, u32* out_len, const KSliceMeta* meta, u32* status)
{
    u32 const i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (in_len[i] > cap) out_len[i] = 0;
    else if (meta && meta[i].status == 3u) { out_len[i] = 0; atomicOr(status, (u32)KMP_STATUS_LEVEL_SIZE); }
    else if (meta && in_len[i] >= 8 && meta[i].status != 0) { out_len[i] = 0; atomicOr(status, (u32)KMP_STATUS_KERNEL_GUARD); }
}

// --------------------------------------------------------------------------
// errors
// --------------------------------------------------------------------------
thread_local std::string g_last_error;
int hip_fail(hipError_t e, const char* what)
{
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return KMP_ERR_HIP;
}

extern "C" const char* kmp_last_error(void) { return g_last_error.c_str(); }

// Random 4-byte read-modify-writes over a region, the way the level-3 parser touches its tables: how fast is THIS piece
// of HBM?  (The rate differs by a sixth between regions of one device: DESIGN.md section 5a; tools/region_probe.py.)
__global__ __launch_bounds__(256) void k_region_probe(u32* p, u64 words, u32 iters, u32 salt)
{
    u64 x = ((u64)blockIdx.x * 256u + threadIdx.x) * 0x9E3779B97F4A7C15ull + salt;
    u32 acc = 0;
    for (u32 i = 0; i < iters; i++) {
        x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
        u64 const w = x % words;
        u32 const v = kx_ld_nt(p + w);
        acc += v;
        kx_st_nt(p + ((w * 2654435761ull + 12345u) % words), v + i);
    }
    if (acc == 0x12345678u) p[0] = acc;
}
// milliseconds for blocks x 256 threads x iters random read + write pairs over [p, p + bytes)
extern "C" int kmp_debug_probe_region(void* p, size_t bytes, uint32_t blocks, uint32_t iters, float* ms, void* hip_stream)
{
    if (!p || bytes < 4096 || !ms) { g_last_error = "kmp_debug_probe_region: bad argument"; return KMP_ERR_ARG; }
    hipStream_t const st = (hipStream_t)hip_stream;
    hip_event e0, e1; KMP_TRY(e0.create(hipEventDefault)); KMP_TRY(e1.create(hipEventDefault));
    hipLaunchKernelGGL(k_region_probe, dim3(blocks), dim3(256), 0, st, (u32*)p, (u64)(bytes / 4), 8u, 1u);       // warm
    HIP_TRY(hipEventRecord(e0, st));
    hipLaunchKernelGGL(k_region_probe, dim3(blocks), dim3(256), 0, st, (u32*)p, (u64)(bytes / 4), iters, 7u);
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipEventSynchronize(e1));
    HIP_TRY(hipEventElapsedTime(ms, e0, e1));
    return KMP_OK;
}
// What the memory system gives the level-3 parser's tables WHERE THEY LIE: random accesses over the context's table pieces,
// four independent chains per lane, 16 waves per CU.  mode 0: 4-byte loads (a probe that inserts nothing); mode 1: a load
// and a store into the same word (a probe + insert: the line comes in and goes back).  Run once when a context with large
// tables is created, before the tables are zeroed; bench.py prices the parser's measured memory requests with the two rates
// (DESIGN.md section 4.1).
__global__ __launch_bounds__(64) void k_table_probe(u32* p0, u32* p1, u32* p2, u32* p3, u32 pieces, u64 words, u32 iters, u32 mode, u32* sink)
{
    u64 s[4]; u32 acc = 0;
    u64 const gid = (u64)blockIdx.x * 64 + threadIdx.x;
    for (int j = 0; j < 4; j++) s[j] = (gid * 4 + j) * 0x9E3779B97F4A7C15ull + 12345;
    for (u32 i = 0; i < iters; i++) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            s[j] = s[j] * 6364136223846793005ull + 1442695040888963407ull;
            u64 const r = s[j] >> 11;
            u32 const pc = pieces == 4 ? (u32)(r & 3) : 0u;
            u32* const base = pc == 0 ? p0 : pc == 1 ? p1 : pc == 2 ? p2 : p3;
            u32* const q = base + __umul64hi(r << 11, words);
            u32 v = *q;
            if (mode) kx_st_nt(q, v + 1);
            acc += v; s[j] += v & 1;
        }
    }
    if (acc == 0x12345678u) sink[0] = acc;
}
extern "C" const char* kmp_version(void) { return "kompressor_hip 0.5 (gfx950; zstd levels -131072 .. -1 and 1 .. 3: frames and streams up to 1 GiB, dictionaries (raw content and zstd format) at all of these levels up to 128 KiB; level 4 up to 128 KiB, above 256 KiB and streams; levels 5 .. 10 up to 2 MiB (one-shot and staged frames, streams); deflate / zlib / gzip levels 1-9, windowBits 9-15, memLevel 1-9; zstd and inflate decoders; zstd seekable containers: levels -131072 .. 8, frames up to 128 KiB, range reads)"; }

u32 env_u32(const char* name, u32 dflt)
{
    const char* v = getenv(name);
    return (v && *v) ? (u32)strtoul(v, nullptr, 10) : dflt;
}

// Where a randomly accessed table lands matters a little: read + insert pairs confined to a few dozen GiB of this device's HBM
// run at 20 G/s, over a span of 72 GiB or more at 26 (tools/spanprobe, profiles/r03_match_floor.txt).  The level-3 team tables
// get their span from the context's arena (kmp_batch_create); for the other large tables a placement by trial is available
// as an option: with KMP_PLACE_TRIES = 2 .. 8 that many allocations are probed with the tables' access pattern
// (k_region_probe, ~30 ms each) until one is of the fast kind, the fastest stays, the others are freed.  The default is one
// plain allocation: the candidates of a trial are held until the choice is made, and a library must not take that much
// memory behind its caller's back.
static int place_alloc(dev_buf<u32>& out, size_t bytes, float* kept_ms, u32* tried_out)
{
    u32 tries = KMP_KNOB("KMP_PLACE_TRIES", 1); if (tries < 1) tries = 1; if (tries > 8) tries = 8;
    if (bytes < ((size_t)4 << 30)) tries = 1;
    dev_buf<u32> cand[8]; float ms[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    u32 got = 0, best = 0;
    for (u32 t = 0; t < tries; t++) {
        if (cand[t].alloc(bytes) != KMP_OK) break;
        got = t + 1;
        if (tries > 1 && kmp_debug_probe_region(cand[t], bytes, 4096u, 384u, &ms[t], nullptr) != KMP_OK) ms[t] = 1e30f;
        if (ms[t] < ms[best]) best = t;
        // 805 M accesses: the fast kind of region takes 23.5 ms (34 G/s), the slow kind 29.2 (27.6 G/s) on an MI355X
        if (ms[t] <= 26.0f) break;
    }
    if (got == 0) return hip_fail(hipErrorOutOfMemory, "hipMalloc(parser tables)");
    if (env_u32("KMP_VERBOSE", 0)) { fprintf(stderr, "place_alloc %zu MiB:", bytes >> 20); for (u32 t = 0; t < got; t++) fprintf(stderr, " %.1f ms%s", ms[t], t == best ? "*" : ""); fprintf(stderr, "\n"); }
    for (u32 t = 0; t < got; t++) if (t != best) cand[t].reset();
    out = std::move(cand[best]);
    if (kept_ms) *kept_ms = ms[best];
    if (tried_out) *tried_out = got;
    return KMP_OK;
}

struct create_opts { int span_gib; int retry; };          // -1 = the environment's / the default
static int batch_create_body(kmp_batch_ctx* c, int device, uint32_t max_slices, uint32_t max_slice_bytes, int team_lanes, create_opts const& o);
static int batch_create_with(kmp_batch_ctx** out, int device, uint32_t max_slices, uint32_t max_slice_bytes, int team_lanes, create_opts const& o)
{
    if (!out || max_slices == 0) { g_last_error = "kmp_batch_create: bad argument"; return KMP_ERR_ARG; }
    if (max_slice_bytes > KMP_MAX_BIG_SLICE_BYTES) { g_last_error = "kmp_batch_create: slices above 1 GiB are not supported"; return KMP_ERR_CAPACITY; }
    int const team_fixed = (team_lanes != 0 || getenv("KMP_TEAM_LANES")) ? 1 : 0;
    if (team_lanes == 0) team_lanes = (int)env_u32("KMP_TEAM_LANES", 4);
    if (team_lanes != 2 && team_lanes != 4 && team_lanes != 8 && team_lanes != 16 && team_lanes != 32 && team_lanes != 64) { g_last_error = "team_lanes must be 2, 4, 8, 16, 32 or 64"; return KMP_ERR_ARG; }
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<kmp_batch_ctx> c(new (std::nothrow) kmp_batch_ctx());
    if (!c) { g_last_error = "out of host memory"; return KMP_ERR_ARG; }
    c->team_fixed = team_fixed;
    KMP_TRY(batch_create_body(c.get(), device, max_slices, max_slice_bytes, team_lanes, o));      // (nothing half-built is left behind)
    *out = c.release();
    return KMP_OK;
}
extern "C" int kmp_batch_create(kmp_batch_ctx** out, int device, uint32_t max_slices, uint32_t max_slice_bytes, int team_lanes)
{
    create_opts const o = { -1, -1 };
    return batch_create_with(out, device, max_slices, max_slice_bytes, team_lanes, o);
}
extern "C" int kmp_batch_create_ex(kmp_batch_ctx** out, int device, uint32_t max_slices, uint32_t max_slice_bytes, const kmp_batch_options* opts)
{
    if (!opts || opts->struct_bytes < sizeof(kmp_batch_options)) { g_last_error = "kmp_batch_create_ex: options missing or of another version"; return KMP_ERR_ARG; }
    create_opts const o = { opts->table_span_gib, opts->table_retry };
    return batch_create_with(out, device, max_slices, max_slice_bytes, opts->team_lanes, o);
}
// a context whose arena is packed (the engines of the host-memory batch: kmp_coalesce.h)
int batch_create_packed(kmp_batch_ctx** out, int device, uint32_t max_slices, uint32_t max_slice_bytes)
{
    create_opts const o = { 0, 0 };
    return batch_create_with(out, device, max_slices, max_slice_bytes, 0, o);
}
static int batch_create_body(kmp_batch_ctx* c, int device, uint32_t max_slices, uint32_t max_slice_bytes, int team_lanes, create_opts const& o)
{
    c->device = device; c->max_slices = max_slices; c->max_slice_bytes = max_slice_bytes < 64 ? 64 : max_slice_bytes; c->G = team_lanes;
    hipDeviceProp_t prop; HIP_TRY(hipGetDeviceProperties(&prop, device));
    // the context's own stream: the second stream of its pipelines, and where creation's probes and clears run (non-blocking:
    // nothing here serialises with the caller's streams, the NULL stream included)
    KMP_TRY(c->st2.create(hipStreamNonBlocking));
    u32 const waves_per_cu = KMP_KNOB("KMP_MATCH_WAVES_PER_CU", 16);     // 16 x 16 teams x 256 CUs = 65 536 slices in flight at team width 4
    u32 const teams_per_wave = 64 / (u32)team_lanes;
    u32 blocks = (u32)prop.multiProcessorCount * waves_per_cu;
    u32 const need = (max_slices + teams_per_wave - 1) / teams_per_wave;
    if (blocks > need) blocks = need;
    c->match_blocks = blocks; c->nteams = blocks * teams_per_wave;
    // Every parser wants every slice in flight: 16 waves per CU.  (The level-3 parser ran with 12 for most of two rounds --
    // 49 152 team slots, a 65 536-slice batch in two launches with the entropy kernel of the first beside the second: 251 ms.
    // That optimum belonged to an entropy kernel that was a third slower than it had to be (zstd_common.h kx_xcd_chunk);
    // with it fixed, one launch of each kernel at 16 waves per CU takes 191 + 27 ms.)
    { u32 const l3 = (u32)prop.multiProcessorCount * KMP_KNOB("KMP_MATCH_WAVES_PER_CU_L3", 16); c->match_blocks_l3 = l3 < blocks ? l3 : blocks; c->l3_team_slots = l3 * teams_per_wave; }
    c->big = c->max_slice_bytes > KMP_MAX_SLICE_BYTES;
    u32 const block_cap = c->big ? KMP_MAX_SLICE_BYTES : c->max_slice_bytes;     // the sequence / literal workspaces hold one block
    { KWorkCaps const w = kx_work_caps(block_cap); c->seq_cap = w.seq_cap; c->lit_cap = w.lit_cap; c->scratch_words = w.scratch_words; }
    size_t const ns = max_slices;
    if (c->big) {
        c->big_G = (int)KMP_KNOB("KMP_BIG_TEAM_LANES", 0);      // 0 = by batch size (zstd_compress_big)
        if (c->big_G != 0 && c->big_G != 2 && c->big_G != 4 && c->big_G != 8 && c->big_G != 16 && c->big_G != 32 && c->big_G != 64) c->big_G = 0;
        KMP_TRY(c->fstate.alloc(ns * sizeof(KFrameState), "hipMalloc(frame states)"));
        KMP_TRY(c->hufct.alloc(ns * 512 * sizeof(u32), "hipMalloc(Huffman tables)"));
        KMP_TRY(place_alloc(c->big_tables, ns * KX_BIG_TBL_ENTRIES * sizeof(u32), nullptr, nullptr));     // (the block-chain parser's tables: the same access pattern)
        KMP_TRY(c->remaining.alloc(64, "hipMalloc(open frames)"));
        KMP_TRY(c->big_counters.alloc(ns * 4, "hipMalloc(block-chain counters)"));
    }
    {
        // The workspace of a context with large team tables is ONE allocation (an arena): the tables in four pieces (team t:
        // piece t & 3) with the sequence, literal and staging buffers between them, laid out over a span of
        // KMP_TABLE_SPAN_GIB / kmp_batch_options.table_span_gib (default 100) GiB.  Why a span: read + insert pairs run a quarter
        // faster when they straddle the coarse blocks this device's HBM is laid out in -- 20 G pairs/s inside any 24 .. 36 GiB,
        // 25 - 26 from 72 GiB of span on (tools/spanprobe, profiles/r03_match_floor.txt) -- and the parser lives on that rate:
        // the same context takes 205 ms per batch with its 41 GiB packed, 183 - 190 over 100 - 140 GiB on every box tried.
        // The gaps between the parts are memory the context holds and does not use (59 GiB of a 65 536-slice context's 100), so
        // the span is BOUNDED: never more than half of what the device has free when the context is created (a second context,
        // the caller's own buffers and the host engines must still fit: ADVICE r3); below the parts' own size the arena is
        // packed.  Span 0 packs it (memory over ~11 % of parser time).  kmp_batch_memory reports what the context holds.
        // A second arena is tried only on request (KMP_TABLE_RETRY=1 / table_retry: when the first measures slow whatever the
        // layout -- some allocations land on slower memory, 212 ms instead of 189 -- and the device has room for both; one of
        // the two is freed before creation returns).  That is the one transient allocation creation can make, hence opt-in;
        // bench.py asks for it and says so in its line.
        size_t const tbytes = (size_t)c->nteams * KX_TBL_ENTRIES * sizeof(u32);
        size_t const A = (size_t)2 << 20;                                // every part starts on a 2 MiB boundary
        auto up = [&](size_t v) { return (v + A - 1) & ~(A - 1); };
        size_t const seqs_b = up(ns * c->seq_cap * sizeof(KSeq)), lits_b = up(ns * c->lit_cap), meta_b = up(ns * sizeof(KSliceMeta)), scr_b = up(ns * c->scratch_words * sizeof(u32));
        c->tseg_n = 1;
        if (KMP_KNOB("KMP_TABLE_ARENA", 1) && tbytes >= ((size_t)4 << 30) && (c->nteams & 3u) == 0) {
            size_t const piece = up(tbytes / 4);
            size_t const need = 4 * piece + seqs_b + lits_b + meta_b + scr_b;
            size_t want = (size_t)(o.span_gib >= 0 ? (u32)o.span_gib : env_u32("KMP_TABLE_SPAN_GIB", 100)) << 30;
            size_t fr = 0, tot = 0;
            if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = 0;
            if (want > fr / 2) want = fr / 2;                               // bounded: at most half of the free memory
            if (want > need && fr < want + ((size_t)16 << 30)) want = 0;    // not that much room: pack
            size_t const gap = want > need ? ((want - need) / 3) & ~(A - 1) : 0;     // unused bytes behind each of the three buffers between the pieces (rounded down: the span is a bound)
            size_t const total = need + 3 * gap;
            if (fr > total + ((size_t)1 << 30) && c->arena.alloc(total) == KMP_OK) {
                // Where in the arena the four pieces go is chosen by measurement, inside the arena (nothing else is allocated):
                // up to eight layouts are probed with the tables' own traffic (k_table_probe, read + insert pairs, ~12 ms each) and
                // the fastest stays.  Which physical blocks of the HBM an offset of the arena falls into differs from process to
                // process: with one fixed layout the same box gave 21.6 and 24.9 G pairs/s (parser 213 and 196 ms) in two runs
                // a minute apart.  KMP_TABLE_LAYOUT = 1 .. 8 fixes a layout (1: two pieces at either end; 2: evenly spread;
                // 3: the ends moved inwards by an eighth; 4: the second and third quarter; 5 .. 8: below).  The other buffers fill the space
                // the pieces leave.
                size_t const slackT = total - 4 * piece;                                   // bytes that are not table
                size_t lay[8][4]; u32 nlay = 0;
                // (a layout counts only if its pieces do not overlap and the other buffers fit into what it leaves free)
                auto fits = [&](const size_t* o, KSeq** ps, u8** pl, KSliceMeta** pm, u32** pc) -> bool {
                    size_t fs_[5], fe_[5]; u32 nf = 0; size_t cur = 0;
                    for (int i = 0; i < 4; i++) { if (o[i] < cur || o[i] + piece > total) return false; if (o[i] > cur) { fs_[nf] = cur; fe_[nf] = o[i]; nf++; } cur = o[i] + piece; }
                    if (cur < total) { fs_[nf] = cur; fe_[nf] = total; nf++; }
                    auto take = [&](size_t bytes) -> u8* { for (u32 f = 0; f < nf; f++) if (fe_[f] - fs_[f] >= bytes) { u8* const r = c->arena + fs_[f]; fs_[f] += bytes; return r; } return nullptr; };
                    u8* const a0 = take(seqs_b); u8* const a1 = take(lits_b); u8* const a2 = take(meta_b); u8* const a3 = take(scr_b);
                    if (!a0 || !a1 || !a2 || !a3) return false;
                    if (ps) { *ps = (KSeq*)a0; *pl = a1; *pm = (KSliceMeta*)a2; *pc = (u32*)a3; }
                    return true;
                };
                auto add = [&](size_t o0, size_t o1, size_t o2, size_t o3) {
                    size_t const o[4] = { o0 & ~(A - 1), o1 & ~(A - 1), o2 & ~(A - 1), o3 & ~(A - 1) };
                    if (!fits(o, nullptr, nullptr, nullptr, nullptr)) return;
                    for (int i = 0; i < 4; i++) lay[nlay][i] = o[i];
                    nlay++;
                };
                add(0, piece, total - 2 * piece, total - piece);
                if (gap) {
                    add(0, up(slackT / 3) + piece, 2 * up(slackT / 3) + 2 * piece, total - piece);
                    add(up(total / 8), up(total / 8) + piece, total - 2 * piece - up(total / 8), total - piece - up(total / 8));
                    add(up(total / 4), up(total / 4) + piece, total - 2 * piece - up(total / 4), total - piece - up(total / 4));
                    add(0, up(total / 2) - piece, up(total / 2), total - piece);                                    // 5: the ends and the middle
                    add(up(total / 16), up(total / 16) + piece, total - 2 * piece - up(total / 16), total - piece - up(total / 16));
                    add(up(total / 16 * 3), up(total / 16 * 3) + piece, total - 2 * piece - up(total / 16 * 3), total - piece - up(total / 16 * 3));
                    add(up(total / 16), up(total / 16 * 5), up(total / 16 * 9), up(total / 16 * 13));               // 8: one piece in every quarter
                }
                u32 pick = 0;
                u32 const fixed = KMP_KNOB("KMP_TABLE_LAYOUT", 0);
                // probes every layout on the arena at `base`: the fastest one (priced with the parser's own mix) and its pair rate
                auto probe_arena = [&](u8* base, u32* best_l, float* best_ms, float* best_pairs) -> int {
                    hip_event e[3];
                    for (int i = 0; i < 3; i++) KMP_TRY(e[i].create(hipEventDefault));
                    u64 const words = (u64)(piece / 4); u32 const pb = (u32)prop.multiProcessorCount * 16u;
                    int rc = KMP_OK; *best_ms = 1e30f; *best_l = 0; *best_pairs = 0;
                    for (u32 l = 0; l < nlay && rc == KMP_OK; l++) {
                        u32* t[4]; for (int i = 0; i < 4; i++) t[i] = (u32*)(base + lay[l][i]);
                        hipLaunchKernelGGL(k_table_probe, dim3(pb), dim3(64), 0, c->st2, t[0], t[1], t[2], t[3], 4u, words, 4u, 1u, t[0]);       // warm (TLB)
                        bool ok = hipEventRecord(e[0], c->st2) == hipSuccess;
                        hipLaunchKernelGGL(k_table_probe, dim3(pb), dim3(64), 0, c->st2, t[0], t[1], t[2], t[3], 4u, words, 96u, 1u, t[0]);
                        ok = ok && hipEventRecord(e[1], c->st2) == hipSuccess;
                        hipLaunchKernelGGL(k_table_probe, dim3(pb), dim3(64), 0, c->st2, t[0], t[1], t[2], t[3], 4u, words, 96u, 0u, t[0]);
                        ok = ok && hipEventRecord(e[2], c->st2) == hipSuccess && hipEventSynchronize(e[2]) == hipSuccess;
                        float msp = 0, msr = 0;
                        ok = ok && hipEventElapsedTime(&msp, e[0], e[1]) == hipSuccess && hipEventElapsedTime(&msr, e[1], e[2]) == hipSuccess;
                        if (!ok) { g_last_error = "kmp_batch_create: probing the arena failed"; rc = KMP_ERR_HIP; break; }
                        // the parser's own mix: per batch 3.97 G probe + insert pairs and 1.80 G reads that insert nothing (profiles/pmc_latest.json)
                        float const ms = 3.97f * msp + 1.80f * msr;
                        float const pairs = (float)((double)pb * 64.0 * 96.0 * 4.0 / (msp * 1e-3));
                        if (env_u32("KMP_VERBOSE", 0)) fprintf(stderr, "arena %p layout %u: %.1f G pairs/s, %.1f G reads/s\n", (void*)base, l + 1, pairs / 1e9, (double)pb * 64.0 * 96.0 * 4.0 / (msr * 1e-3) / 1e9);
                        if (ms < *best_ms) { *best_ms = ms; *best_l = l; *best_pairs = pairs; }
                    }
                    return rc;
                };
                if (fixed >= 1 && fixed <= nlay) pick = fixed - 1;
                else if (nlay > 1) {
                    float ms1 = 0, pr1 = 0;
                    { int const rc = probe_arena(c->arena, &pick, &ms1, &pr1); if (rc != KMP_OK) return rc; }
                    // Some allocations are slow whatever the layout (one box: every second process, 21.7 G pairs/s at best against
                    // 25; the parser then takes 212 ms instead of 189 -- which physical memory the allocator hands out is not ours to
                    // choose).  On request (table_retry / KMP_TABLE_RETRY = 1), when that happens and the device has room for a second
                    // arena beside the first, ONE more is allocated and probed, the faster of the two stays and the other is freed
                    // before creation returns (0: never, the default; 2: always, for the tests).
                    size_t fr2 = 0, tot2 = 0;
                    u32 const retry = o.retry >= 0 ? (u32)o.retry : env_u32("KMP_TABLE_RETRY", 0);     // 0 never (the default), 1 when slow, 2 always (tests)
                    if ((pr1 < (float)KMP_KNOB("KMP_TABLE_RETRY_BELOW", 235) * 1e8f || retry == 2) && retry && hipMemGetInfo(&fr2, &tot2) == hipSuccess && fr2 > total + ((size_t)16 << 30)) {
                        dev_buf<u8> second;
                        if (second.alloc(total) == KMP_OK) {
                            u32 pick2 = 0; float ms2 = 0, pr2 = 0;
                            KMP_TRY(probe_arena(second, &pick2, &ms2, &pr2));
                            if (env_u32("KMP_VERBOSE", 0)) fprintf(stderr, "arena retry: %.1f -> %.1f G pairs/s\n", pr1 / 1e9, pr2 / 1e9);
                            if (ms2 < ms1 * 0.98f) { c->arena.reset(); c->arena = std::move(second); pick = pick2; c->table_retry = 2; }
                            else { second.reset(); c->table_retry = 1; }
                        }
                    }
                }
                c->table_layout = pick + 1;
                for (int i = 0; i < 4; i++) c->tseg[i] = (u32*)(c->arena + lay[pick][i]);
                // the other buffers: first fit into what the pieces leave free
                if (nlay == 0 || !fits(lay[pick], &c->seqs, &c->lits, &c->meta, &c->scratch)) { g_last_error = "kmp_batch_create: arena layout failed"; return KMP_ERR_ARG; }
                c->tseg_n = 4; c->tables = c->tseg[0];
            } else (void)hipGetLastError();
        }
        if (!c->arena) {
            KMP_TRY(c->seqs_buf.alloc(ns * c->seq_cap * sizeof(KSeq), "hipMalloc(sequences)")); c->seqs = c->seqs_buf;
            KMP_TRY(c->lits_buf.alloc(ns * c->lit_cap, "hipMalloc(literals)")); c->lits = c->lits_buf;
            KMP_TRY(c->meta_buf.alloc(ns * sizeof(KSliceMeta), "hipMalloc(slice records)")); c->meta = c->meta_buf;
            KMP_TRY(c->scratch_buf.alloc(ns * c->scratch_words * sizeof(u32), "hipMalloc(scratch)")); c->scratch = c->scratch_buf;
            KMP_TRY(place_alloc(c->tables_buf, tbytes, &c->place_ms, &c->place_tried));
            c->tables = c->tseg[0] = c->tables_buf;
        }
    }
    KMP_TRY(c->team_epoch.alloc((size_t)c->nteams * sizeof(u32), "hipMalloc(team epochs)"));
    KMP_TRY(c->counter.alloc(64, "hipMalloc(work counters)"));
    if ((size_t)c->nteams * KX_TBL_ENTRIES * sizeof(u32) >= ((size_t)4 << 30) && KMP_KNOB("KMP_TABLE_PROBE", 1)) {
        // ~40 ms: the two rates the parser lives on, measured on these very tables (they are zeroed right below)
        hip_event e[3]; for (int i = 0; i < 3; i++) KMP_TRY(e[i].create(hipEventDefault));
        u64 const words = (u64)c->nteams * KX_TBL_ENTRIES / c->tseg_n; u32 const blocks = (u32)prop.multiProcessorCount * 16u, iters = 96u;
        u32* const t1 = c->tseg_n == 4 ? c->tseg[1] : c->tseg[0]; u32* const t2 = c->tseg_n == 4 ? c->tseg[2] : c->tseg[0]; u32* const t3 = c->tseg_n == 4 ? c->tseg[3] : c->tseg[0];
        hipLaunchKernelGGL(k_table_probe, dim3(blocks), dim3(64), 0, c->st2, c->tseg[0], t1, t2, t3, c->tseg_n, words, 8u, 1u, c->counter);     // warm (TLB)
        HIP_TRY(hipEventRecord(e[0], c->st2));
        hipLaunchKernelGGL(k_table_probe, dim3(blocks), dim3(64), 0, c->st2, c->tseg[0], t1, t2, t3, c->tseg_n, words, iters, 0u, c->counter);
        HIP_TRY(hipEventRecord(e[1], c->st2));
        hipLaunchKernelGGL(k_table_probe, dim3(blocks), dim3(64), 0, c->st2, c->tseg[0], t1, t2, t3, c->tseg_n, words, iters, 1u, c->counter);
        HIP_TRY(hipEventRecord(e[2], c->st2));
        HIP_TRY(hipEventSynchronize(e[2]));
        float ms0 = 0, ms1 = 0; HIP_TRY(hipEventElapsedTime(&ms0, e[0], e[1])); HIP_TRY(hipEventElapsedTime(&ms1, e[1], e[2]));
        double const ops = (double)blocks * 64.0 * iters * 4.0;
        if (ms0 > 0) c->table_reads_per_s = (float)(ops / (ms0 * 1e-3));
        if (ms1 > 0) c->table_pairs_per_s = (float)(ops / (ms1 * 1e-3));
    }
    for (u32 i = 0; i < c->tseg_n; i++) HIP_TRY(hipMemsetAsync(c->tseg[i], 0, (size_t)c->nteams * KX_TBL_ENTRIES * sizeof(u32) / c->tseg_n, c->st2));
    HIP_TRY(hipMemsetAsync(c->team_epoch, 0, (size_t)c->nteams * sizeof(u32), c->st2));
    HIP_TRY(hipMemsetAsync(c->meta, 0, ns * sizeof(KSliceMeta), c->st2));
    for (kmp_span* t : { &c->decode_t, &c->deflate_t, &c->tune }) { KMP_TRY(t->start.create(hipEventDefault)); KMP_TRY(t->end.create(hipEventDefault)); }
    for (hip_event* e : { &c->dfl_mark.chains, &c->dfl_mark.best, &c->dfl_mark.best_done, &c->dfl_mark.parse, &c->dfl_mark.encode, &c->dfl_mark.encode_done }) KMP_TRY(e->create(hipEventDefault));
    for (int i = 0; i < KMP_MAX_CHUNKS; i++) for (kmp_span* t : { &c->match[i], &c->entropy[i] }) { KMP_TRY(t->start.create(hipEventDefault)); KMP_TRY(t->end.create(hipEventDefault)); }
    KMP_TRY(c->ev_join.create(hipEventDisableTiming));
    KMP_TRY(c->ev_done.create(hipEventDisableTiming));
    for (int i = 0; i < KMP_MAX_PIECES; i++) KMP_TRY(c->ev_piece[i].create(hipEventDisableTiming));
    for (int i = 0; i <= KMP_MAX_CHUNKS; i++) KMP_TRY(c->ev_pre[i].create(hipEventDisableTiming));
    c->cus = (u32)prop.multiProcessorCount;
    KMP_TRY(c->len_ok.alloc(ns * sizeof(u32), "hipMalloc(slice lengths)"));
    KMP_TRY(c->d_status.alloc(64, "hipMalloc(status word)"));
    HIP_TRY(hipMemsetAsync(c->d_status, 0, 64, c->st2));
    c->knob.chunks = KMP_KNOB("KMP_ZSTD_CHUNKS", 0); c->knob.match_flags = KMP_KNOB("KMP_MATCH_FLAGS", KXM_NT_STORES | KXM_NO_LITS); c->knob.entropy_pad = KMP_KNOB("KMP_ENTROPY_PAD_LDS", 0);
    c->knob.first_permille = KMP_KNOB("KMP_ZSTD_FIRST_PERMILLE", 500); c->knob.fast_first_permille = KMP_KNOB("KMP_ZSTD_FAST_FIRST_PERMILLE", 550); c->knob.entropy_flags = KMP_KNOB("KMP_ENTROPY_FLAGS", 0);
    c->knob.decode_flags = KMP_KNOB("KMP_DECODE_FLAGS", 0); c->knob.decode_pad = KMP_KNOB("KMP_DECODE_PAD_LDS", 0);
    c->knob.big_rounds = KMP_KNOB("KMP_BIG_ROUNDS", 0); c->knob.big_spw = KMP_KNOB("KMP_BIG_SLICES_PER_WAVE", 0);
    c->knob.dfl_chunk = env_u32("KMP_DEFLATE_CHUNK", 16384u); c->knob.dfl_chain_waves = KMP_KNOB("KMP_DEFLATE_CHAIN_WAVES", 4);
    c->knob.dfl_serial = KMP_KNOB("KMP_DEFLATE_SERIAL", 0); c->knob.dfl_flags = KMP_KNOB("KMP_DEFLATE_FLAGS", 0);
    // the decoder's pre-decode kernels (on by default for batches of KMP_PRE_MIN_BATCH = 256 entries or more, DESIGN.md section
    // 4.3): bit 0 = sequences decoded ahead of k_zstd_decode (k_zstd_seq_predecode, one lane per frame), bit 1 = literals
    // (k_zstd_lit_predecode, one lane per stream)
    c->knob.decode_pre = KMP_KNOB("KMP_DECODE_PRE", 3); c->knob.decode_sort = KMP_KNOB("KMP_DECODE_SORT", 1); c->knob.decode_pieces = KMP_KNOB("KMP_DECODE_PIECES", 1); c->knob.decode_stage_slices = env_u32("KMP_DECODE_STAGE_SLICES", 0); c->knob.inflate_pre = KMP_KNOB("KMP_INFLATE_PRE", 1); c->knob.inflate_pieces = KMP_KNOB("KMP_INFLATE_PIECES", 1); c->knob.autotune = KMP_KNOB("KMP_ZSTD_AUTOTUNE", 0);      // opt-in: one launch or two chunks, tried once each (two blocking event reads on the 2nd / 3rd batch)
    c->knob.fuse = KMP_KNOB("KMP_FUSE", 0);                             // 1: k_zstd_l3_fused (the entropy stage inside the parse kernel's waves)
    // entropy sweeps beside the level-3 parse: K (0: off) and the smallest batch that takes the path
    c->knob.sweeps = KMP_KNOB("KMP_ENTROPY_SWEEPS", KMP_SWEEPS_DEFAULT); if (c->knob.sweeps > KX_MAX_SWEEPS) c->knob.sweeps = KX_MAX_SWEEPS;
    c->knob.sweep_min = KMP_KNOB("KMP_ENTROPY_SWEEP_MIN", 16384);
    { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeCanUseStreamWaitValue, device) == hipSuccess) c->can_wait_value = v; else (void)hipGetLastError(); }
    if (!c->big && c->knob.sweeps && c->can_wait_value) {
        KMP_TRY(c->sweep_rec.alloc((KMP_SWEEP_HEAD + 2 * ns) * sizeof(u32), "hipMalloc(sweep records)"));
        KMP_TRY(c->ev_fork.create(hipEventDisableTiming));
    }
    KMP_TRY(c->frame_cks.alloc(ns * sizeof(u32), "hipMalloc(frame checksums)"));
    c->knob.match_v2 = KMP_KNOB("KMP_MATCH_V2", 0);                     // 0: zstd_match.h (the default: 4 % faster, both sit on the same memory floor); 1: zstd_match2.h; 2: with a 512-byte window at team width 4
    HIP_TRY(hipStreamSynchronize(c->st2));
    return KMP_OK;
}

extern "C" void kmp_batch_destroy(kmp_batch_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

/* What the context holds on the device right now, by part (bytes): the arena (or the separate workspace allocations), the other
 * table sets, the decoders' staging, the DEFLATE workspace, the block-chain state.  Sets allocated on first use count once they exist. */
static size_t dict_bytes(const kmp_batch_ctx* c) { size_t b = 0; for (auto const& d : c->dict) b += part_bytes(d); return b; }
extern "C" int kmp_batch_memory(kmp_batch_ctx* c, kmp_batch_memory_info* info)
{
    if (!c || !info || info->struct_bytes < sizeof(kmp_batch_memory_info)) { g_last_error = "kmp_batch_memory: bad argument"; return KMP_ERR_ARG; }
    size_t const ns = c->max_slices;
    kmp_batch_memory_info m = {}; m.struct_bytes = sizeof m;
    m.arena = c->arena.bytes;
    if (c->arena) m.arena_used = (size_t)c->nteams * KX_TBL_ENTRIES * sizeof(u32) + ns * c->seq_cap * sizeof(KSeq) + ns * c->lit_cap + ns * sizeof(KSliceMeta) + ns * c->scratch_words * sizeof(u32);
    m.workspace = c->seqs_buf.bytes + c->lits_buf.bytes + c->meta_buf.bytes + c->scratch_buf.bytes + c->tables_buf.bytes
                + c->team_epoch.bytes + c->counter.bytes + c->len_ok.bytes + c->d_status.bytes + c->sweep_rec.bytes + c->frame_cks.bytes;
    m.other_tables = part_bytes(c->flat) + part_bytes(c->t4) + part_bytes(c->chain_t4) + dict_bytes(c) + part_bytes(c->ddict) + part_bytes(c->lz) + part_bytes(c->lzb);
    m.block_chain = c->fstate.bytes + c->hufct.bytes + c->big_tables.bytes + c->remaining.bytes + c->big_counters.bytes;
    m.decode_staging = part_bytes(c->pre_seq) + part_bytes(c->pre_lit);
    m.deflate_workspace = part_bytes(c->dfl) + part_bytes(c->dflf);
    m.total = m.arena + m.workspace + m.other_tables + m.block_chain + m.decode_staging + m.deflate_workspace;
    *info = m;
    return KMP_OK;
}

/* What the zstd compress batches queued on this context from now on write around their blocks (KMP_FRAME_*): no wait, no device work --
 * a batch takes the flags as they stand when it is queued (batch_view). */
extern "C" int kmp_batch_set_frame_flags(kmp_batch_ctx* c, uint32_t flags)
{
    if (!c) { g_last_error = "kmp_batch_set_frame_flags: null context"; return KMP_ERR_ARG; }
    if (flags & ~(uint32_t)(KMP_FRAME_CHECKSUM | KMP_FRAME_NO_CONTENT_SIZE | KMP_FRAME_NO_DICT_ID)) { g_last_error = "kmp_batch_set_frame_flags: unknown flag"; return KMP_ERR_ARG; }
    c->frame_flags = flags;
    return KMP_OK;
}
extern "C" uint32_t kmp_batch_frame_flags(kmp_batch_ctx* c) { return c ? c->frame_flags : 0u; }
extern "C" int kmp_batch_set_profiling(kmp_batch_ctx* c, int on) { if (!c) return KMP_ERR_ARG; c->profiling = on; return KMP_OK; }
// 0 / 1: mean duration of the k_zstd_match / k_zstd_entropy launches of the last timed level-3 batch; 2: decode; 3: DEFLATE.
// A batch with entropy sweeps beside its parse: 1 is the final sweep alone, the entropy time the step still shows.
extern "C" int kmp_batch_last_kernel_ms(kmp_batch_ctx* c, int which, float* ms)
{
    int const timed = !c || !ms ? 0 : which == 0 || which == 1 ? c->zstd_timed : which == 2 ? c->decode_timed : which == 3 ? c->deflate_timed : 0;
    if (!timed) { g_last_error = "no timing recorded"; return KMP_ERR_ARG; }
    if (which <= 1) {
        float sum = 0;
        for (u32 i = 0; i < c->timed_chunks; i++) {
            kmp_span const& t = which == 0 ? c->match[i] : c->entropy[i]; float x = 0;
            HIP_TRY(hipEventSynchronize(t.end));
            HIP_TRY(hipEventElapsedTime(&x, t.start, t.end));
            sum += x;
        }
        *ms = sum / (float)c->timed_chunks;
        return KMP_OK;
    }
    kmp_span const& t = which == 2 ? c->decode_t : c->deflate_t;
    HIP_TRY(hipEventSynchronize(t.end));
    HIP_TRY(hipEventElapsedTime(ms, t.start, t.end));
    return KMP_OK;
}
/* random 4-byte loads per second and load + store pairs per second over this context's level-3 team tables, measured when
 * the context was created (0 when its tables are small: nothing to price) */
extern "C" int kmp_batch_table_rates(kmp_batch_ctx* c, float* reads_per_s, float* pairs_per_s)
{
    if (!c || !reads_per_s || !pairs_per_s) { g_last_error = "kmp_batch_table_rates: null argument"; return KMP_ERR_ARG; }
    *reads_per_s = c->table_reads_per_s; *pairs_per_s = c->table_pairs_per_s;
    return KMP_OK;
}
// diagnostics: the per-slice records of the last one-block zstd batch (KSliceMeta, 32 bytes each) copied to host memory
extern "C" int kmp_debug_copy_meta(kmp_batch_ctx* c, void* h_dst, uint32_t n)
{
    if (!c || !h_dst || n > c->max_slices) { g_last_error = "kmp_debug_copy_meta: bad argument"; return KMP_ERR_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h_dst, c->meta, (size_t)n * sizeof(KSliceMeta), hipMemcpyDeviceToHost));
    return KMP_OK;
}
/* entropy sweeps of the last level-3 batch: how many were launched, the final one included (0: the batch took the plain path), and
 * with profiling on the slices each of them coded, in launch order.  Waits for the batch. */
extern "C" int kmp_batch_last_sweeps(kmp_batch_ctx* c, uint32_t* coded, uint32_t cap)
{
    if (!c || (cap && !coded)) { g_last_error = "kmp_batch_last_sweeps: null argument"; return -1; }
    u32 const k = c->last_sweeps < cap ? c->last_sweeps : cap;
    if (k) {
        if (hipSetDevice(c->device) != hipSuccess || (c->have_done && hipEventSynchronize(c->ev_done) != hipSuccess)
            || hipMemcpy(coded, c->sweep_rec + 1, k * sizeof(u32), hipMemcpyDeviceToHost) != hipSuccess) { (void)hip_fail(hipGetLastError(), "kmp_batch_last_sweeps"); return -1; }
    }
    return (int)c->last_sweeps;
}
/* launches of each zstd compress kernel in the last batch (the batch is cut into that many chunks) */
extern "C" int kmp_batch_last_chunks(kmp_batch_ctx* c) { return c ? (int)c->last_chunks : 0; }

extern "C" int kmp_batch_status(kmp_batch_ctx* c, uint32_t* bits, void* hip_stream)
{
    if (!c) { g_last_error = "kmp_batch_status: null context"; return KMP_ERR_ARG; }
    hipStream_t const st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(c->device));
    KMP_TRY(batch_wait_previous(c, st));
    // read and clear in ONE atomic exchange: a bit raised by a batch on another stream between a copy and a memset would be lost
    u32 v = 0;
    hipLaunchKernelGGL(k_status_take, dim3(1), dim3(1), 0, st, c->d_status, c->d_status + 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&v, c->d_status + 1, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bits) *bits = v;
    if (v & KMP_STATUS_SLICE_TOO_LARGE) { g_last_error = "a slice is larger than the context was created for: its out_len is 0"; return KMP_ERR_CAPACITY; }
    if (v & KMP_STATUS_KERNEL_GUARD) { g_last_error = "a parser's loop guard tripped: the slice's out_len is 0"; return KMP_ERR_KERNEL; }
    if (v & KMP_STATUS_LEVEL_SIZE) { g_last_error = "the level is not served at a slice's size (levels 9 and 10 up to 16 KiB; level 4 up to 16 KiB on a context for larger slices, and between 128 and 256 KiB as a staged frame; levels 5 .. 10 above 2 MiB): that slice's out_len is 0"; return KMP_ERR_CAPACITY; }
    return KMP_OK;
}

// A batch begins: it waits for the previous batch of this context (whatever stream that ran on), and its kernels get
// the sanitised lengths (k_len_guard).  A batch ends: oversized slices lose their frames, the event is recorded.
int batch_wait_previous(kmp_batch_ctx* c, hipStream_t st)
{
    if (c->have_done) HIP_TRY(hipStreamWaitEvent(st, c->ev_done, 0));
    for (u32 p = 0; p < c->pieces_pending; p++) HIP_TRY(hipStreamWaitEvent(st, c->ev_piece[p], 0));
    return KMP_OK;
}
int batch_begin(kmp_batch_ctx* c, hipStream_t st, const u32* d_in_len, u32 n, u32 cap)
{
    KMP_TRY(batch_wait_previous(c, st));
    if (d_in_len) {
        hipLaunchKernelGGL(k_len_guard, dim3((n + 255) / 256), dim3(256), 0, st, d_in_len, n, cap, c->len_ok, c->d_status);
        HIP_TRY(hipGetLastError());
    }
    return KMP_OK;
}
int batch_end(kmp_batch_ctx* c, hipStream_t st, const u32* d_in_len, u32 n, u32 cap, u32* d_out_len, const KSliceMeta* meta)
{
    if (d_in_len) {
        hipLaunchKernelGGL(k_len_guard_finish, dim3((n + 255) / 256), dim3(256), 0, st, d_in_len, n, cap, d_out_len, meta, c->d_status);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(c->ev_done, st)); c->have_done = 1; c->pieces_pending = 0;      // (this batch waited for the pieces before it)
    return KMP_OK;
}

extern "C" size_t kmp_zstd_compress_bound(size_t n)
{
    return n + (n >> 8) + ((n < (128u << 10)) ? (((128u << 10) - n) >> 11) : 0);
}
// A batch as this context's compress kernels see it: the caller's arrays (the lengths: the sanitised copy) over the context's workspace.
static KBatchView batch_view(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len)
{
    KBatchView v = { (const u8*)d_src, d_in_off, c->len_ok, (u8*)d_dst, d_out_off, d_out_len, n, c->seqs, c->lits, c->meta, c->scratch,
                     kx_work_caps(c->big ? KMP_MAX_SLICE_BYTES : c->max_slice_bytes) };
    v.fflags = c->frame_flags; v.cks = (v.fflags & KXH_CHECKSUM) ? c->frame_cks.p : nullptr;
    return v;
}
// ... and, when its frames carry checksums, the XXH64 pass over its slices, in front of everything that closes a frame (st: where the
// batch -- or this piece of it -- has begun: the sanitised lengths are there)
static int frame_checksums(hipStream_t st, KBatchView const& v)
{
    if (!(v.fflags & KXH_CHECKSUM) || v.n == 0) return KMP_OK;
    hipLaunchKernelGGL(k_frame_xxh64, dim3(kx_frame_xxh_blocks(v.n)), dim3(256), 0, st, kx_frame_xxh_args(v));
    HIP_TRY(hipGetLastError());
    return KMP_OK;
}
static KTeamTables team_tables(kmp_batch_ctx* c) { KTeamTables t = { c->tables, c->team_epoch, c->tseg, c->tseg_n, false }; return t; }
// the tables of the one-position-per-step parsers (levels 1 / 2, dictionary): the level-3 tables when those are one piece,
// else a piece of their own with its own epochs (measured over the spread tables: level 1 19.8 GB/s against 23.9)
static int flat_tables(kmp_batch_ctx* c, KTeamTables* t)
{
    if (c->tseg_n == 1) { *t = kx_one_piece(c->tables, c->team_epoch); return KMP_OK; }
    auto fill = [c](table_part& f) {
        size_t const tbytes = (size_t)c->nteams * KX_TBL_ENTRIES * sizeof(u32);
        KMP_TRY(place_alloc(f.tables, tbytes, nullptr, nullptr));
        KMP_TRY(f.epochs.alloc((size_t)c->nteams * sizeof(u32), "hipMalloc(flat team epochs)"));
        HIP_TRY(hipMemset(f.tables, 0, tbytes));
        HIP_TRY(hipMemset(f.epochs, 0, (size_t)c->nteams * sizeof(u32)));
        return KMP_OK;
    };
    if (!c->flat) KMP_TRY(build_part(c->flat, KMP_PART_FLAT_TABLES, fill));
    *t = kx_one_piece(c->flat->tables, c->flat->epochs);
    return KMP_OK;
}

// ---- levels 1 and 2 -------------------------------------------------------------------------------------
static int zstd_compress_dfast(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                               uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, void* hip_stream, int level);
// ---- levels 5 .. 10: strategies greedy / lazy / lazy2 (zstd_lazy.h), slices of one block ------------------------------------------------
// The batch goes through in pieces that share one workspace (20 bytes a position: the sorted positions with their first bytes, where each
// position stands): sort, then the wave-per-slice parse; the entropy kernel runs once over the whole batch.
static int lazy_workspace(kmp_batch_ctx* c, u32 need_bytes);
static int lazy_parse(kmp_batch_ctx* c, hipStream_t st, KBatchView const& v, int level);
static int zstd_compress_lazy_big(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                  uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, hipStream_t st, int level, u32 mode = KXF_ONE_SHOT, u32 out_chunk = 0);
static int zstd_compress_lazy(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                              uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, void* hip_stream, int level)
{
    KMP_TRY(batch_args("kmp_zstd_compress_batch_level", c, n, { d_src, d_in_off, d_in_len, d_dst, d_out_off, d_out_len }));
    if (n == 0) return KMP_OK;
    hipStream_t const st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(c->device));
    if (c->big) return zstd_compress_lazy_big(c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, st, level);
    KMP_TRY(batch_begin(c, st, d_in_len, n, c->max_slice_bytes));          // (first: waits for the context's previous batch, whose workspace this may replace)
    KMP_TRY(lazy_workspace(c, c->max_slice_bytes));
    KBatchView const v = batch_view(c, d_src, d_in_off, n, d_dst, d_out_off, d_out_len);
    KMP_TRY(frame_checksums(st, v));
    KMP_TRY(lazy_parse(c, st, v, level));
    KEntropyArgs const e = kx_entropy_args(v, kx_entropy_flags_lazy(level));      // literals are gathered by the entropy kernel; the level: it derives each slice's strategy from it
    hipLaunchKernelGGL(k_zstd_entropy, dim3(n), dim3(64), 0, st, e);
    HIP_TRY(hipGetLastError());
    c->last_chunks = 1; c->zstd_timed = 0;          // (no per-chunk timings: those are level 3's)
    return batch_end(c, st, d_in_len, n, c->max_slice_bytes, d_out_len, c->meta);
}
// need_bytes: the largest slice these kernels will parse (level 4 hands them only its slices up to 16 KiB: a quarter of the memory)
static int lazy_workspace(kmp_batch_ctx* c, u32 need_bytes)
{
    u32 const pos_cap = kx_work_caps(need_bytes).pos_cap;
    if (c->lz && c->lz->pos_cap < pos_cap) c->lz.reset();                  // made for a smaller need: once more, larger
    if (c->lz) return KMP_OK;
    auto fill = [c, pos_cap](lazy_part& z) {
        u32 cap = (u32)((1ull << 30) / pos_cap); if (cap > 16384u) cap = 16384u; if (cap < 1u) cap = 1u;
        z.chunk = c->max_slices < cap ? c->max_slices : cap; z.pos_cap = pos_cap;
        KMP_TRY(z.srt.alloc((size_t)z.chunk * pos_cap * sizeof(KLazyRec), "kmp_zstd_compress_batch_level: no memory for the workspace of levels 5 .. 10"));
        KMP_TRY(z.wr.alloc((size_t)z.chunk * pos_cap * sizeof(u32), "kmp_zstd_compress_batch_level: no memory for the workspace of levels 5 .. 10"));
        (void)z.order.alloc(((size_t)2 * z.chunk + 256) * sizeof(u32));      // (without it the slices go as they come)
        return KMP_OK;
    };
    return build_part(c->lz, KMP_PART_LAZY_LEVELS, fill);
}
// sort + parse of the slices of v (a batch or a chunk of one), piece by piece (sequences and the per-slice record go where the other
// parsers put theirs).  Slices the level does not parse this way at their size are skipped: at
// level 4 their record stays what k_zstd_match left (it serves 16 KiB < size <= 128 KiB), at the other levels it says "not served".
static int lazy_parse(kmp_batch_ctx* c, hipStream_t st, KBatchView const& v, int level)
{
    lazy_part const& z = *c->lz;
    for (u32 first = 0; first < v.n; first += z.chunk) {
        u32 const m = (v.n - first < z.chunk) ? v.n - first : z.chunk;
        KLazyArgs g = kx_lazy_args(v.sub(first, m), (KLazyRec*)z.srt.p, z.wr, z.pos_cap, level);
        // (the parse takes the costliest slices first: cost classes from the sort, a counting sort of the classes; batches worth ordering only)
        u32* const ord = (m >= 1024u && z.order) ? z.order.p : nullptr;
        if (ord) { g.order_key = ord; g.order_hist = ord + z.chunk; HIP_TRY(hipMemsetAsync(g.order_hist, 0, 256 * sizeof(u32), st)); }
        hipLaunchKernelGGL(k_zstd_lazy_sort, dim3(m), dim3(256), 0, st, g);
        if (ord) { KMP_TRY(size_sort_keys(c, st, m, g.order_key, g.order_hist, ord + z.chunk + 256)); g.order = ord + z.chunk + 256; }
        if (c->max_slice_bytes <= 65536u) hipLaunchKernelGGL(k_zstd_lazy<2048>, dim3(m), dim3(64), 0, st, g);
        else hipLaunchKernelGGL(k_zstd_lazy<4096>, dim3(m), dim3(64), 0, st, g);
        HIP_TRY(hipGetLastError());
    }
    return KMP_OK;
}

// ... on a context for slices above 128 KiB.  The slices up to 128 KiB go through the one-block kernels above, which see every larger slice
// as an empty one; then k_zstd_lazy_big walks the chains of the slices of 128 KiB + 1 .. 2 MiB, in pieces of as many slices as the part
// holds table slots for.  A slice above 2 MiB is refused (libzstd's parameters are pinned up to there): out_len 0, KMP_STATUS_LEVEL_SIZE.
// mode (KFrameArgs.stream): the reference driver's staged frames (KXF_REFERENCE) go the same way with the input taken in chunks of 128 KiB;
// of a batch of streams every slice, from 0 bytes on, goes through the chain kernel under the unknown-size parameters.
// slot_bytes: what a table slot must hold for this batch.  One-shot and staged frames: by the context's largest slice; streams: by the level's
// hashLog whatever their length (20 MiB at level 10).  A part made with smaller slots is made once more.
static int lazy_big_workspace(kmp_batch_ctx* c, u64 slot_bytes)
{
    if (c->lzb && c->lzb->slot_bytes < slot_bytes) c->lzb.reset();
    if (c->lzb) return KMP_OK;
    auto fill = [c, slot_bytes](lazy_big_part& z) {
        z.slot_bytes = slot_bytes;
        // slices in flight: what 8 GiB of tables hold, 4 096 at most (twice what the device runs at once); KMP_LAZY_BIG_SLICES caps it (the
        // tests run a handful of slices through fewer slots)
        u64 fit = ((u64)8 << 30) / z.slot_bytes; if (fit > 4096u) fit = 4096u;
        u32 const cap = env_u32("KMP_LAZY_BIG_SLICES", (u32)fit);
        if (cap && fit > cap) fit = cap;
        if (fit > c->max_slices) fit = c->max_slices;
        if (fit < 1u) fit = 1u;
        z.chunk = (u32)fit;
        KMP_TRY(z.tables.alloc((size_t)z.chunk * z.slot_bytes, "kmp_zstd_compress_batch_level: no memory for the row tables of levels 5 .. 10"));
        KMP_TRY(z.prev.alloc((size_t)z.chunk * sizeof(KSeqPrev), "kmp_zstd_compress_batch_level: no memory for the workspace of levels 5 .. 10"));
        KMP_TRY(z.small_len.alloc((size_t)c->max_slices * sizeof(u32), "kmp_zstd_compress_batch_level: no memory for the workspace of levels 5 .. 10"));
        return KMP_OK;
    };
    return build_part(c->lzb, KMP_PART_LAZY_BIG, fill);
}
static int zstd_compress_lazy_big(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                  uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, hipStream_t st, int level, u32 mode, u32 out_chunk)
{
    bool const streaming = mode == KXF_STREAM || mode == KXF_STREAM_EMPTY_END;
    KMP_TRY(batch_begin(c, st, d_in_len, n, c->max_slice_bytes));
    KMP_TRY(lazy_big_workspace(c, kx_lazy_big_slot_bytes_mode(c->max_slice_bytes, level, mode)));
    if (!streaming) KMP_TRY(lazy_workspace(c, KMP_MAX_SLICE_BYTES));
    lazy_big_part const& z = *c->lzb;
    KBatchView const v = batch_view(c, d_src, d_in_off, n, d_dst, d_out_off, d_out_len);
    KMP_TRY(frame_checksums(st, v));
    if (!streaming) {
        // the one-block slices (the others: empty frames there, replaced below); staged = in place up to 128 KiB
        hipLaunchKernelGGL(k_zstd_lazy_small_len, dim3((n + 255) / 256), dim3(256), 0, st, v.in_len, n, z.small_len.p);
        HIP_TRY(hipGetLastError());
        KBatchView sv = v; sv.in_len = z.small_len;
        KMP_TRY(lazy_parse(c, st, sv, level));
        KEntropyArgs const e = kx_entropy_args(sv, kx_entropy_flags_lazy(level));
        hipLaunchKernelGGL(k_zstd_entropy, dim3(n), dim3(64), 0, st, e);
        HIP_TRY(hipGetLastError());
    }
    // the frames of several blocks
    HIP_TRY(hipMemsetAsync(c->remaining, 0, 4, st));
    for (u32 first = 0; first < n; first += z.chunk) {
        u32 const m = (n - first < z.chunk) ? n - first : z.chunk;
        KBatchView const pv = v.sub(first, m);
        KLazyBigArgs const g = kx_lazy_big_args(pv, c->fstate + first, c->hufct + (size_t)first * 512u, c->remaining, c->d_status, z.tables, z.slot_bytes, z.prev, level, mode, out_chunk);
        if (mode == KXF_ONE_SHOT) {
            hipLaunchKernelGGL(k_zstd_lazy_big_init, dim3((m + 255) / 256), dim3(256), 0, st, pv.in_len, m, c->fstate + first, z.prev.p, pv.out_len, c->remaining.p, c->d_status.p);
            hipLaunchKernelGGL(k_zstd_lazy_big, dim3(m), dim3(64), 0, st, g);
        } else {
            hipLaunchKernelGGL(k_zstd_lazy_big_init_modes, dim3((m + 255) / 256), dim3(256), 0, st, pv.in_len, m, c->fstate + first, z.prev.p, pv.dst, pv.out_off, pv.out_len, c->remaining.p, c->d_status.p, mode, (u32)level, pv.fflags, pv.cks);
            hipLaunchKernelGGL(k_zstd_lazy_big_modes, dim3(m), dim3(64), 0, st, g);
        }
        HIP_TRY(hipGetLastError());
    }
    c->last_rounds = 0; c->last_chunks = 1; c->zstd_timed = 0;
    // (the per-slice records: of the one-block slices what their parser left -- "not served" at levels 9 and 10 up to 16 KiB --, of the others
    // their last block's; a batch of streams has none for its shortest slices, and a tripped guard is in the status word already)
    return batch_end(c, st, d_in_len, n, c->max_slice_bytes, d_out_len, streaming ? nullptr : c->meta);
}

extern "C" int kmp_zstd_compress_batch_level(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                             uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, int level, void* hip_stream)
{
    if (level == 3 || level == 0) return kmp_zstd_compress_batch(c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, hip_stream);
    if (level == 4) return zstd_compress_dfast(c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, hip_stream, 4);
    if (level >= 5 && level <= 10) return zstd_compress_lazy(c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, hip_stream, level);
    bool const neg = level < 0;                // negative levels: strategy "fast" with a step of 1 - level, literals left uncompressed
    if ((level != 1 && level != 2 && !neg) || level < -131072) { g_last_error = "kmp_zstd_compress_batch_level: levels -131072 .. -1 and 1 .. 10 are served"; return KMP_ERR_ARG; }
    KMP_TRY(batch_args("kmp_zstd_compress_batch_level", c, n, { d_src, d_in_off, d_in_len, d_dst, d_out_off, d_out_len }));
    if (n == 0) return KMP_OK;
    hipStream_t const st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(c->device));
    if (c->big) {
        // frames of several blocks, any size the context holds: beyond the level's window (512 KiB at level 1 and at the negative levels,
        // 1 MiB at level 2) libzstd's staging buffer wraps and the window slides (zstd_match_fast_ext_body)
        KBigLevel const b = kx_big_level(level);
        return zstd_compress_big(c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, st, KXF_ONE_SHOT, b.strategy, 0, b.fast_step0, b.level4);
    }
    KMP_TRY(batch_begin(c, st, d_in_len, n, c->max_slice_bytes));
    HIP_TRY(hipMemsetAsync(c->counter, 0, 4 * KMP_MAX_CHUNKS, st));
    // One launch of each kernel.  (KMP_ZSTD_CHUNKS=2 splits the batch as at level 3, the entropy kernel of the first chunk on
    // the second stream beside the parse of the second: measured 16.3 - 17.1 GB/s against 21.9 in one piece at 65 536 x 64 KiB --
    // this parser needs all the slices in flight.)
    u32 const tpw = 64 / (u32)c->G;
    u32 chunks = c->knob.chunks ? c->knob.chunks : 1u;
    if (chunks > 2) chunks = 2;
    u32 starts[3] = { 0, n, n };
    if (chunks == 2) { u32 const pm = c->knob.fast_first_permille; starts[1] = (u32)((u64)n * (pm >= 100 && pm <= 950 ? pm : 500u) / 1000u) & ~63u; if (starts[1] == 0 || starts[1] >= n) chunks = 1, starts[1] = n; }
    bool forked = false;
    KBatchView const v = batch_view(c, d_src, d_in_off, n, d_dst, d_out_off, d_out_len);
    KMP_TRY(frame_checksums(st, v));
    KTeamTables flat; KMP_TRY(flat_tables(c, &flat));
    for (u32 ci = 0; ci < chunks; ci++) {
        u32 const first = starts[ci], m_n = starts[ci + 1] - first;
        if (m_n == 0) continue;
        KBatchView const cv = v.sub(first, m_n);
        KFastArgs const g = kx_fast_args(cv, flat, c->counter + ci, level);
        u32 blocks = (m_n + tpw - 1) / tpw; if (blocks > c->match_blocks) blocks = c->match_blocks;
        by_team_width(c->G, [&](auto w) { hipLaunchKernelGGL(k_zstd_match_fast<decltype(w)::value>, dim3(blocks), dim3(64), 0, st, g); });
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->match[ci].end, st));
        KEntropyArgs const e = kx_entropy_args(cv, kx_entropy_flags_fast(neg));   // gather literals; strategy "fast"; negative levels: literals stay raw
        hipStream_t es = st;
        if (ci + 1 < chunks) { es = c->st2; HIP_TRY(hipStreamWaitEvent(es, c->match[ci].end, 0)); forked = true; }
        hipLaunchKernelGGL(k_zstd_entropy, dim3(m_n), dim3(64), 0, es, e);
        HIP_TRY(hipGetLastError());
    }
    if (forked) { HIP_TRY(hipEventRecord(c->ev_join, c->st2)); HIP_TRY(hipStreamWaitEvent(st, c->ev_join, 0)); }
    c->last_chunks = chunks; c->zstd_timed = 0;
    return batch_end(c, st, d_in_len, n, c->max_slice_bytes, d_out_len, c->meta);
}

// ---- compressing with a raw-content dictionary ------------------------------------------------------
// libzstd's CDict for the dictionary: parameters of ZSTD_getCParams(3, unknown source size, dictSize) in
// "create CDict" mode, then ZSTD_fillDoubleHashTableForCDict over the dictionary (tagged entries: index << 8 | tag).
int dict_header_state(const unsigned char* dict, size_t dict_size, int for_decoder)
{
    KDictPrior pr; KDictDPrior dp; size_t off = 0;
    return cdict_parse_formatted(dict, dict_size, &pr, &off, for_decoder ? &dp : nullptr);
}

// level: 3, 1, 2 or a negative one; fn: the entry point's name for the messages
static int zstd_compress_dict(const char* fn, kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                              uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len,
                              const void* h_dict, uint32_t dict_size, int level, void* hip_stream)
{
    std::string const name(fn);
    KMP_TRY(batch_args(fn, c, n, { d_src, d_in_off, d_in_len, d_dst, d_out_off, d_out_len }, h_dict != nullptr));
    if (c->big) { g_last_error = name + ": slices above 128 KiB are not served with a dictionary"; return KMP_ERR_CAPACITY; }
    if (dict_size < 8 || dict_size > KX_MAX_DICT) { g_last_error = name + ": dictionary of 8 .. 130560 bytes expected"; return KMP_ERR_CAPACITY; }
    if (n == 0) return KMP_OK;
    hipStream_t const st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(c->device));
    // the CDict of this dictionary at this level class: one the context holds, else built now
    int const cls = kx_dict_level_class(level);
    u64 hsh = 1469598103934665603ull; for (u32 i = 0; i < dict_size; i++) { hsh ^= ((const u8*)h_dict)[i]; hsh *= 1099511628211ull; }
    int slot = -1;
    for (int i = 0; i < KMP_DICT_SLOTS; i++) if (c->dict[i] && c->dict[i]->size == dict_size && c->dict[i]->hash == hsh && c->dict[i]->level_class == cls) slot = i;
    if (slot < 0) {
        // A dictionary in zstd's own format (magic EC30A437) is loaded as libzstd loads it: entropy tables and repeat offsets for the first
        // block (KDictPrior), the bytes behind them as the content matches are searched in; anything else is content from its first byte.
        KDictPrior prior; size_t content_off = 0;
        int const formatted = cdict_parse_formatted((const u8*)h_dict, dict_size, &prior, &content_off);
        if (formatted < 0) { g_last_error = name + ": the dictionary starts with zstd's dictionary magic but its header is damaged (libzstd: Dictionary is corrupted)"; return KMP_ERR_ARG; }
        const u8* const content = (const u8*)h_dict + content_off; u32 const content_size = dict_size - (u32)content_off;
        HIP_TRY(hipStreamSynchronize(st));
        // into a free slot, else over the one unused longest
        slot = 0;
        for (int i = 0; i < KMP_DICT_SLOTS; i++) if (!c->dict[i]) { slot = i; break; } else if (c->dict[i]->used < c->dict[slot]->used) slot = i;
        c->dict[slot].reset();
        auto fill = [&](dict_part& d) {
            cdict_params(dict_size, &d.W, &d.C, &d.H, &d.M, cls);   // (libzstd sizes the CDict and the frame's window by the whole dictionary, header included)
            std::vector<u32> tl, ts;
            if (cls == 3) cdict_fill(tl, d.H, ts, d.C, d.M, content, content_size);
            else cdict_fill_fast(tl, d.H, d.C, d.M, content, content_size);
            KMP_TRY(d.content.alloc(content_size + 64, "hipMalloc(dictionary)"));
            KMP_TRY(d.L.alloc(tl.size() * 4, "hipMalloc(dictionary tables)"));
            HIP_TRY(hipMemcpy(d.content, content, content_size, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(d.L, tl.data(), tl.size() * 4, hipMemcpyHostToDevice));
            if (cls == 3) {
                KMP_TRY(d.S.alloc(ts.size() * 4, "hipMalloc(dictionary tables)"));
                HIP_TRY(hipMemcpy(d.S, ts.data(), ts.size() * 4, hipMemcpyHostToDevice));
            }
            if (formatted) {
                KMP_TRY(d.prior.alloc(sizeof(KDictPrior), "hipMalloc(dictionary entropy tables)"));
                HIP_TRY(hipMemcpy(d.prior, &prior, sizeof(KDictPrior), hipMemcpyHostToDevice));
                d.rep[0] = prior.rep[0]; d.rep[1] = prior.rep[1];
            } else { d.rep[0] = 1; d.rep[1] = 4; }
            d.content_size = content_size;
            d.size = dict_size; d.hash = hsh; d.level_class = cls;
            return KMP_OK;
        };
        // (a build that fails -- memory is short -- leaves no dictionary behind: the ones the context kept go as well)
        if (int const rc = build_part(c->dict[slot], KMP_PART_DICT, fill)) { for (auto& d : c->dict) d.reset(); return rc; }
    }
    dict_part& dp = *c->dict[slot];
    dp.used = ++c->dict_tick;
    KMP_TRY(batch_begin(c, st, d_in_len, n, c->max_slice_bytes));
    HIP_TRY(hipMemsetAsync(c->counter, 0, 4, st));
    KBatchView const v = batch_view(c, d_src, d_in_off, n, d_dst, d_out_off, d_out_len);
    KMP_TRY(frame_checksums(st, v));
    KTeamTables flat; KMP_TRY(flat_tables(c, &flat));
    u32 const tpw = 64 / (u32)c->G;
    u32 blocks = (n + tpw - 1) / tpw; if (blocks > c->match_blocks) blocks = c->match_blocks;
    u32 eflags = KXE_GATHER_LITS;                                 // literals are gathered by the entropy kernel
    if (c->profiling) HIP_TRY(hipEventRecord(c->match[0].start, st));
    if (cls == 3) {
        KDictArgs const g = kx_dict_args(v, flat, c->counter, dp.content, dp.content_size, dp.L, dp.S, dp.W, dp.H, dp.C, dp.M, dp.rep[0], dp.rep[1]);
        by_team_width(c->G, [&](auto w) { hipLaunchKernelGGL(k_zstd_match_dict<decltype(w)::value>, dim3(blocks), dim3(64), 0, st, g); });
    } else {
        KFastDictArgs const g = kx_fast_dict_args(v, flat, c->counter, dp.content, dp.content_size, dp.L, dp.W, dp.H, dp.M, dp.rep[0], dp.rep[1], level);
        by_team_width(c->G, [&](auto w) { hipLaunchKernelGGL(k_zstd_match_fast_dict<decltype(w)::value>, dim3(blocks), dim3(64), 0, st, g); });
        eflags = kx_entropy_flags_fast(level < 0);               // strategy "fast"; negative levels: literals stay raw
    }
    HIP_TRY(hipGetLastError());
    if (c->profiling) { HIP_TRY(hipEventRecord(c->match[0].end, st)); HIP_TRY(hipEventRecord(c->entropy[0].start, st)); }
    KEntropyArgs const e = kx_entropy_args(v, eflags, dp.prior, dp.size);
    if (dp.prior) hipLaunchKernelGGL(k_zstd_entropy_prior, dim3(n), dim3(64), 0, st, e);
    else hipLaunchKernelGGL(k_zstd_entropy, dim3(n), dim3(64), 0, st, e);
    HIP_TRY(hipGetLastError());
    if (c->profiling) HIP_TRY(hipEventRecord(c->entropy[0].end, st));
    c->last_chunks = 1; c->zstd_timed = c->profiling; c->timed_chunks = 1;      // (kmp_batch_last_kernel_ms: the parse and the entropy launch)
    return batch_end(c, st, d_in_len, n, c->max_slice_bytes, d_out_len, c->meta);
}

extern "C" int kmp_zstd_compress_batch_dict(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                            uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len,
                                            const void* h_dict, uint32_t dict_size, void* hip_stream)
{ return zstd_compress_dict("kmp_zstd_compress_batch_dict", c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, h_dict, dict_size, 3, hip_stream); }

extern "C" int kmp_zstd_compress_batch_dict_level(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                                  uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len,
                                                  const void* h_dict, uint32_t dict_size, int level, void* hip_stream)
{
    if (level == 0 || level == 3) return kmp_zstd_compress_batch_dict(c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, h_dict, dict_size, hip_stream);
    if (level > 3 || level < -131072) { g_last_error = "kmp_zstd_compress_batch_dict_level: levels -131072 .. -1 and 1 .. 3 are served with a dictionary"; return KMP_ERR_ARG; }
    return zstd_compress_dict("kmp_zstd_compress_batch_dict_level", c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, h_dict, dict_size, level, hip_stream);
}

// Level 4's slices of 128 KiB + 1 .. 256 KiB in a one-shot batch: libzstd parses that size class "greedy" over its row-based match finder
// (ZSTD_getCParams(4, n)), which is zstd_lazy_big.h's chain with level 4's row.  Runs behind k_zstd_big on the batch's stream: the other
// slices' frames stand, these slices' states are made anew (k_zstd_lazy_big_init_l4) and their chains walked in pieces of as many slices as the
// part holds table slots for (5 << 17 bytes each at this row's hashLog).
static int level4_greedy_class(kmp_batch_ctx* c, hipStream_t st, KBatchView const& v)
{
    KMP_TRY(lazy_big_workspace(c, kx_lazy_big_slot_bytes(17u)));
    lazy_big_part const& z = *c->lzb;
    for (u32 first = 0; first < v.n; first += z.chunk) {
        u32 const m = (v.n - first < z.chunk) ? v.n - first : z.chunk;
        KBatchView const pv = v.sub(first, m);
        KLazyBigArgs const g = kx_lazy_big_args(pv, c->fstate + first, c->hufct + (size_t)first * 512u, c->remaining, c->d_status, z.tables, z.slot_bytes, z.prev, 4);
        hipLaunchKernelGGL(k_zstd_lazy_big_init_l4, dim3((m + 255) / 256), dim3(256), 0, st, pv.in_len, m, c->fstate + first, z.prev.p, c->remaining.p);
        hipLaunchKernelGGL(k_zstd_lazy_big, dim3(m), dim3(64), 0, st, g);
        HIP_TRY(hipGetLastError());
    }
    return KMP_OK;
}

// Slices above 128 KiB: frames of several blocks.  Every round runs the match kernel and the frame kernel over
// one block of every unfinished slice; block sizes depend on the bytes already produced (ZSTD_optimalBlockSize),
// so the rounds are sequential and the host only reads back how many frames are still open.
// stream: KFrameArgs.stream (0 ZSTD_compress2's frames, 1 / 2 streaming frames, 3 the reference's one-shot driver)
int zstd_compress_big(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                      uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, hipStream_t st, u32 stream, u32 strategy, u32 tail_direct, u32 fast_step0, bool level4)
{
    bool const streaming = stream == KXF_STREAM || stream == KXF_STREAM_EMPTY_END;
    KMP_TRY(batch_begin(c, st, d_in_len, n, c->max_slice_bytes));
    if (level4) {
        // level 4's double-fast rows on this path (16 - 128 KiB: hash 17 / chain 17; above 256 KiB and streams: 18 / 18): per-slice tables of
        // 2 MiB, allocated by the first such batch of the context
        auto fill = [c](table_part& t) { return t.tables.alloc((size_t)c->max_slices * KX_BIG4_ENTRIES * sizeof(u32), "kmp_zstd_compress_batch_level: no memory for level 4's tables"); };
        if (!c->chain_t4) KMP_TRY(build_part(c->chain_t4, KMP_PART_CHAIN_TABLES4, fill));
        HIP_TRY(hipMemsetAsync(c->chain_t4->tables, 0, (size_t)n * KX_BIG4_ENTRIES * sizeof(u32), st));
    } else
    HIP_TRY(hipMemsetAsync(c->big_tables, 0, (size_t)n * KX_BIG_TBL_ENTRIES * sizeof(u32), st));
    HIP_TRY(hipMemsetAsync(c->remaining, 0, 4, st));
    // strategy: 0 level 3 (double-fast), 1 level 1 (fast), 2 level 2 (fast, but double-fast for 128 KiB < size <= 256 KiB when the size is known)
    KBatchView const v = batch_view(c, d_src, d_in_off, n, d_dst, d_out_off, d_out_len);
    KMP_TRY(frame_checksums(st, v));
#ifdef KMP_ABLATIONS
    bool const chains = strategy || c->knob.big_rounds == 0;
#else
    bool const chains = true;
#endif
    // level 4, sizes known: the "greedy" class above a block (128 - 256 KiB) goes through k_zstd_lazy_big behind the chains of the others (one-shot
    // frames on the product path); staged frames of that class and the class up to 16 KiB stay refused here
    bool const l4_greedy = level4 && stream == KXF_ONE_SHOT && chains;
    hipLaunchKernelGGL(k_zstd_frame_init, dim3((n + 255) / 256), dim3(256), 0, st, v.in_len, n, c->fstate, v.dst, d_out_off, d_out_len, c->remaining, kx_big_window_byte(stream, strategy), stream != KXF_ONE_SHOT ? 1u : 0u, level4 ? (l4_greedy ? 2u : 1u) : 0u, c->d_status, v.fflags, v.cks);
    HIP_TRY(hipGetLastError());
    KMatchArgs const m = kx_match_args_blk(v, team_tables(c), c->counter, streaming, c->max_slice_bytes >= KX_BLK_WIDE_FROM, c->fstate, level4 ? c->chain_t4->tables.p : c->big_tables.p, level4);
    // (a negative level: the level-1 machinery (window 2^19) on row 0 of the tables, a step of 1 - level, raw literals)
    KBigLevel const lv = { strategy, fast_step0, level4 };
    KFrameArgs const e = kx_frame_args(v, c->fstate, c->hufct, c->remaining, c->d_status, stream, lv, tail_direct);
    if (chains) {
        // one wave per slice walks its chain of blocks
        // few slices: one per wave (most waves); many: up to 64 / G per wave so that all of them are in flight
        // lanes per slice: every slice of the batch should be in flight (its block chain is serial), and a parse team
        // gains little beyond 8 lanes -- measured on 1 MiB and 256 KiB slices: 8 lanes up to 16 K slices, 4 above
        int const bigG = c->big_G ? c->big_G : (n >= 16384u ? 4 : 8);
        u32 const resident = 12u * c->cus;
        u32 spw = c->knob.big_spw ? c->knob.big_spw : (n + resident - 1) / resident;
        if (spw < 1) spw = 1; if (spw > 64u / (u32)bigG) spw = 64u / (u32)bigG;
        if (!c->knob.big_spw) {
            // ... and a grid that is a whole number of waves per CU when a few more slices per wave give one: the launch lasts as
            // long as its fullest CU (8 192 x 1 MiB: 3 slices per wave = 2 731 waves 6.5 GB/s, 4 = 2 048 waves 7.3)
            for (u32 t = spw; t <= 64u / (u32)bigG && t <= spw + 2u; t++) if (((n + t - 1) / t) % c->cus == 0) { spw = t; break; }
        }
        KBigArgs g = kx_big_args(m, e, c->big_counters, spw);
        u32 const grid = (n + spw - 1) / spw;
        HIP_TRY(hipMemsetAsync(c->big_counters, 0, (size_t)n * 4, st));
        if (strategy == 2u && !streaming) {
            // level 2, sizes known: the slices of its double-fast row first (class 1), the others (class 2) through the fast parser below
            kx_big_set_class(g, m.flags, KXC_L2_DFAST);
            by_team_width(bigG, [&](auto w) { hipLaunchKernelGGL(k_zstd_big<decltype(w)::value>, dim3(grid), dim3(64), 0, st, g); });
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemsetAsync(c->big_counters, 0, (size_t)n * 4, st));
            kx_big_set_class(g, m.flags, KXC_L2_FAST);
        }
        if (strategy) by_team_width(bigG, [&](auto w) { hipLaunchKernelGGL(k_zstd_big_fast<decltype(w)::value>, dim3(grid), dim3(64), 0, st, g); });
        else by_team_width(bigG, [&](auto w) { hipLaunchKernelGGL(k_zstd_big<decltype(w)::value>, dim3(grid), dim3(64), 0, st, g); });
        HIP_TRY(hipGetLastError());
        if (l4_greedy) KMP_TRY(level4_greedy_class(c, st, v));
        c->last_rounds = 0; c->last_chunks = 1; c->zstd_timed = 0;
        return batch_end(c, st, d_in_len, n, c->max_slice_bytes, d_out_len, nullptr);
    }
#ifdef KMP_ABLATIONS
    // (experiment switch KMP_BIG_ROUNDS=1) the same steps as separate launches per round of blocks
    int const bigR = c->big_G ? c->big_G : 8;
    u32 const tpw = 64 / (u32)bigR;
    u32 const blocks = (n + tpw - 1) / tpw;
    u32 rounds = 0;
    for (;;) {
        u32 left = 0;
        HIP_TRY(hipMemcpyAsync(&left, c->remaining, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (left == 0) break;
        if (++rounds > KMP_MAX_BIG_SLICE_BYTES / 64u) { g_last_error = "kmp_zstd_compress_batch: block rounds did not finish"; return KMP_ERR_KERNEL; }
        HIP_TRY(hipMemsetAsync(c->counter, 0, 8, st));
        by_team_width(bigR, [&](auto w) { hipLaunchKernelGGL(k_zstd_match_blk<decltype(w)::value>, dim3(blocks), dim3(64), 0, st, m); });
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_zstd_frame, dim3(n), dim3(64), 0, st, e);
        HIP_TRY(hipGetLastError());
    }
    c->last_rounds = rounds; c->last_chunks = 1; c->zstd_timed = 0;
    return batch_end(c, st, d_in_len, n, c->max_slice_bytes, d_out_len, nullptr);
#else
    g_last_error = "zstd_compress_big: unreachable"; return KMP_ERR_ARG;
#endif
}
/* Streaming frames: what libzstd writes when a slice arrives through finish = false calls and is closed with
 * finish = true (size unknown when the frame starts).  empty_end: the closing calls brought no data.  The context must
 * have been created for slices above 128 KiB (the block-chain path and its 2^17 / 2^16 tables serve every size here). */
extern "C" int kmp_zstd_compress_batch_stream_level(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                                    uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, int empty_end, int level, void* hip_stream);
extern "C" int kmp_zstd_compress_batch_stream(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                              uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, int empty_end, void* hip_stream)
{ return kmp_zstd_compress_batch_stream_level(c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, empty_end, 3, hip_stream); }
/* level 3, or level 1 (the Ktor encoder's: streams <= 512 KiB, its window) or level 2 (<= 1 MiB) */
extern "C" int kmp_zstd_compress_batch_stream_level(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                                    uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, int empty_end, int level, void* hip_stream)
{
    if (level == 0) level = 3;
    bool const neg = level < 0;
    if ((level < 1 && !neg) || level > 10 || level < -131072) { g_last_error = "kmp_zstd_compress_batch_stream_level: levels -131072 .. -1 and 1 .. 10 are served"; return KMP_ERR_ARG; }
    KMP_TRY(args_present("kmp_zstd_compress_batch_stream", c != nullptr, n, { d_src, d_in_off, d_in_len, d_dst, d_out_off, d_out_len }));
    if (!c->big) { g_last_error = "kmp_zstd_compress_batch_stream: the context must be created with max_slice_bytes above 128 KiB"; return KMP_ERR_CAPACITY; }
    KMP_TRY(args_count("kmp_zstd_compress_batch_stream", c, n));
    if (n == 0) return KMP_OK;
    HIP_TRY(hipSetDevice(c->device));
    // levels 5 .. 10: streams of 0 .. 2 MiB, every one through the chain kernel of zstd_lazy_big.h (longer ones are refused per slice)
    if (level >= 5) return zstd_compress_lazy_big(c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, (hipStream_t)hip_stream, level, empty_end ? KXF_STREAM_EMPTY_END : KXF_STREAM, 0);
    KBigLevel const b = kx_big_level(level);
    return zstd_compress_big(c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, (hipStream_t)hip_stream, empty_end ? KXF_STREAM_EMPTY_END : KXF_STREAM, b.strategy, 0, b.fast_step0, b.level4);
}
/* What ZstdCompressor(level).transform(ByteArray) returns: above 128 KiB libzstd stages the input in chunks of 128 KiB
 * because the reference's output slices are smaller than ZSTD_compressBound (include/kompressor_hip.h). */
extern "C" int kmp_zstd_compress_batch_reference(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                                 uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, int level, uint32_t out_chunk, void* hip_stream)
{
    if (level == 0) level = 3;
    KMP_TRY(args_present("kmp_zstd_compress_batch_reference", c != nullptr, 0, {}));
    if (!c->big) return kmp_zstd_compress_batch_level(c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, level, hip_stream);   // one block: one chunk
    bool const neg = level < 0;
    if ((level < 1 && !neg) || level > 10 || level < -131072) { g_last_error = "kmp_zstd_compress_batch_reference: levels -131072 .. -1 and 1 .. 10 are served"; return KMP_ERR_ARG; }
    KMP_TRY(batch_args("kmp_zstd_compress_batch_reference", c, n, { d_src, d_in_off, d_in_len, d_dst, d_out_off, d_out_len }));
    if (n == 0) return KMP_OK;
    HIP_TRY(hipSetDevice(c->device));
    // levels 5 .. 10: one block up to 128 KiB (staged = in place there), staged frames up to 2 MiB, larger slices refused per slice
    if (level >= 5) return zstd_compress_lazy_big(c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, (hipStream_t)hip_stream, level, KXF_REFERENCE, out_chunk);
    KBigLevel const b = kx_big_level(level);
    return zstd_compress_big(c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, (hipStream_t)hip_stream, KXF_REFERENCE, b.strategy, out_chunk, b.fast_step0, b.level4);
}
/* block rounds of the last batch of a context for slices above 128 KiB */
extern "C" int kmp_batch_last_rounds(kmp_batch_ctx* c) { return c ? (int)c->last_rounds : 0; }

// Level 4 where it is the double-fast parse (slices above 16 KiB up to 128 KiB: zstd_common.h kx_params_l4): its tables are
// 1 MiB per team, a set of their own allocated by the first such batch (as many teams as level 3 has, memory permitting; the
// batch's slices go through them by the work counter).
static int ensure_tables4(kmp_batch_ctx* c)
{
    if (c->t4) return KMP_OK;
    // as many teams as level 3 has (65 536 x 64 KiB: 19.4 GB/s with 65 536 teams = 64 GiB of tables, 15.9 with 32 768, 14.6 with 16 384:
    // tools/r03_l4.sh), fewer when the device has less room (16 GiB stay free); KMP_L4_TEAMS caps it (the tests run many slices
    // through few teams)
    u32 const cap4 = env_u32("KMP_L4_TEAMS", 65536);
    u32 teams = c->nteams < cap4 ? c->nteams : cap4;
    { size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) == hipSuccess) { size_t const room = fr > ((size_t)16 << 30) ? (fr - ((size_t)16 << 30)) / ((size_t)KX_TBL4_ENTRIES * sizeof(u32)) : 0; if (teams > room) teams = (u32)room; } else (void)hipGetLastError(); }
    teams &= ~63u; if (teams == 0) teams = 64;
    size_t const bytes = (size_t)teams * KX_TBL4_ENTRIES * sizeof(u32);
    auto fill = [bytes, teams](table_part& t) {
        KMP_TRY(t.tables.alloc(bytes, "kmp_zstd_compress_batch_level: no memory for level 4's tables"));
        KMP_TRY(t.epochs.alloc((size_t)teams * sizeof(u32), "kmp_zstd_compress_batch_level: no memory for level 4's tables"));
        if (hipMemset(t.tables, 0, bytes) != hipSuccess || hipMemset(t.epochs, 0, (size_t)teams * sizeof(u32)) != hipSuccess) { (void)hipGetLastError(); g_last_error = "kmp_zstd_compress_batch_level: hipMemset failed"; return KMP_ERR_HIP; }
        t.teams = teams;
        return KMP_OK;
    };
    return build_part(c->t4, KMP_PART_TABLES4, fill);
}

static int zstd_compress_dfast(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                               uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, void* hip_stream, int level)
{
    KMP_TRY(batch_args("kmp_zstd_compress_batch", c, n, { d_src, d_in_off, d_in_len, d_dst, d_out_off, d_out_len }));
    if (n == 0) return KMP_OK;
    hipStream_t const st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(c->device));
    bool const l4 = level == 4;
    if (l4 && !c->big) KMP_TRY(ensure_tables4(c));
    if (c->big) return zstd_compress_big(c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, st, KXF_ONE_SHOT, 0, 0, 0, l4);
    // Chunks: the match kernel of chunk i+1 (memory-transaction bound) runs beside the entropy kernel of
    // chunk i (latency bound) on a second stream; the caller's stream sees everything finished.
    // (two chunks only when each still fills at least half of the match kernel's team slots: 65 536 x 64 KiB -> 2,
    // 32 768 x 128 KiB -> 1: 17.7 GB/s against 13.1 with two half-empty launches)
    u32 const team_slots = c->l3_team_slots;                 // what the device holds, whatever this context's max_slices
    u32 chunks = l4 ? 1u : c->knob.chunks ? c->knob.chunks : (n > team_slots ? 2u : 1u);       // measured: 49 152 slices (= the slots) 16.4 GB/s in one launch, 15.5 in two; 57 344: 15.2 / 16.2
    bool const tunable = !l4 && !c->knob.chunks && c->knob.autotune && n <= team_slots && 2u * n > team_slots;
    if (tunable) {
        if (c->tune_pending) {                       // the previous such batch was a trial: its whole-step time
            c->tune_pending = 0;
            float ms = 0;
            if (hipEventSynchronize(c->tune.end) == hipSuccess && hipEventElapsedTime(&ms, c->tune.start, c->tune.end) == hipSuccess) c->tune_ms[c->tune_state++] = ms;
            else { (void)hipGetLastError(); c->tune_state = 2; c->tune_pick = 0; }
            if (c->tune_state == 2 && c->tune_ms[1] > 0) c->tune_pick = c->tune_ms[1] < c->tune_ms[0] ? 1u : 0u;
        }
        chunks = (c->tune_state < 2 ? (u32)c->tune_state : c->tune_pick) ? 2u : 1u;
    }
    if (chunks < 1) chunks = 1; if (chunks > KMP_MAX_CHUNKS) chunks = KMP_MAX_CHUNKS; if (chunks > n) chunks = 1;
    // One batch at a time per context (the sequence / literal / scratch workspaces and the team tables are shared): a
    // batch queued on another stream waits for the last kernel of the previous one.  (Letting the next batch's match
    // kernel start beside this batch's last entropy launch was measured and gave nothing: DESIGN.md section 8.)
    KMP_TRY(batch_begin(c, st, d_in_len, n, c->max_slice_bytes));
    if (tunable && c->tune_state < 2) HIP_TRY(hipEventRecord(c->tune.start, st));
    HIP_TRY(hipMemsetAsync(c->counter, 0, 4 * KMP_MAX_CHUNKS, st));
    // Team width per batch: a small batch is bound by each slice's own chain, not by the memory system, and 8 lanes per slice
    // (7 positions per step) run it a quarter faster than 4 (64 slices: 29 ms against 39; 4 096: 43 against 49; 16 384 and up: 4
    // wins).  The tables belong to team slots, not to a width, so the choice is free per batch (KMP_TEAM_LANES or an explicit
    // team_lanes fixes it).
    int const G = (c->G == 4 && !c->team_fixed && n <= 8192u) ? 8 : c->G;
    u32 const tpw = 64 / (u32)G;
    u32 const match_flags = c->knob.match_flags, entropy_pad = c->knob.entropy_pad;   // experiments only
    u32 const per = (n + chunks - 1) / chunks;
    u32 starts[KMP_MAX_CHUNKS + 1];
    for (u32 ci = 0; ci <= chunks; ci++) starts[ci] = (ci * per < n) ? ci * per : n;
    // two chunks: the last entropy launch is the only one nothing runs beside, so the second chunk is the smaller one
    if (chunks == 2) { u32 const pm = c->knob.first_permille; if (pm >= 100 && pm <= 950) starts[1] = (u32)((u64)n * pm / 1000u) & ~63u; if (starts[1] == 0 || starts[1] >= n) starts[1] = per; }
    bool forked = false;
    // Entropy sweeps beside the parse: level 3, one launch, team width 4 (the parse kernel that leaves a wave slot free) and a batch
    // large enough to fill the device; neither of the ablation build's other forms of the step
    bool const sweep = !l4 && chunks == 1 && G == 4 && c->sweep_rec && n >= c->knob.sweep_min && !c->knob.fuse && !c->knob.match_v2 && (match_flags & KXM_NO_LITS);
    KSweepRecords const rec = { c->sweep_rec + KMP_SWEEP_HEAD, c->sweep_rec + KMP_SWEEP_HEAD + n, c->sweep_rec };
    c->last_sweeps = 0;
    KBatchView const v = batch_view(c, d_src, d_in_off, n, d_dst, d_out_off, d_out_len);
    KMP_TRY(frame_checksums(st, v));
    KTeamTables const tables = l4 ? kx_one_piece(c->t4->tables, c->t4->epochs, true) : team_tables(c);
    for (u32 ci = 0; ci < chunks; ci++) {
        u32 const first = starts[ci], m_n = starts[ci + 1] - first;
        if (m_n == 0) continue;
        KBatchView const cv = v.sub(first, m_n);
        KMatchArgs m = kx_match_args(cv, tables, c->counter + ci, match_flags);
        if (sweep) {
            // cleared per batch on the caller's stream; the second stream starts behind the clears, so no wait reads an old count
            HIP_TRY(hipMemsetAsync(c->sweep_rec, 0, (KMP_SWEEP_HEAD + 2 * (size_t)n) * sizeof(u32), st));
            HIP_TRY(hipEventRecord(c->ev_fork, st));
            kx_match_records(m, rec);
        }
        u32 max_blocks = (u32)((u64)c->match_blocks_l3 * (64u / (u32)c->G) / tpw);      // the context's team slots at this batch's width
        if (l4 && max_blocks > c->t4->teams / tpw) max_blocks = c->t4->teams / tpw;
        u32 blocks = (m_n + tpw - 1) / tpw; if (blocks > max_blocks) blocks = max_blocks;
        if (c->profiling) HIP_TRY(hipEventRecord(c->match[ci].start, st));
#ifdef KMP_ABLATIONS
        // the ablation build's other two forms of the level-3 step: the split-phase parser, the fused kernel
        bool const fuse = c->knob.fuse && !c->knob.match_v2 && !l4 && (G == 4 || G == 8);
        if (fuse) {
            KEntropyArgs const e = kx_entropy_args(cv, c->knob.entropy_flags | kx_entropy_flags_dfast(m.flags, false));
            if (G == 4) hipLaunchKernelGGL(k_zstd_l3_fused<4>, dim3(blocks), dim3(64), 0, st, m, e);
            else hipLaunchKernelGGL(k_zstd_l3_fused<8>, dim3(blocks), dim3(64), 0, st, m, e);
        } else
        if (c->knob.match_v2 && !l4 && (G == 2 || G == 4 || G == 8)) {
            m.flags |= KXM_NO_LITS;                                       // this parser never copies literals: the entropy kernel gathers them
            bool const r512 = c->knob.match_v2 == 2;
            switch (G) {
            case 2:  hipLaunchKernelGGL((k_zstd_match2<2, 256>), dim3(blocks), dim3(64), 0, st, m); break;
            case 4:  if (r512) hipLaunchKernelGGL((k_zstd_match2<4, 512>), dim3(blocks), dim3(64), 0, st, m); else hipLaunchKernelGGL((k_zstd_match2<4, 256>), dim3(blocks), dim3(64), 0, st, m); break;
            default: hipLaunchKernelGGL((k_zstd_match2<8, 512>), dim3(blocks), dim3(64), 0, st, m); break;
            }
        } else
#else
        bool const fuse = false;
#endif
        by_team_width(G, [&](auto w) { hipLaunchKernelGGL(k_zstd_match<decltype(w)::value>, dim3(blocks), dim3(64), 0, st, m); });
        HIP_TRY(hipGetLastError());
        if (l4) {
            // level 4 up to 16 KiB is strategy "greedy" (ZSTD_getCParams(4, n <= 16 KiB)): those slices, which k_zstd_match has passed over, are
            // parsed by the kernels of levels 5 .. 10 (zstd_lazy.h), which pass over all the others
            KMP_TRY(lazy_workspace(c, c->max_slice_bytes < 16384u ? c->max_slice_bytes : 16384u));
            KMP_TRY(lazy_parse(c, st, cv, 4));
        }
        HIP_TRY(hipEventRecord(c->match[ci].end, st));
        KEntropyArgs const e = kx_entropy_args(cv, c->knob.entropy_flags | kx_entropy_flags_dfast(m.flags, l4));
        if (sweep) {
            // Sweep j starts once the parse has counted T_j finished slices (hipStreamWaitValue32, queued behind the parse's launch,
            // and the parse counts every slice: zstd_match.h KST_CLEANUP) and codes whatever is finished and uncoded by then, in the
            // wave slot the parse leaves free on every SIMD.  No kernel waits for anything.  The final sweep runs on the caller's
            // stream behind the parse and the other sweeps and codes the rest: the frames do not depend on what ran when.
            u32 T[KX_MAX_SWEEPS]; u32 const nt = kx_sweep_thresholds(n, c->knob.sweeps, T);
            HIP_TRY(hipStreamWaitEvent(c->st2, c->ev_fork, 0));
            for (u32 j = 0; j < nt; j++) {
                HIP_TRY(hipStreamWaitValue32(c->st2, rec.count, T[j], hipStreamWaitValueGte, 0xFFFFFFFFu));
                hipLaunchKernelGGL(k_zstd_entropy, dim3(m_n), dim3(64), 0, c->st2, kx_entropy_sweep_args(e, rec, c->profiling ? c->sweep_rec + 1 + j : nullptr));
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(hipEventRecord(c->ev_join, c->st2)); HIP_TRY(hipStreamWaitEvent(st, c->ev_join, 0));
            if (c->profiling) HIP_TRY(hipEventRecord(c->entropy[ci].start, st));
            hipLaunchKernelGGL(k_zstd_entropy, dim3(m_n), dim3(64), 0, st, kx_entropy_sweep_args(e, rec, c->profiling ? c->sweep_rec + 1 + nt : nullptr));
            HIP_TRY(hipGetLastError());
            if (c->profiling) HIP_TRY(hipEventRecord(c->entropy[ci].end, st));
            c->last_sweeps = nt + 1;
            continue;
        }
        hipStream_t es = st;
        if (ci + 1 < chunks) { es = c->st2; HIP_TRY(hipStreamWaitEvent(es, c->match[ci].end, 0)); forked = true; }
        if (c->profiling) HIP_TRY(hipEventRecord(c->entropy[ci].start, es));
        if (!fuse) hipLaunchKernelGGL(k_zstd_entropy, dim3(m_n), dim3(64), entropy_pad, es, e);
        HIP_TRY(hipGetLastError());
        if (c->profiling) HIP_TRY(hipEventRecord(c->entropy[ci].end, es));
    }
    if (forked) { HIP_TRY(hipEventRecord(c->ev_join, c->st2)); HIP_TRY(hipStreamWaitEvent(st, c->ev_join, 0)); }
    c->last_chunks = chunks;
    c->zstd_timed = c->profiling; c->timed_chunks = chunks;
    if (tunable && c->tune_state < 2) { HIP_TRY(hipEventRecord(c->tune.end, st)); c->tune_pending = 1; }
    return batch_end(c, st, d_in_len, n, c->max_slice_bytes, d_out_len, c->meta);
}
// ---- a batch in pieces, each on a stream of its own ---------------------------------------------------------------------
// What a caller with HOST memory needs (every caller of the reference's boundary starts and ends there): the slices arrive over
// PCIe while earlier ones are being compressed, the frames leave while later ones still are.  One launch over the whole batch
// cannot start before its last slice is in; pieces run one after the other lose what makes this parser fast -- every slice in
// flight (16 384 slices alone take 73 ms, 65 536 together 187).  So the pieces of one batch run SIDE BY SIDE: piece p's kernels
// go to hip_streams[p] (behind whatever the caller queued there: its copy in), own the p-th part of the context's team slots
// (KMatchArgs.block_base) and of its workspace, and the device fills up as the pieces arrive.
extern "C" void kmp_batch_piece_range(uint32_t n, uint32_t pieces, uint32_t piece, uint32_t* first, uint32_t* count)
{
    if (pieces == 0) pieces = 1;
    auto cut = [&](u32 p) -> u32 { return p >= pieces ? n : (u32)(((u64)n * p / pieces) & ~63ull); };
    u32 const a = cut(piece), b = cut(piece + 1);
    if (first) *first = a;
    if (count) *count = b > a ? b - a : 0u;
}
// the three steps of a batch in pieces (kmp_coalesce.h queues a piece as soon as its copy in is queued)
int pieces_begin(kmp_batch_ctx* c, u32 pieces, void* const* hip_streams)
{
    KMP_TRY(args_present("kmp_zstd_compress_batch_pieces", c && hip_streams, 0, {}));
    if (pieces < 1 || pieces > KMP_MAX_PIECES) { g_last_error = "kmp_zstd_compress_batch_pieces: 1 .. 8 pieces"; return KMP_ERR_ARG; }
    if (c->big) { g_last_error = "kmp_zstd_compress_batch_pieces: contexts for slices up to 128 KiB only"; return KMP_ERR_CAPACITY; }
    if (c->match_blocks_l3 / pieces == 0) { g_last_error = "kmp_zstd_compress_batch_pieces: more pieces than the context has workgroups"; return KMP_ERR_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    // every stream first waits for whatever ran on this context before (a batch, or the pieces of one)
    for (u32 p = 0; p < pieces; p++) KMP_TRY(batch_wait_previous(c, (hipStream_t)hip_streams[p]));
    return KMP_OK;
}
int piece_enqueue(kmp_batch_ctx* c, u32 p, u32 pieces, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n,
                  void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, hipStream_t st)
{
    u32 const tpw = 64 / (u32)c->G;
    u32 const blocks_per_piece = c->match_blocks_l3 / pieces;
    u32 first = 0, m_n = 0; kmp_batch_piece_range(n, pieces, p, &first, &m_n);
    if (m_n == 0) { HIP_TRY(hipEventRecord(c->ev_piece[p], st)); return KMP_OK; }
    hipLaunchKernelGGL(k_len_guard, dim3((m_n + 255) / 256), dim3(256), 0, st, d_in_len + first, m_n, c->max_slice_bytes, c->len_ok + first, c->d_status);
    HIP_TRY(hipMemsetAsync(c->counter + p, 0, 4, st));
    KBatchView const v = batch_view(c, d_src, d_in_off, n, d_dst, d_out_off, d_out_len).sub(first, m_n);
    KMP_TRY(frame_checksums(st, v));
    KMatchArgs const m = kx_match_args(v, team_tables(c), c->counter + p, c->knob.match_flags, p * blocks_per_piece);
    u32 blocks = (m_n + tpw - 1) / tpw; if (blocks > blocks_per_piece) blocks = blocks_per_piece;
    by_team_width(c->G, [&](auto w) { hipLaunchKernelGGL(k_zstd_match<decltype(w)::value>, dim3(blocks), dim3(64), 0, st, m); });
    HIP_TRY(hipGetLastError());
    KEntropyArgs const e = kx_entropy_args(v, c->knob.entropy_flags | kx_entropy_flags_dfast(m.flags, false));
    hipLaunchKernelGGL(k_zstd_entropy, dim3(m_n), dim3(64), 0, st, e);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_len_guard_finish, dim3((m_n + 255) / 256), dim3(256), 0, st, d_in_len + first, m_n, c->max_slice_bytes, d_out_len + first, c->meta + first, c->d_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_piece[p], st));
    return KMP_OK;
}

extern "C" int kmp_zstd_compress_batch_pieces(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n,
                                              void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, uint32_t pieces, void* const* hip_streams)
{
    KMP_TRY(batch_args("kmp_zstd_compress_batch_pieces", c, n, { d_src, d_in_off, d_in_len, d_dst, d_out_off, d_out_len }, hip_streams != nullptr));
    KMP_TRY(pieces_begin(c, pieces, hip_streams));
    if (n == 0) return KMP_OK;
    pieces_end end = { c, pieces, hip_streams, 0 };
    for (; end.queued < pieces; end.queued++) KMP_TRY(piece_enqueue(c, end.queued, pieces, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, (hipStream_t)hip_streams[end.queued]));
    return KMP_OK;
}
// frame i of a piece straight into the caller's HOST memory (registered / pinned: h_dst is its device-visible address): what the
// dense packing + copy out + host-side memcpy do for pageable memory, in one kernel over PCIe.  A frame larger than its room is
// not written: out_len 0, status 70 (libzstd's "Destination buffer is too small").
__global__ __launch_bounds__(64) void k_scatter_frames(const u8* src, const u64* in_off, u32* len, u32 n, u8* h_dst, const u64* h_off, const u32* h_cap, u32* status)
{
    int const lane = threadIdx.x;
    for (u32 it = blockIdx.x; it < n; it += gridDim.x) {
        u32 const i = kx_xcd_chunk(it, n);
        u32 const L = len[i];
        bool const fits = L <= h_cap[i];
        if (lane == 0) status[i] = (L == 0) ? 1u : fits ? 0u : 70u;
        if (!fits) { if (lane == 0) len[i] = 0; continue; }
        const u8* s = src + in_off[i]; u8* d = h_dst + h_off[i];
        // 16 bytes per lane where both sides allow it (the strided frames start on 64-byte boundaries; the caller's offsets may not)
        u32 k = (u32)lane * 8u;
        for (; k + 8 <= L; k += 512u) kx_st64(d + k, kx_ld64(s + k));
        u32 const tail = L & ~7u;
        if (lane < (int)(L - tail)) d[tail + lane] = s[tail + lane];
    }
}
int scatter_frames(kmp_batch_ctx* c, hipStream_t st, const u8* d_src, const u64* d_in_off, u32* d_len, u32 n, u8* h_dst_dev, const u64* d_h_off, const u32* d_h_cap, u32* d_status)
{
    (void)c;
    if (!n) return KMP_OK;
    u32 const blocks = n < 16384u ? n : 16384u;
    hipLaunchKernelGGL(k_scatter_frames, dim3(blocks), dim3(64), 0, st, d_src, d_in_off, d_len, n, h_dst_dev, d_h_off, d_h_cap, d_status);
    HIP_TRY(hipGetLastError());
    return KMP_OK;
}

extern "C" int kmp_zstd_compress_batch(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                       uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, void* hip_stream)
{
    return zstd_compress_dfast(c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_len, hip_stream, 3);
}

// Staging for what the pre-decode kernels leave (8 bytes per sequence -- a frame of S bytes holds at most S / 3 -- and
// the literals): allocated on the first call that wants it, for as many entries as 48 GiB hold (all of them for the bench's
// batches; a larger batch goes through in pieces, one after the other, that reuse the staging).  Shared by the zstd decoder
// and inflate.
u32 env_pre_min_batch() { static u32 const v = env_u32("KMP_PRE_MIN_BATCH", 256); return v; }
void ensure_pre_staging(kmp_batch_ctx* c)
{
    if (c->pre_tried || !c->knob.decode_pre) return;
    c->pre_tried = 1;
    u32 const seq_cap = c->max_slice_bytes / 3u + 64u, blk_cap = c->max_slice_bytes / 8192u + 16u, lit_cap = c->max_slice_bytes + 64u;
    u64 const per_entry = (u64)seq_cap * 8u + (u64)lit_cap + (u64)blk_cap * (sizeof(KPreBlk) + sizeof(KPreLit)) + 64u;
    u64 fit = c->knob.decode_stage_slices ? c->knob.decode_stage_slices : (48ull << 30) / per_entry;
    if (fit > c->max_slices) fit = c->max_slices;
    if (fit >= 1024u) fit &= ~1023ull;                           // (whole workgroups of every kernel)
    u32 const ps = (u32)fit;
    c->pre_blk_cap = blk_cap;
    auto seqs = [&](pre_seq_part& q) {
        KMP_TRY(q.stage.alloc((size_t)ps * seq_cap * 8u));
        KMP_TRY(q.blk.alloc((size_t)ps * blk_cap * sizeof(KPreBlk)));
        KMP_TRY(q.nblk.alloc((size_t)ps * 4u));
        KMP_TRY(q.sort.alloc(((size_t)ps * 2u + KXP_SORT_BUCKETS) * 4u));
        q.seq_cap = seq_cap;
        return KMP_OK;
    };
    auto lits = [&](pre_lit_part& q) {
        KMP_TRY(q.lits.alloc((size_t)ps * lit_cap));
        KMP_TRY(q.rec.alloc((size_t)ps * blk_cap * sizeof(KPreLit)));
        KMP_TRY(q.nrec.alloc((size_t)ps * 4u));
        q.lit_cap = lit_cap;
        return KMP_OK;
    };
    if (ps && (c->knob.decode_pre & 1u) && build_part(c->pre_seq, KMP_PART_PRE_SEQ, seqs) == KMP_OK) c->pre_slices = ps;
    if (ps && (c->knob.decode_pre & 2u) && build_part(c->pre_lit, KMP_PART_PRE_LIT, lits) == KMP_OK) c->pre_slices = ps;
}

// the counting sort behind the lane-per-entry kernels' slot order (key, rank, permutation: three small launches)
int size_sort(kmp_batch_ctx* c, hipStream_t st, const u8* src, const u64* in_off, const u32* in_len, u32 m, u32* key, u32* hist, u32* perm, u32 len_shift)
{
    (void)c;
    HIP_TRY(hipMemsetAsync(hist, 0, (size_t)KXP_SORT_BUCKETS * 4u, st));
    KSeqSortArgs sa;
    sa.src = src; sa.in_off = in_off; sa.in_len = in_len; sa.n_slices = m; sa.key = key; sa.hist = hist; sa.perm = perm; sa.len_shift = len_shift;
    hipLaunchKernelGGL(k_zstd_seq_count, dim3((m + 255) / 256), dim3(256), 0, st, sa);
    hipLaunchKernelGGL(k_zstd_seq_rank, dim3(1), dim3(256), 0, st, sa);
    hipLaunchKernelGGL(k_zstd_seq_perm, dim3((m + 255) / 256), dim3(256), 0, st, sa);
    HIP_TRY(hipGetLastError());
    return KMP_OK;
}

int size_sort_keys(kmp_batch_ctx* c, hipStream_t st, u32 m, u32* key, u32* hist, u32* perm)
{
    (void)c;
    KSeqSortArgs sa;
    sa.src = nullptr; sa.in_off = nullptr; sa.in_len = nullptr; sa.n_slices = m; sa.key = key; sa.hist = hist; sa.perm = perm; sa.len_shift = 0;
    hipLaunchKernelGGL(k_zstd_seq_rank, dim3(1), dim3(256), 0, st, sa);
    hipLaunchKernelGGL(k_zstd_seq_perm, dim3((m + 255) / 256), dim3(256), 0, st, sa);
    HIP_TRY(hipGetLastError());
    return KMP_OK;
}

static int zstd_decompress_impl(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                uint32_t n, void* d_dst, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                                uint32_t* d_out_len, uint32_t* d_status, const void* d_dict, uint32_t dict_size, void* hip_stream)
{
    KMP_TRY(batch_args("kmp_zstd_decompress_batch", c, n, { d_src, d_in_off, d_in_len, d_dst, d_out_off, d_out_cap, d_out_len, d_status }));
    if (n == 0) return KMP_OK;
    hipStream_t const st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(c->device));
    KDecodeArgs d;
    d.src = (const u8*)d_src; d.in_off = d_in_off; d.in_len = d_in_len; d.n_slices = n;
    d.dst = (u8*)d_dst; d.out_off = d_out_off; d.out_cap = d_out_cap; d.out_len = d_out_len; d.status = d_status;
    d.lits = c->lits; d.lit_cap = c->lit_cap; d.flags = c->knob.decode_flags;
    KMP_TRY(batch_begin(c, st, nullptr, n, 0));            // the decoder checks every length itself; lits is shared with the compressors
    d.dict = (const u8*)d_dict; d.dict_size = d_dict ? dict_size : 0u;
    u32 start_rep[3] = { 1, 4, 8 };
    if (d_dict && dict_size >= 8) {
        // A dictionary in zstd's own format brings tables, repeat offsets and an ID (ZSTD_loadDEntropy): its head is read back and parsed once
        // per dictionary (recognised by address, size and the head's bytes); the kernels get the content part and the parsed rest.
        u8 head[2048]; u32 const hn = dict_size < sizeof head ? dict_size : (u32)sizeof head;
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpy(head, d_dict, hn, hipMemcpyDeviceToHost));
        u64 hsh = 1469598103934665603ull; for (u32 i = 0; i < hn; i++) { hsh ^= head[i]; hsh *= 1099511628211ull; }
        if (!c->ddict || c->ddict->ptr != d_dict || c->ddict->size != dict_size || c->ddict->hash != hsh) {
            KDictDPrior dp; size_t off = 0;
            int const formatted = cdict_parse_formatted(head, dict_size, nullptr, &off, &dp, hn);
            if (formatted < 0) { g_last_error = "kmp_zstd_decompress_batch_dict: the dictionary starts with zstd's dictionary magic but its header is damaged (libzstd: Dictionary is corrupted)"; return KMP_ERR_ARG; }
            c->ddict.reset();
            auto fill = [&](ddict_part& q) {
                if (formatted) {
                    KMP_TRY(q.prior.alloc(sizeof(KDictDPrior), "hipMalloc(dictionary entropy tables)"));
                    HIP_TRY(hipMemcpy(q.prior, &dp, sizeof(KDictDPrior), hipMemcpyHostToDevice));
                    q.off = (u32)off; q.id = dp.dictID; q.rep[0] = dp.rep[0]; q.rep[1] = dp.rep[1]; q.rep[2] = dp.rep[2];
                }
                q.ptr = d_dict; q.size = dict_size; q.hash = hsh;
                return KMP_OK;
            };
            KMP_TRY(build_part(c->ddict, KMP_PART_DDICT, fill));
        }
        ddict_part const& q = *c->ddict;
        if (q.prior) {
            d.dict = (const u8*)d_dict + q.off; d.dict_size = dict_size - q.off; d.dprior = q.prior; d.dict_id = q.id;
            start_rep[0] = q.rep[0]; start_rep[1] = q.rep[1]; start_rep[2] = q.rep[2];
        }
    }
    // The pre-decoders' staging (ensure_pre_staging) serves batches of KMP_PRE_MIN_BATCH entries or more.
    // (a small batch -- the one-frame contexts of the streaming entry points above all -- goes straight to k_zstd_decode: a quad
    // or a lane doing a whole frame's serial decode first is the old serial cost plus a second pass, and the staging is memory)
    bool const use_pre = n >= env_pre_min_batch();
    if (use_pre) ensure_pre_staging(c);
    pre_seq_part const* const ps = use_pre ? c->pre_seq.get() : nullptr; pre_lit_part const* const pl = use_pre ? c->pre_lit.get() : nullptr;
    d.pre_stage = nullptr; d.pre_seq_cap = 0; d.pre_blk = nullptr; d.pre_blk_cap = c->pre_blk_cap; d.pre_nblk = nullptr;
    d.pre_lits = nullptr; d.pre_lit_cap = 0; d.pre_lit = nullptr; d.pre_nlit = nullptr;
    if (c->profiling) HIP_TRY(hipEventRecord(c->decode_t.start, st));
    if (!ps && !pl) {
        hipLaunchKernelGGL(k_zstd_decode, dim3(n), dim3(64), c->knob.decode_pad, st, d);   // padding = occupancy experiment only
        HIP_TRY(hipGetLastError());
    } else {
        // piece by piece (one piece unless the batch is larger than the staging; KMP_DECODE_PIECES asks for more): the two
        // pre-decoders side by side -- literals on the caller's stream, sequences on the context's second one, their lane
        // slots in order of sequence count (neighbours in size share a wave) -- then k_zstd_decode
        u32 pieces = (n + c->pre_slices - 1) / c->pre_slices;
        if (c->knob.decode_pieces > pieces && n >= 8192u) pieces = c->knob.decode_pieces;
        u32 per = ((n + pieces - 1) / pieces + 63u) & ~63u;
        if (per > c->pre_slices) per = c->pre_slices;
        u32* const sort_key = ps ? ps->sort.p : nullptr; u32* const sort_perm = ps ? ps->sort + c->pre_slices : nullptr; u32* const sort_hist = ps ? ps->sort + 2u * (size_t)c->pre_slices : nullptr;
        for (u32 first = 0; first < n; first += per) {
            u32 const m = (n - first < per) ? n - first : per;
            bool const sorted = ps && c->knob.decode_sort != 0 && m >= 1024u;
            if (sorted) KMP_TRY(size_sort(c, st, d.src, d_in_off + first, d_in_len + first, m, sort_key, sort_hist, sort_perm, 0));
            KDecodeArgs q = d;
            q.in_off = d_in_off + first; q.in_len = d_in_len + first; q.n_slices = m;
            q.out_off = d_out_off + first; q.out_cap = d_out_cap + first; q.out_len = d_out_len + first; q.status = d_status + first;
            q.lits = c->lits + (size_t)first * c->lit_cap;
            if (ps) {
                // (st2 starts where st stands: behind the previous piece's k_zstd_decode, which read the staging)
                HIP_TRY(hipEventRecord(c->ev_pre[0], st)); HIP_TRY(hipStreamWaitEvent(c->st2, c->ev_pre[0], 0));
                KPreArgs p;
                p.perm = sorted ? sort_perm : nullptr;
                p.src = d.src; p.in_off = q.in_off; p.in_len = q.in_len; p.n_slices = m;
                p.stage = ps->stage; p.seq_cap = ps->seq_cap; p.blk = ps->blk; p.blk_cap = c->pre_blk_cap; p.nblk = ps->nblk;
                p.rep[0] = start_rep[0]; p.rep[1] = start_rep[1]; p.rep[2] = start_rep[2];
                hipLaunchKernelGGL(k_zstd_seq_predecode, dim3((m + KXP_FRAMES - 1) / KXP_FRAMES), dim3(4 * KXP_FRAMES), 0, c->st2, p);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipEventRecord(c->ev_pre[1], c->st2));
                q.pre_stage = ps->stage; q.pre_seq_cap = ps->seq_cap; q.pre_blk = ps->blk; q.pre_nblk = ps->nblk;
            }
            if (pl) {
                KLitArgs p;
                p.perm = sorted ? sort_perm : nullptr;
                p.src = d.src; p.in_off = q.in_off; p.in_len = q.in_len; p.n_slices = m;
                p.lits = pl->lits; p.lit_cap = pl->lit_cap; p.rec = pl->rec; p.blk_cap = c->pre_blk_cap; p.nrec = pl->nrec;
                hipLaunchKernelGGL(k_zstd_lit_predecode, dim3((m + KXL_FRAMES - 1) / KXL_FRAMES), dim3(64), 0, st, p);
                HIP_TRY(hipGetLastError());
                q.pre_lits = pl->lits; q.pre_lit_cap = pl->lit_cap; q.pre_lit = pl->rec; q.pre_nlit = pl->nrec;
            }
            if (ps) HIP_TRY(hipStreamWaitEvent(st, c->ev_pre[1], 0));
            hipLaunchKernelGGL(k_zstd_decode, dim3(m), dim3(64), c->knob.decode_pad, st, q);
            HIP_TRY(hipGetLastError());
        }
    }
    if (c->profiling) { HIP_TRY(hipEventRecord(c->decode_t.end, st)); c->decode_timed = 1; }
    return batch_end(c, st, nullptr, n, 0, nullptr, nullptr);
}

extern "C" int kmp_zstd_decompress_batch(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                         uint32_t n, void* d_dst, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                                         uint32_t* d_out_len, uint32_t* d_status, void* hip_stream)
{ return zstd_decompress_impl(c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_cap, d_out_len, d_status, nullptr, 0, hip_stream); }
extern "C" int kmp_zstd_decompress_batch_dict(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                              uint32_t n, void* d_dst, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                                              uint32_t* d_out_len, uint32_t* d_status, const void* d_dict, uint32_t dict_size, void* hip_stream)
{ return zstd_decompress_impl(c, d_src, d_in_off, d_in_len, n, d_dst, d_out_off, d_out_cap, d_out_len, d_status, d_dict, dict_size, hip_stream); }
// Frame inspection: neither call allocates, waits or touches the context's decode staging; they are queued on the caller's stream
// like any kernel of its own (no batch_begin: nothing of the context is used but its device and max_slices).
extern "C" int kmp_zstd_frame_info_batch(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n,
                                         kmp_zstd_frame_info* d_info, void* hip_stream)
{
    KMP_TRY(batch_args("kmp_zstd_frame_info_batch", c, n, { d_src, d_in_off, d_in_len, d_info }));
    if (n == 0) return KMP_OK;
    HIP_TRY(hipSetDevice(c->device));
    KFrameInfoArgs const a = { (const u8*)d_src, d_in_off, d_in_len, n, d_info };
    u32 const blocks = (n + 255u) / 256u;                    // (n is bounded by max_slices; the body strides over what a smaller grid leaves)
    hipLaunchKernelGGL(k_zstd_frame_info, dim3(blocks < 4096u ? blocks : 4096u), dim3(256), 0, (hipStream_t)hip_stream, a);
    HIP_TRY(hipGetLastError());
    return KMP_OK;
}
extern "C" int kmp_batch_layout(kmp_batch_ctx* c, const kmp_zstd_frame_info* d_info, uint32_t n, uint32_t align,
                                uint64_t* d_out_off, uint32_t* d_out_cap, uint64_t* d_total, void* hip_stream)
{
    KMP_TRY(batch_args("kmp_batch_layout", c, n, { d_info, d_out_off, d_out_cap, d_total }));
    if (align == 0 || align > 4096u || (align & (align - 1u))) { g_last_error = "kmp_batch_layout: align must be a power of two from 1 to 4096"; return KMP_ERR_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) { if (d_total) HIP_TRY(hipMemsetAsync(d_total, 0, 2 * sizeof(uint64_t), (hipStream_t)hip_stream)); return KMP_OK; }
    KLayoutArgs const a = { d_info, n, align, d_out_off, d_out_cap, d_total };
    hipLaunchKernelGGL(k_batch_layout, dim3(1), dim3(64 * KFI_LAYOUT_WAVES), 0, (hipStream_t)hip_stream, a);
    HIP_TRY(hipGetLastError());
    return KMP_OK;
}
// ... and on the host: the same body through the compiler's host pass, no GPU touched; large batches on up to 16 threads
extern "C" int kmp_zstd_frame_info_host(const void* h_src, const uint64_t* in_off, const uint32_t* in_len, uint32_t n, kmp_zstd_frame_info* info)
{
    KMP_TRY(args_present("kmp_zstd_frame_info_host", true, n, { h_src, in_off, in_len, info }));
    auto run = [=](u32 b, u32 e) { for (u32 i = b; i < e; i++) kx_frame_info((const u8*)h_src + in_off[i], in_len[i], info + i); };
    u32 hw = std::thread::hardware_concurrency();
    u32 const workers = n < 8192u ? 1u : hw < 2u ? 1u : hw > 16u ? 16u : hw;
    if (workers == 1u) { run(0, n); return KMP_OK; }
    std::vector<std::thread> th;
    u32 const per = (n + workers - 1u) / workers;
    for (u32 b = per; b < n; b += per) th.emplace_back(run, b, n - b < per ? n : b + per);
    run(0, per);
    for (auto& t : th) t.join();
    return KMP_OK;
}
extern "C" int kmp_compact_batch(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_len, uint32_t n,
                                 void* d_dst, uint64_t* d_out_off, void* hip_stream)
{
    if (!c || !d_src || !d_in_off || !d_len || !d_dst || !d_out_off) { g_last_error = "kmp_compact_batch: null argument"; return KMP_ERR_ARG; }
    hipStream_t const st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(c->device));
    hipLaunchKernelGGL(k_scan_lengths, dim3(1), dim3(1024), 0, st, d_len, n, d_out_off);
    HIP_TRY(hipGetLastError());
    if (n) {
        u32 const blocks = n < 65536u ? n : 65536u;
        hipLaunchKernelGGL(k_compact, dim3(blocks), dim3(64), 0, st, (const u8*)d_src, d_in_off, d_len, n, (u8*)d_dst, (const u64*)d_out_off);
        HIP_TRY(hipGetLastError());
    }
    return KMP_OK;
}
