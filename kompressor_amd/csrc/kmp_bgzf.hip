// kmp_bgzf.hip -- the host half of the BGZF container (bgzf.h): kmp_bgzf_*.  A container is made of calls the library already has --
// kmp_deflate_compress_batch_level (format 0) over the blocks, kmp_compact_batch to pack the members, kmp_inflate_batch (format 0) over
// the covering members of a read -- with this unit's kernels around them: the wrap, the marker, the trailers' check, and the open, which
// finds the members of a blob in parallel (BGZF has no table).  The context allocates nothing here: compress works in the caller's
// scratch, a reader's arrays belong to its handle, the open's tables live for the call.
#include "kx_wave.h"
#include "zstd_seekable.h"           // (seekable_plan_body: the blocks of one buffer as a batch)
#include "bgzf.h"
#include "kmp_internal.h"

#include <algorithm>
#include <vector>

__global__ __launch_bounds__(256) void k_bgzf_plan(KSeekPlanArgs a) { seekable_plan_body(a); }
__global__ __launch_bounds__(64) void k_bgzf_wrap(KBgzfWrapArgs a) { bgzf_wrap_body(a); }
__global__ __launch_bounds__(256) void k_bgzf_finish(KBgzfFinishArgs a) { bgzf_finish_body(a); }
__global__ __launch_bounds__(64) void k_bgzf_walk(const u8* blob, u64 size, kmp_bgzf_stat* stat, u64* member_off, u64* content_off, u64 cap, KBgzfArrays arr)
{ bgzf_walk_body(blob, size, stat, member_off, content_off, cap, arr); }
__global__ __launch_bounds__(256) void k_bgzf_scan(KBgzfScanArgs a) { bgzf_scan_body(a); }
__global__ __launch_bounds__(1024) void k_bgzf_prefix(u32* v, u64 n) { bgzf_prefix_body(v, n); }
__global__ __launch_bounds__(256) void k_bgzf_link(KBgzfLinkArgs a) { bgzf_link_body(a); }
__global__ __launch_bounds__(256) void k_bgzf_double(const u32* prev, u32* next, u32 n) { bgzf_double_body(prev, next, n); }
__global__ __launch_bounds__(256) void k_bgzf_mark(const u32* jump, u32* mark, u32 n) { bgzf_mark_body(jump, mark, n); }
__global__ __launch_bounds__(1024) void k_bgzf_gather(KBgzfGatherArgs a) { bgzf_gather_body(a); }
__global__ __launch_bounds__(64) void k_bgzf_verify(KBgzfVerifyArgs a) { bgzf_verify_body(a); }

static u32 grid_for(u64 items, u32 per_block, u32 most) { u64 const b = (items + per_block - 1u) / per_block; return (u32)(b < 1u ? 1u : b < most ? b : most); }

// ---- the caller's scratch: four arrays over the n blocks, then the members at `stride` ---------------------------------------------
struct bgzf_layout { u64 n, stride, in_off, out_off, dense_off, in_len, out_len, frames, total; };
static bool bgzf_block_bytes_ok(u32 block_bytes) { return block_bytes >= 1u && block_bytes <= KBZ_BLOCK_MAX; }
static u64 bgzf_member_bound(u64 len) { return (u64)kmp_deflate_bound((size_t)len) + 8u; }      // (kmp_deflate_bound holds 18 bytes of wrapper already)
static bgzf_layout bgzf_scratch_layout(size_t src_size, u32 block_bytes)
{
    bgzf_layout l;
    l.n = ((u64)src_size + block_bytes - 1u) / block_bytes;
    l.stride = (KBZ_HEAD + bgzf_member_bound(block_bytes) + 63u) & ~63ull;        // (the batch is promised kmp_deflate_bound behind the header)
    l.in_off = 0; l.out_off = l.in_off + 8u * l.n; l.dense_off = l.out_off + 8u * l.n;
    l.in_len = l.dense_off + 8u * (l.n + 1u); l.out_len = l.in_len + 4u * l.n;
    l.frames = (l.out_len + 4u * l.n + 63u) & ~63ull;
    l.total = l.frames + l.n * l.stride + 64u;
    return l;
}

extern "C" size_t kmp_bgzf_bound(size_t src_size, uint32_t block_bytes, uint32_t flags)
{
    if (!bgzf_block_bytes_ok(block_bytes)) return 0;
    u64 const n = ((u64)src_size + block_bytes - 1u) / block_bytes;
    u64 const last = n ? (u64)src_size - (n - 1u) * block_bytes : 0u;
    return (size_t)((n ? (n - 1u) * bgzf_member_bound(block_bytes) + bgzf_member_bound(last) : 0u) + ((flags & KMP_BGZF_NO_EOF) ? 0u : KBZ_EOF_BYTES));
}
extern "C" size_t kmp_bgzf_scratch(size_t src_size, uint32_t block_bytes)
{
    return bgzf_block_bytes_ok(block_bytes) ? (size_t)bgzf_scratch_layout(src_size, block_bytes).total : 0;
}

extern "C" int kmp_bgzf_compress(kmp_batch_ctx* c, const void* d_src, size_t src_size, uint32_t block_bytes, int level, uint32_t flags,
                                 void* d_dst, size_t dst_cap, void* d_scratch, size_t scratch_bytes, uint64_t* d_result, void* hip_stream)
{
    const char* const fn = "kmp_bgzf_compress";
    if (!c || !d_dst || !d_scratch || !d_result || (src_size && !d_src)) { g_last_error = std::string(fn) + ": null argument"; return KMP_ERR_ARG; }
    if (!bgzf_block_bytes_ok(block_bytes)) { g_last_error = std::string(fn) + ": block_bytes must be 1 .. 65280"; return KMP_ERR_ARG; }
    if (level == -1) level = 6;
    if (level < 1 || level > 9) { g_last_error = std::string(fn) + ": levels 1 .. 9 (-1 = 6) are served"; return KMP_ERR_ARG; }
    if (flags & ~KMP_BGZF_NO_EOF) { g_last_error = std::string(fn) + ": unknown flag"; return KMP_ERR_ARG; }
    if (((uintptr_t)d_scratch | (uintptr_t)d_result) & 7u) { g_last_error = std::string(fn) + ": d_scratch and d_result must be 8-byte aligned"; return KMP_ERR_ARG; }
    if (block_bytes > c->max_slice_bytes) { g_last_error = std::string(fn) + ": block_bytes exceeds the context's max_slice_bytes"; return KMP_ERR_CAPACITY; }
    bgzf_layout const l = bgzf_scratch_layout(src_size, block_bytes);
    if (l.n > c->max_slices) { g_last_error = std::string(fn) + ": more blocks than the context's max_slices"; return KMP_ERR_CAPACITY; }
    if (scratch_bytes < l.total) { g_last_error = std::string(fn) + ": scratch_bytes below kmp_bgzf_scratch"; return KMP_ERR_CAPACITY; }
    if (dst_cap < kmp_bgzf_bound(src_size, block_bytes, flags)) { g_last_error = std::string(fn) + ": dst_cap below kmp_bgzf_bound"; return KMP_ERR_CAPACITY; }
    hipStream_t const st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(c->device));
    u8* const s = (u8*)d_scratch; u32 const n = (u32)l.n;
    u64* const in_off = (u64*)(s + l.in_off); u64* const out_off = (u64*)(s + l.out_off); u64* const dense_off = (u64*)(s + l.dense_off);
    u32* const in_len = (u32*)(s + l.in_len); u32* const out_len = (u32*)(s + l.out_len);
    if (n) {
        KSeekPlanArgs const p = { (u64)src_size, block_bytes, n, l.stride, in_off, in_len, out_off };
        hipLaunchKernelGGL(k_bgzf_plan, dim3((n + 255u) / 256u), dim3(256), 0, st, p);
        HIP_TRY(hipGetLastError());
        // the payloads land KBZ_HEAD bytes into their stride slots: the header goes in front of them where they lie
        KMP_TRY(kmp_deflate_compress_batch_level(c, d_src, in_off, in_len, n, s + l.frames + KBZ_HEAD, out_off, out_len, 0, level, hip_stream));
        KBgzfWrapArgs const w = { (const u8*)d_src, in_off, in_len, s + l.frames, out_off, out_len, n };
        hipLaunchKernelGGL(k_bgzf_wrap, dim3(n), dim3(64), 0, st, w);
        HIP_TRY(hipGetLastError());
        KMP_TRY(kmp_compact_batch(c, s + l.frames, out_off, out_len, n, d_dst, dense_off, hip_stream));
    }
    KBgzfFinishArgs const f = { (u8*)d_dst, dense_off, out_len, n, flags, c->d_status, d_result };
    hipLaunchKernelGGL(k_bgzf_finish, dim3(1), dim3(256), 0, st, f);
    HIP_TRY(hipGetLastError());
    return KMP_OK;
}

// ---- reading -----------------------------------------------------------------------------------------------------------------------
// The prefix sums on the host find a range's covering members without a read-back.  The device arrays are the ABSOLUTE positions of every
// member's payload in the blob and of its content in the container's content, written once by the open's last kernel: a read passes
// kmp_inflate_batch the slice of them that covers its range and a destination base moved back by the first covering member's start.
struct kmp_bgzf {
    kmp_batch_ctx* ctx = nullptr; kmp_bgzf_stat st = {};
    std::vector<u64> member_off, content_off;                  // blocks + 1 entries each
    dev_buf<u64> d_member_off, d_content_off, d_in_off; dev_buf<u32> d_in_len, d_out_cap, d_out_len; dev_buf<kmp_bgzf_stat> d_stat;
};

extern "C" int kmp_bgzf_index_host(const void* h_blob, size_t blob_size, kmp_bgzf_stat* stat, uint64_t* member_off, uint64_t* content_off, size_t prefix_cap)
{
    if (!stat || (blob_size && !h_blob)) { g_last_error = "kmp_bgzf_index_host: null argument"; return KMP_ERR_ARG; }
    kx_bgzf_walk((const u8*)h_blob, blob_size, stat, nullptr, nullptr, 0);
    if (stat->status == 0 && prefix_cap >= (size_t)stat->blocks + 1u && (member_off || content_off))
        kx_bgzf_walk((const u8*)h_blob, blob_size, stat, member_off, content_off, prefix_cap);
    return KMP_OK;
}

static int bgzf_alloc_arrays(kmp_bgzf* h, size_t n)
{
    const char* const what = "kmp_bgzf_open: hipMalloc";
    KMP_TRY(h->d_member_off.alloc((n + 1) * 8, what)); KMP_TRY(h->d_content_off.alloc((n + 1) * 8, what)); KMP_TRY(h->d_in_off.alloc((n + 1) * 8, what));
    KMP_TRY(h->d_in_len.alloc((n + 1) * 4, what)); KMP_TRY(h->d_out_cap.alloc((n + 1) * 4, what)); KMP_TRY(h->d_out_len.alloc((n + 1) * 4, what));
    return KMP_OK;
}
// the stat and, for a good blob, both prefix arrays (room for `room` + 1 entries, of which blocks + 1 count) come back: one wait
static int bgzf_fetch(kmp_bgzf* h, size_t room, hipStream_t st)
{
    h->member_off.assign(room + 1, 0); h->content_off.assign(room + 1, 0);
    HIP_TRY(hipMemcpyAsync(&h->st, h->d_stat.p, sizeof(kmp_bgzf_stat), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h->member_off.data(), h->d_member_off.p, (room + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h->content_off.data(), h->d_content_off.p, (room + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    size_t const keep = h->st.status == 0 ? (size_t)h->st.blocks + 1u : 0u;
    h->member_off.resize(keep); h->content_off.resize(keep);
    return KMP_OK;
}

// the serial open: k_bgzf_walk once for the stat (the first wait), once more into arrays of the size it found (the second)
static int bgzf_open_walk(kmp_bgzf* h, const u8* blob, u64 size, hipStream_t st)
{
    KBgzfArrays const none = { nullptr, nullptr, nullptr };
    hipLaunchKernelGGL(k_bgzf_walk, dim3(1), dim3(64), 0, st, blob, size, h->d_stat.p, (u64*)nullptr, (u64*)nullptr, (u64)0, none);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h->st, h->d_stat.p, sizeof(kmp_bgzf_stat), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h->st.status != 0) return KMP_OK;
    size_t const n = h->st.blocks;
    KMP_TRY(bgzf_alloc_arrays(h, n));
    KBgzfArrays const arr = { h->d_in_off.p, h->d_in_len.p, h->d_out_cap.p };
    hipLaunchKernelGGL(k_bgzf_walk, dim3(1), dim3(64), 0, st, blob, size, h->d_stat.p, h->d_member_off.p, h->d_content_off.p, (u64)n + 1u, arr);
    HIP_TRY(hipGetLastError());
    return bgzf_fetch(h, n, st);
}

// max_candidates: KBZ_MAX_CANDIDATES (a policy constant: the doubling tables are 4 bytes x candidates x levels)
static int bgzf_open_impl(kmp_batch_ctx* c, const void* d_blob, size_t blob_size, kmp_bgzf** out, hipStream_t st, u32 max_candidates)
{
    const char* const what = "kmp_bgzf_open: hipMalloc";
    std::unique_ptr<kmp_bgzf> h(new (std::nothrow) kmp_bgzf());
    if (!h) { g_last_error = "out of host memory"; return KMP_ERR_HIP; }
    h->ctx = c;
    KMP_TRY(h->d_stat.alloc(sizeof(kmp_bgzf_stat), what));
    const u8* const blob = (const u8*)d_blob; u64 const size = blob_size;
    if (size == 0 || (size >> 36) != 0 || max_candidates == 0) {
        KMP_TRY(bgzf_open_walk(h.get(), blob, size, st));
        *out = h.release();
        return KMP_OK;
    }
    // count: a wave per tile, then the tiles' exclusive scan; the total is the first wait
    u64 const ntiles = (size + KBZ_TILE - 1u) / KBZ_TILE;
    dev_buf<u32> tiles;
    KMP_TRY(tiles.alloc((size_t)(ntiles + 1u) * 4, what));
    u32 const scan_grid = grid_for(ntiles, 4, 16384);
    KBgzfScanArgs sc = { blob, size, ntiles, tiles.p, nullptr, nullptr };
    hipLaunchKernelGGL(k_bgzf_scan, dim3(scan_grid), dim3(256), 0, st, sc);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_bgzf_prefix, dim3(1), dim3(1024), 0, st, tiles.p, ntiles);
    HIP_TRY(hipGetLastError());
    u32 n = 0;
    HIP_TRY(hipMemcpyAsync(&n, tiles.p + ntiles, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n > max_candidates) {
        KMP_TRY(bgzf_open_walk(h.get(), blob, size, st));
        *out = h.release();
        return KMP_OK;
    }
    u32 levels = 0;
    while (levels < 32u && (1ull << levels) < n) levels++;                   // ceil(log2 n); 0 for n <= 1
    dev_buf<KBgzfCand> cand; dev_buf<u32> jump, mark;
    KMP_TRY(bgzf_alloc_arrays(h.get(), n));
    if (n) {
        KMP_TRY(cand.alloc((size_t)n * sizeof(KBgzfCand), what));
        KMP_TRY(jump.alloc((size_t)n * 4 * (levels ? levels : 1u), what));
        KMP_TRY(mark.alloc((size_t)n * 4, what));
        sc.tile_base = tiles.p; sc.cand = cand.p;
        hipLaunchKernelGGL(k_bgzf_scan, dim3(scan_grid), dim3(256), 0, st, sc);
        HIP_TRY(hipGetLastError());
        u32 const grid = grid_for(n, 256, 4096);
        KBgzfLinkArgs const lk = { cand.p, n, size, jump.p, mark.p };
        hipLaunchKernelGGL(k_bgzf_link, dim3(grid), dim3(256), 0, st, lk);
        HIP_TRY(hipGetLastError());
        for (u32 k = 1; k < levels; k++) {
            hipLaunchKernelGGL(k_bgzf_double, dim3(grid), dim3(256), 0, st, (const u32*)(jump.p + (size_t)(k - 1u) * n), jump.p + (size_t)k * n, n);
            HIP_TRY(hipGetLastError());
        }
        for (u32 k = levels; k-- > 0;) {
            hipLaunchKernelGGL(k_bgzf_mark, dim3(grid), dim3(256), 0, st, (const u32*)(jump.p + (size_t)k * n), mark.p, n);
            HIP_TRY(hipGetLastError());
        }
    }
    KBgzfGatherArgs const g = { blob, size, cand.p, jump.p, mark.p, n, h->d_member_off.p, h->d_content_off.p,
                                { h->d_in_off.p, h->d_in_len.p, h->d_out_cap.p }, h->d_stat.p };
    hipLaunchKernelGGL(k_bgzf_gather, dim3(1), dim3(1024), 0, st, g);
    HIP_TRY(hipGetLastError());
    KMP_TRY(bgzf_fetch(h.get(), n, st));             // the second wait (the open's tables are freed behind it)
    *out = h.release();
    return KMP_OK;
}

extern "C" int kmp_bgzf_open(kmp_batch_ctx* c, const void* d_blob, size_t blob_size, kmp_bgzf** out, void* hip_stream)
{
    if (!c || !out || (blob_size && !d_blob)) { g_last_error = "kmp_bgzf_open: null argument"; return KMP_ERR_ARG; }
    *out = nullptr;
    HIP_TRY(hipSetDevice(c->device));
    return bgzf_open_impl(c, d_blob, blob_size, out, (hipStream_t)hip_stream, KMP_KNOB("KMP_BGZF_MAX_CANDIDATES", KBZ_MAX_CANDIDATES));
}
extern "C" void kmp_bgzf_close(kmp_bgzf* h)
{
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    (void)hipDeviceSynchronize();             // (a read may still be using the handle's arrays)
    delete h;
}
extern "C" int kmp_bgzf_stat_of(const kmp_bgzf* h, kmp_bgzf_stat* stat)
{
    if (!h || !stat) { g_last_error = "kmp_bgzf_stat_of: null argument"; return KMP_ERR_ARG; }
    *stat = h->st;
    return KMP_OK;
}

// the members that cover [lo, hi) of the content: first .. last, or false for an empty range (empty members in front of the range or
// behind it are left out; one inside it is kept: it decodes to nothing)
static bool bgzf_cover(const kmp_bgzf* h, u64 lo, u64 hi, u32* first, u32* last)
{
    if (!h || h->st.status != 0 || h->st.blocks == 0) return false;
    if (hi > h->st.content) hi = h->st.content;
    if (lo >= hi) return false;
    auto const b = h->content_off.begin(), e = h->content_off.end();
    *first = (u32)(std::upper_bound(b, e, lo) - b) - 1u;
    *last = (u32)(std::lower_bound(b, e, hi) - b) - 1u;
    return true;
}
extern "C" size_t kmp_bgzf_read_bound(const kmp_bgzf* h, uint64_t lo, uint64_t hi)
{
    u32 first, last;
    return bgzf_cover(h, lo, hi, &first, &last) ? (size_t)(h->content_off[(size_t)last + 1] - h->content_off[first]) : 0;
}
extern "C" uint32_t kmp_bgzf_read_blocks(const kmp_bgzf* h, uint64_t lo, uint64_t hi, uint32_t* first_out)
{
    u32 first, last;
    if (!bgzf_cover(h, lo, hi, &first, &last)) return 0;
    if (first_out) *first_out = first;
    return last - first + 1u;
}
extern "C" uint64_t kmp_bgzf_tell(const kmp_bgzf* h, uint64_t content_pos)
{
    if (!h || h->st.status != 0 || content_pos > h->st.content) return ~0ull;
    auto const b = h->content_off.begin(), e = h->content_off.end();
    size_t const i = (size_t)(std::upper_bound(b, e, content_pos) - b) - 1u;
    return (h->member_off[i] << 16) | (content_pos - h->content_off[i]);
}
extern "C" int kmp_bgzf_read(kmp_bgzf* h, const void* d_blob, uint64_t lo, uint64_t hi, int verify, void* d_dst, size_t dst_cap,
                             uint64_t* skip, int32_t* d_status, void* hip_stream)
{
    const char* const fn = "kmp_bgzf_read";
    if (!h || !skip) { g_last_error = std::string(fn) + ": null argument"; return KMP_ERR_ARG; }
    if (h->st.status != 0) { g_last_error = std::string(fn) + ": the blob was rejected (kmp_bgzf_stat_of)"; return KMP_ERR_ARG; }
    *skip = 0;
    u32 first, last;
    if (!bgzf_cover(h, lo, hi, &first, &last)) return KMP_OK;
    if (!d_blob || !d_dst || !d_status) { g_last_error = std::string(fn) + ": null argument"; return KMP_ERR_ARG; }
    u64 const start = h->content_off[first];
    if (dst_cap < h->content_off[(size_t)last + 1] - start) { g_last_error = std::string(fn) + ": dst_cap below kmp_bgzf_read_bound"; return KMP_ERR_CAPACITY; }
    kmp_batch_ctx* const c = h->ctx;
    HIP_TRY(hipSetDevice(c->device));
    u8* const base = (u8*)d_dst - start;              // (only base + content_off[i], i >= first, is ever formed into an access)
    u32 const m = last - first + 1u;
    for (u32 r = 0; r < m; r += c->max_slices) {
        u32 const k = m - r < c->max_slices ? m - r : c->max_slices; size_t const at = (size_t)first + r;
        KMP_TRY(kmp_inflate_batch(c, d_blob, h->d_in_off.p + at, h->d_in_len.p + at, k, base, h->d_content_off.p + at, h->d_out_cap.p + at,
                                  h->d_out_len.p + at, d_status + r, 0, hip_stream));
        KBgzfVerifyArgs const v = { (const u8*)d_blob, h->d_in_off.p + at, h->d_in_len.p + at, base, h->d_content_off.p + at, h->d_out_len.p + at,
                                    h->d_out_cap.p + at, d_status + r, k, verify ? 1u : 0u };
        hipLaunchKernelGGL(k_bgzf_verify, dim3(k), dim3(64), 0, (hipStream_t)hip_stream, v);
        HIP_TRY(hipGetLastError());
    }
    *skip = lo - start;
    return KMP_OK;
}
