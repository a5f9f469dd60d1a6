// kmp_seekable.hip -- the host half of zstd's seekable container (zstd_seekable.h): kmp_zstd_seekable_*.  A container is made of calls the
// library already has -- kmp_zstd_compress_batch_level over the chunks, kmp_compact_batch to pack the frames, kmp_zstd_decompress_batch
// over the covering frames of a read -- with this unit's kernels around them: the plan, XXH64 of every chunk / decoded frame, the table
// and its validation.  The context allocates nothing here: compress works in the caller's scratch, a reader's arrays belong to its handle.
#include "kx_wave.h"
#include "zstd_seekable.h"
#include "kmp_internal.h"

#include <algorithm>
#include <vector>

__global__ __launch_bounds__(256) void k_seekable_plan(KSeekPlanArgs a) { seekable_plan_body(a); }
__global__ __launch_bounds__(256) void k_seekable_xxh64(KSeekXxhArgs a) { seekable_xxh64_body(a); }
__global__ __launch_bounds__(256) void k_seekable_table(KSeekTableArgs a) { seekable_table_body(a); }
__global__ __launch_bounds__(64) void k_seekable_index(const u8* blob, u64 size, kmp_seekable_stat* out) { seekable_index_body(blob, size, out); }

// XXH64 of n pieces on `st`: a workgroup of four waves takes 64 pieces at a time (zstd_seekable.h)
static int launch_xxh64(hipStream_t st, KSeekXxhArgs const& a)
{
    u32 const blocks = (a.n + 63u) / 64u;
    hipLaunchKernelGGL(k_seekable_xxh64, dim3(blocks < 8192u ? blocks : 8192u), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return KMP_OK;
}

// ---- the caller's scratch: six arrays over the n chunks, then the frames at `stride` -----------------------------------------------
struct seek_layout { u64 n, stride, in_off, out_off, dense_off, in_len, out_len, cks, frames, total; };
static bool seek_frame_bytes_ok(u32 frame_bytes) { return frame_bytes >= 1u && frame_bytes <= KMP_MAX_SLICE_BYTES; }
static seek_layout seek_scratch_layout(size_t src_size, u32 frame_bytes)
{
    seek_layout l;
    l.n = ((u64)src_size + frame_bytes - 1u) / frame_bytes;
    l.stride = ((u64)kmp_zstd_compress_bound(frame_bytes) + 8u + 63u) & ~63ull;
    l.in_off = 0; l.out_off = l.in_off + 8u * l.n; l.dense_off = l.out_off + 8u * l.n;
    l.in_len = l.dense_off + 8u * (l.n + 1u); l.out_len = l.in_len + 4u * l.n; l.cks = l.out_len + 4u * l.n;
    l.frames = (l.cks + 4u * l.n + 63u) & ~63ull;
    l.total = l.frames + l.n * l.stride + 64u;
    return l;
}

extern "C" size_t kmp_zstd_seekable_bound(size_t src_size, uint32_t frame_bytes, uint32_t flags)
{
    if (!seek_frame_bytes_ok(frame_bytes)) return 0;
    u64 const n = ((u64)src_size + frame_bytes - 1u) / frame_bytes;
    u64 const last = n ? (u64)src_size - (n - 1u) * frame_bytes : 0u;
    return (size_t)((n ? (n - 1u) * kmp_zstd_compress_bound(frame_bytes) + kmp_zstd_compress_bound((size_t)last) : 0u) + ksk_table_bytes(n, flags & KMP_SEEKABLE_CHECKSUMS));
}
extern "C" size_t kmp_zstd_seekable_scratch(size_t src_size, uint32_t frame_bytes)
{
    return seek_frame_bytes_ok(frame_bytes) ? (size_t)seek_scratch_layout(src_size, frame_bytes).total : 0;
}

extern "C" int kmp_zstd_seekable_compress(kmp_batch_ctx* c, const void* d_src, size_t src_size, uint32_t frame_bytes, int level, uint32_t flags,
                                          void* d_dst, size_t dst_cap, void* d_scratch, size_t scratch_bytes, uint64_t* d_result, void* hip_stream)
{
    const char* const fn = "kmp_zstd_seekable_compress";
    if (!c || !d_dst || !d_scratch || !d_result || (src_size && !d_src)) { g_last_error = std::string(fn) + ": null argument"; return KMP_ERR_ARG; }
    if (!seek_frame_bytes_ok(frame_bytes)) { g_last_error = std::string(fn) + ": frame_bytes must be 1 .. 131072"; return KMP_ERR_ARG; }
    if (level > 8 || level < -131072) { g_last_error = std::string(fn) + ": levels -131072 .. 8 are served (9 and 10 refuse a short last chunk)"; return KMP_ERR_ARG; }
    if (flags & ~KMP_SEEKABLE_CHECKSUMS) { g_last_error = std::string(fn) + ": unknown flag"; return KMP_ERR_ARG; }
    if (((uintptr_t)d_scratch | (uintptr_t)d_result) & 7u) { g_last_error = std::string(fn) + ": d_scratch and d_result must be 8-byte aligned"; return KMP_ERR_ARG; }
    if (frame_bytes > c->max_slice_bytes) { g_last_error = std::string(fn) + ": frame_bytes exceeds the context's max_slice_bytes"; return KMP_ERR_CAPACITY; }
    seek_layout const l = seek_scratch_layout(src_size, frame_bytes);
    if (l.n > c->max_slices) { g_last_error = std::string(fn) + ": more chunks than the context's max_slices"; return KMP_ERR_CAPACITY; }
    if (scratch_bytes < l.total) { g_last_error = std::string(fn) + ": scratch_bytes below kmp_zstd_seekable_scratch"; return KMP_ERR_CAPACITY; }
    if (dst_cap < kmp_zstd_seekable_bound(src_size, frame_bytes, flags)) { g_last_error = std::string(fn) + ": dst_cap below kmp_zstd_seekable_bound"; return KMP_ERR_CAPACITY; }
    hipStream_t const st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(c->device));
    u8* const s = (u8*)d_scratch; u32 const n = (u32)l.n;
    u64* const in_off = (u64*)(s + l.in_off); u64* const out_off = (u64*)(s + l.out_off); u64* const dense_off = (u64*)(s + l.dense_off);
    u32* const in_len = (u32*)(s + l.in_len); u32* const out_len = (u32*)(s + l.out_len); u32* const cks = (u32*)(s + l.cks);
    if (n) {
        KSeekPlanArgs const p = { (u64)src_size, frame_bytes, n, l.stride, in_off, in_len, out_off };
        hipLaunchKernelGGL(k_seekable_plan, dim3((n + 255u) / 256u), dim3(256), 0, st, p);
        HIP_TRY(hipGetLastError());
        if (flags & KMP_SEEKABLE_CHECKSUMS) {
            KSeekXxhArgs const x = { (const u8*)d_src, in_off, in_len, n, cks, nullptr, nullptr };
            KMP_TRY(launch_xxh64(st, x));
        }
        // (the container's frames stay as the format specifies them, whatever kmp_batch_set_frame_flags has left on the context)
        u32 const held = c->frame_flags; c->frame_flags = 0;
        int const rc = kmp_zstd_compress_batch_level(c, d_src, in_off, in_len, n, s + l.frames, out_off, out_len, level, hip_stream);
        c->frame_flags = held;
        KMP_TRY(rc);
        KMP_TRY(kmp_compact_batch(c, s + l.frames, out_off, out_len, n, d_dst, dense_off, hip_stream));
    }
    KSeekTableArgs const t = { (u8*)d_dst, dense_off, out_len, in_len, cks, n, flags & KMP_SEEKABLE_CHECKSUMS, c->d_status, d_result };
    hipLaunchKernelGGL(k_seekable_table, dim3(1), dim3(256), 0, st, t);
    HIP_TRY(hipGetLastError());
    return KMP_OK;
}

// ---- reading -----------------------------------------------------------------------------------------------------------------------
// The prefix sums on the host find a range's covering frames without a read-back.  The device arrays are the ABSOLUTE positions of every
// frame -- in the blob, and in the container's content --, written once: a read passes kmp_zstd_decompress_batch the slice of them that
// covers its range and a destination base moved back by the first covering frame's start, so frame `first` lands at d_dst[0].
struct kmp_seekable {
    kmp_batch_ctx* ctx = nullptr; kmp_seekable_stat st = {};
    std::vector<u64> frame_off, content_off;                   // frames + 1 entries each
    dev_buf<u64> d_in_off, d_out_off; dev_buf<u32> d_in_len, d_out_cap, d_out_len; dev_buf<kmp_seekable_stat> d_stat;
    std::vector<u32> h_len, h_cap;
};
enum { KSK_TAIL_GUESS = 256 * 1024 };

// entries -> prefix sums; the entries were validated (their sums fit 64 bits: 2^27 entries of 32 bits each)
static void seek_prefix(const u8* entries, u32 n, u32 eb, u64* frame_off, u64* content_off, u32* len, u32* cap)
{
    u64 c = 0, d = 0;
    for (u32 i = 0; i < n; i++, entries += eb) {
        u32 const cs = zf_ld32(entries), ds = zf_ld32(entries + 4);
        if (frame_off) frame_off[i] = c;
        if (content_off) content_off[i] = d;
        if (len) len[i] = cs;
        if (cap) cap[i] = ds;
        c += cs; d += ds;
    }
    if (frame_off) frame_off[n] = c;
    if (content_off) content_off[n] = d;
}

extern "C" int kmp_zstd_seekable_index_host(const void* h_blob, size_t blob_size, kmp_seekable_stat* stat, uint64_t* frame_off, uint64_t* content_off, size_t prefix_cap)
{
    if (!stat || (blob_size && !h_blob)) { g_last_error = "kmp_zstd_seekable_index_host: null argument"; return KMP_ERR_ARG; }
    kx_seekable_index((const u8*)h_blob, blob_size, stat);
    if (stat->status == 0 && prefix_cap >= (size_t)stat->frames + 1u && (frame_off || content_off))
        seek_prefix((const u8*)h_blob + stat->table_off + KSK_HEADER, stat->frames, ksk_entry_bytes(stat->flags), frame_off, content_off, nullptr, nullptr);
    return KMP_OK;
}

extern "C" int kmp_zstd_seekable_open(kmp_batch_ctx* c, const void* d_blob, size_t blob_size, kmp_seekable** out, void* hip_stream)
{
    if (!c || !out || (blob_size && !d_blob)) { g_last_error = "kmp_zstd_seekable_open: null argument"; return KMP_ERR_ARG; }
    *out = nullptr;
    hipStream_t const st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(c->device));
    std::unique_ptr<kmp_seekable> h(new (std::nothrow) kmp_seekable());
    if (!h) { g_last_error = "out of host memory"; return KMP_ERR_HIP; }
    h->ctx = c;
    KMP_TRY(h->d_stat.alloc(sizeof(kmp_seekable_stat), "kmp_zstd_seekable_open: hipMalloc"));
    hipLaunchKernelGGL(k_seekable_index, dim3(1), dim3(64), 0, st, (const u8*)d_blob, (u64)blob_size, h->d_stat.p);
    HIP_TRY(hipGetLastError());
    // the one wait: the device's answer and, with it, the blob's tail, where the table is unless it is a large one
    size_t const guess = blob_size < (size_t)KSK_TAIL_GUESS ? blob_size : (size_t)KSK_TAIL_GUESS;
    std::vector<u8> tail(guess ? guess : 1);
    HIP_TRY(hipMemcpyAsync(&h->st, h->d_stat.p, sizeof(kmp_seekable_stat), hipMemcpyDeviceToHost, st));
    if (guess) HIP_TRY(hipMemcpyAsync(tail.data(), (const u8*)d_blob + (blob_size - guess), guess, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (h->st.status == 0) {
        u32 const n = h->st.frames, eb = ksk_entry_bytes(h->st.flags);
        size_t const table = (size_t)ksk_table_bytes(n, h->st.flags);          // (<= blob_size: the device checked it)
        if (table > guess) {
            tail.resize(table);
            HIP_TRY(hipMemcpy(tail.data(), (const u8*)d_blob + h->st.table_off, table, hipMemcpyDeviceToHost));
        }
        const u8* const entries = tail.data() + (tail.size() - table) + KSK_HEADER;
        h->frame_off.resize((size_t)n + 1); h->content_off.resize((size_t)n + 1); h->h_len.resize(n); h->h_cap.resize(n);
        seek_prefix(entries, n, eb, h->frame_off.data(), h->content_off.data(), h->h_len.data(), h->h_cap.data());
        if (n) {
            const char* const what = "kmp_zstd_seekable_open: hipMalloc";
            KMP_TRY(h->d_in_off.alloc((size_t)n * 8, what)); KMP_TRY(h->d_out_off.alloc((size_t)n * 8, what));
            KMP_TRY(h->d_in_len.alloc((size_t)n * 4, what)); KMP_TRY(h->d_out_cap.alloc((size_t)n * 4, what)); KMP_TRY(h->d_out_len.alloc((size_t)n * 4, what));
            HIP_TRY(hipMemcpyAsync(h->d_in_off.p, h->frame_off.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(h->d_out_off.p, h->content_off.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(h->d_in_len.p, h->h_len.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(h->d_out_cap.p, h->h_cap.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        }
    }
    *out = h.release();
    return KMP_OK;
}
extern "C" void kmp_zstd_seekable_close(kmp_seekable* h)
{
    if (!h) return;
    (void)hipSetDevice(h->ctx->device);
    (void)hipDeviceSynchronize();             // (a read may still be using the handle's arrays)
    delete h;
}
extern "C" int kmp_zstd_seekable_stat(const kmp_seekable* h, kmp_seekable_stat* stat)
{
    if (!h || !stat) { g_last_error = "kmp_zstd_seekable_stat: null argument"; return KMP_ERR_ARG; }
    *stat = h->st;
    return KMP_OK;
}

// the frames that cover [lo, hi) of the content: first .. last, or false for an empty range (entries of no content in front of the
// range or behind it are left out; one inside it is kept: it decodes to nothing)
static bool seek_cover(const kmp_seekable* h, u64 lo, u64 hi, u32* first, u32* last)
{
    if (!h || h->st.status != 0 || h->st.frames == 0) return false;
    if (hi > h->st.content) hi = h->st.content;
    if (lo >= hi) return false;
    auto const b = h->content_off.begin(), e = h->content_off.end();
    *first = (u32)(std::upper_bound(b, e, lo) - b) - 1u;
    *last = (u32)(std::lower_bound(b, e, hi) - b) - 1u;
    return true;
}
extern "C" size_t kmp_zstd_seekable_read_bound(const kmp_seekable* h, uint64_t lo, uint64_t hi)
{
    u32 first, last;
    return seek_cover(h, lo, hi, &first, &last) ? (size_t)(h->content_off[(size_t)last + 1] - h->content_off[first]) : 0;
}
extern "C" uint32_t kmp_zstd_seekable_read_frames(const kmp_seekable* h, uint64_t lo, uint64_t hi, uint32_t* first_out)
{
    u32 first, last;
    if (!seek_cover(h, lo, hi, &first, &last)) return 0;
    if (first_out) *first_out = first;
    return last - first + 1u;
}
extern "C" int kmp_zstd_seekable_read(kmp_seekable* h, const void* d_blob, uint64_t lo, uint64_t hi, int verify, void* d_dst, size_t dst_cap,
                                      uint64_t* skip, uint32_t* d_status, void* hip_stream)
{
    const char* const fn = "kmp_zstd_seekable_read";
    if (!h || !skip) { g_last_error = std::string(fn) + ": null argument"; return KMP_ERR_ARG; }
    if (h->st.status != 0) { g_last_error = std::string(fn) + ": the container's table was rejected (kmp_zstd_seekable_stat)"; return KMP_ERR_ARG; }
    *skip = 0;
    u32 first, last;
    if (!seek_cover(h, lo, hi, &first, &last)) return KMP_OK;
    if (!d_blob || !d_dst || !d_status) { g_last_error = std::string(fn) + ": null argument"; return KMP_ERR_ARG; }
    u64 const start = h->content_off[first];
    if (dst_cap < h->content_off[(size_t)last + 1] - start) { g_last_error = std::string(fn) + ": dst_cap below kmp_zstd_seekable_read_bound"; return KMP_ERR_CAPACITY; }
    kmp_batch_ctx* const c = h->ctx;
    HIP_TRY(hipSetDevice(c->device));
    u8* const base = (u8*)d_dst - start;              // (only base + content_off[i], i >= first, is ever formed into an access)
    u32 const m = last - first + 1u;
    bool const sums = verify && (h->st.flags & KMP_SEEKABLE_CHECKSUMS);
    for (u32 r = 0; r < m; r += c->max_slices) {
        u32 const k = m - r < c->max_slices ? m - r : c->max_slices; size_t const at = (size_t)first + r;
        KMP_TRY(kmp_zstd_decompress_batch(c, d_blob, h->d_in_off.p + at, h->d_in_len.p + at, k, base, h->d_out_off.p + at, h->d_out_cap.p + at,
                                          h->d_out_len.p + at, d_status + r, hip_stream));
        if (sums) {
            KSeekXxhArgs const x = { base, h->d_out_off.p + at, h->d_out_len.p + at, k, nullptr,
                                     (const u8*)d_blob + h->st.table_off + KSK_HEADER + 12ull * at, d_status + r };
            KMP_TRY(launch_xxh64((hipStream_t)hip_stream, x));
        }
    }
    *skip = lo - start;
    return KMP_OK;
}
