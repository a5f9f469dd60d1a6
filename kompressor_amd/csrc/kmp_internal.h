// kmp_internal.h -- what the translation units of libkompressor_hip.so share: the batch context, the error helpers, the
// knob macros and the few host functions one unit calls in another.  Nothing here is part of the C ABI
// (include/kompressor_hip.h); everything is built with hidden visibility.
//
//   kmp_batch.hip    zstd kernels, the batch context, kmp_zstd_{compress,decompress}_batch*, kmp_compact_batch
//   kmp_deflate.hip  DEFLATE / inflate kernels, kmp_deflate_* / kmp_zlib_* / kmp_gzip_compress_batch, kmp_inflate_batch
//   kmp_stream.hip   the streaming-compatible single-slice API (one function per JNI export of the reference) and the
//                    host-memory batch (kmp_coalesce.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include "../../include/kompressor_hip.h"

typedef uint8_t  u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;

struct KSeq; struct KSliceMeta; struct KFrameState; struct KdBest; struct KdSliceMeta; struct KdBlockInfo; struct KPreBlk; struct KPreLit;
struct KDictPrior; struct KDictDPrior; struct KSeqPrev;

// --------------------------------------------------------------------------
// errors
// --------------------------------------------------------------------------
extern thread_local std::string g_last_error;
int hip_fail(hipError_t e, const char* what);
#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return hip_fail(e_, #x); } while (0)
#define KMP_TRY(x) do { int r_ = (x); if (r_ != KMP_OK) return r_; } while (0)

// --------------------------------------------------------------------------
// knobs
// --------------------------------------------------------------------------
// The product reads a short, documented list of environment variables (INTEGRATION.md "Environment"): env_u32.  Everything
// that only ever served an experiment or an ablation is a KMP_KNOB: a compile-time constant in the product build (the
// variable's name does not even reach the binary) and an environment variable in the ablation build
// (-DKMP_ABLATIONS: libkompressor_hip_abl.so, which the tests of those paths load).
u32 env_u32(const char* name, u32 dflt);
#ifdef KMP_ABLATIONS
#define KMP_KNOB(name, dflt) env_u32(name, (u32)(dflt))
#else
#define KMP_KNOB(name, dflt) ((u32)(dflt))
#endif

// --------------------------------------------------------------------------
// owners of device resources
// --------------------------------------------------------------------------
// Move-only owners, the only code that frees device or pinned memory, events and streams.  A buffer records its byte count and
// converts to its pointer (the kernels' argument structs take plain views).  alloc / create release what the owner held, then
// return KMP_OK or KMP_ERR_HIP (the sticky HIP error cleared; g_last_error set unless `what` is null: an allocation allowed to fail).
template <class T, bool Pinned> struct kmp_buf {
    T* p = nullptr; size_t bytes = 0;
    kmp_buf() = default;
    kmp_buf(kmp_buf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    kmp_buf& operator=(kmp_buf o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }
    ~kmp_buf() { reset(); }
    void reset() { if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p)); p = nullptr; bytes = 0; }
    int alloc(size_t n, const char* what = nullptr)
    {
        reset();
        hipError_t const e = Pinned ? hipHostMalloc((void**)&p, n) : hipMalloc((void**)&p, n);
        if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); return what ? hip_fail(e, what) : KMP_ERR_HIP; }
        bytes = n;
        return KMP_OK;
    }
    operator T*() const { return p; }
};
template <class T> using dev_buf = kmp_buf<T, false>;
template <class T> using pinned_buf = kmp_buf<T, true>;
template <class H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)> struct kmp_handle {
    H h = nullptr;
    kmp_handle() = default;
    kmp_handle(kmp_handle&& o) noexcept : h(o.h) { o.h = nullptr; }
    kmp_handle& operator=(kmp_handle o) noexcept { std::swap(h, o.h); return *this; }
    ~kmp_handle() { if (h) (void)Destroy(h); }
    int create(unsigned flags)
    {
        hipError_t const e = Create(&h, flags);       // (on an empty owner)
        if (e != hipSuccess) { h = nullptr; (void)hipGetLastError(); return hip_fail(e, "creating a HIP event / stream"); }
        return KMP_OK;
    }
    operator H() const { return h; }
};
using hip_event = kmp_handle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
using hip_stream = kmp_handle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

// The sets a context adds on first use are parts: absent or complete.  build_part makes one locally and moves it into `slot` only
// when `fill` -- every allocation and clear of the part -- has succeeded; otherwise the slot stays empty and whatever fill
// allocated is freed.  The ablation build's KMP_TEST_FAIL_PART=<code> fails the named part once fill has succeeded: what a
// failing last allocation would leave (the earlier ones made, then freed), without a switch in the owners.
enum { KMP_PART_DEFLATE_LAZY = 1, KMP_PART_DEFLATE_FAST, KMP_PART_LAZY_LEVELS, KMP_PART_DICT, KMP_PART_FLAT_TABLES, KMP_PART_TABLES4,
       KMP_PART_CHAIN_TABLES4, KMP_PART_DDICT, KMP_PART_PRE_SEQ, KMP_PART_PRE_LIT, KMP_PART_LAZY_BIG };
template <class P, class F> int build_part(std::unique_ptr<P>& slot, u32 code, F const& fill)
{
    std::unique_ptr<P> p(new (std::nothrow) P());
    if (!p) { g_last_error = "out of host memory"; return KMP_ERR_HIP; }
    KMP_TRY(fill(*p));
#ifdef KMP_ABLATIONS
    if (KMP_KNOB("KMP_TEST_FAIL_PART", 0) == code) return hip_fail(hipErrorOutOfMemory, "KMP_TEST_FAIL_PART");
#else
    (void)code;
#endif
    slot = std::move(p);
    return KMP_OK;
}
template <class P> size_t part_bytes(std::unique_ptr<P> const& p) { return p ? p->bytes() : 0; }

// parser tables (+ team epochs): levels 1 / 2 and the dictionary parser (one piece, when the level-3 tables are spread), level 4
// (1 MiB per team), level 4 on the block-chain path (2 MiB per slice, no epochs)
struct table_part { dev_buf<u32> tables, epochs; u32 teams = 0; size_t bytes() const { return tables.bytes + epochs.bytes; } };
// zstd levels 5 .. 10 (and level 4 up to 16 KiB): the sorted positions (KLazyRec), where each stands, the parse order (optional)
struct lazy_part { dev_buf<u32> srt, wr, order; u32 pos_cap = 0, chunk = 0; size_t bytes() const { return srt.bytes + wr.bytes + order.bytes; } };
// zstd levels 5 .. 10 over frames of several blocks (zstd_lazy_big.h): libzstd's row table and tags for `chunk` slices in flight (slot_bytes
// each), their previous sequence tables; for the whole batch: the lengths the one-block kernels see (a larger slice reads as empty there)
struct lazy_big_part {
    dev_buf<u8> tables; dev_buf<KSeqPrev> prev; dev_buf<u32> small_len; u32 chunk = 0; u64 slot_bytes = 0;
    size_t bytes() const { return tables.bytes + prev.bytes + small_len.bytes; }
};
// a dictionary of the kmp_zstd_compress_batch_dict calls at one level class (kx_dict_level_class: the CDict's parameters and fill differ by
// it): content, CDict tables (built on the host; strategy "fast" has L alone), a formatted one's tables.  A context keeps the last
// KMP_DICT_SLOTS of them (used: the context's dict_tick when a batch last ran with it; the one unused longest makes room)
enum { KMP_DICT_SLOTS = 4 };
struct dict_part {
    dev_buf<u8> content; dev_buf<u32> L, S; dev_buf<KDictPrior> prior;
    u32 size = 0, content_size = 0; u64 hash = 0; u32 W = 0, H = 0, C = 0, M = 0; u32 rep[2] = { 0, 0 }; int level_class = 3; u64 used = 0;
    size_t bytes() const { return content.bytes + L.bytes + S.bytes + prior.bytes; }
};
// ... for the decoder: the caller's dictionary lies in device memory, its head is read back once per dictionary
struct ddict_part {
    dev_buf<KDictDPrior> prior; const void* ptr = nullptr; u32 size = 0; u64 hash = 0; u32 off = 0, id = 0, rep[3] = { 0, 0, 0 };
    size_t bytes() const { return prior.bytes; }
};
// decoder staging: sequences decoded ahead of k_zstd_decode (+ the size sort's keys, permutation and buckets), literals
struct pre_seq_part { dev_buf<u64> stage; dev_buf<KPreBlk> blk; dev_buf<u32> nblk, sort; u32 seq_cap = 0; size_t bytes() const { return stage.bytes + blk.bytes + nblk.bytes + sort.bytes; } };
struct pre_lit_part { dev_buf<u8> lits; dev_buf<KPreLit> rec; dev_buf<u32> nrec; u32 lit_cap = 0; size_t bytes() const { return lits.bytes + rec.bytes + nrec.bytes; } };
// the raw-deflate workspace, two halves of `chunk` slices each
struct dfl_lazy_part {
    dev_buf<u16> link; dev_buf<KdBest> best; dev_buf<u32> syms, wr, order;
    dev_buf<u16> rank; dev_buf<u32> state, maxlen;                 // slices above 64 KiB (deflate_lazy.h, segments): the sort's ranks, the parse's state between segments, the batch's longest slice
    hip_stream sort_st[2]; hip_event sorted[2][2], parsed[2][2];   // ... a sort stream per half; span arrays in two copies (parity of the segment): sorted / parsed events
    dev_buf<KdSliceMeta> meta; dev_buf<KdBlockInfo> blocks;
    hip_event searched[2], done[2];
    u32 chunk = 0, pos_cap = 0, blk_cap = 0;                         // slices per half, positions / blocks per slice
    size_t bytes() const { return link.bytes + best.bytes + syms.bytes + wr.bytes + order.bytes + rank.bytes + state.bytes + maxlen.bytes + meta.bytes + blocks.bytes; }
};
// levels 1 .. 3: symbols / blocks of 4 * chunk slices (one piece)
struct dfl_fast_part { dev_buf<u32> syms; dev_buf<KdSliceMeta> meta; dev_buf<KdBlockInfo> blocks; size_t bytes() const { return syms.bytes + meta.bytes + blocks.bytes; } };

// --------------------------------------------------------------------------
// batch context
// --------------------------------------------------------------------------
enum { KMP_MAX_CHUNKS = 4, KMP_MAX_PIECES = 8 };
struct kmp_span { hip_event start, end; };                 // a timed stretch of one stream (kmp_batch_set_profiling)
struct kmp_batch_ctx {
    int device = 0; u32 max_slices = 0, max_slice_bytes = 0; int G = 0; int team_fixed = 0; int table_retry = 0; u32 match_blocks = 0, match_blocks_l3 = 0, nteams = 0, l3_team_slots = 0;
    u32 seq_cap = 0, lit_cap = 0, scratch_words = 0;
    // the workspace: one arena (which holds seqs / lits / meta / scratch and the table pieces) or, without one, separate buffers;
    // the plain pointers are views into whichever holds them
    dev_buf<u8> arena;
    dev_buf<KSeq> seqs_buf; dev_buf<u8> lits_buf; dev_buf<KSliceMeta> meta_buf; dev_buf<u32> scratch_buf, tables_buf;
    KSeq* seqs = nullptr; u8* lits = nullptr; KSliceMeta* meta = nullptr; u32* scratch = nullptr; u32* tables = nullptr;
    u32* tseg[4] = { nullptr, nullptr, nullptr, nullptr }; u32 tseg_n = 0;       // the team tables in four pieces spread over the arena (or tseg_n == 1: tables alone)
    dev_buf<u32> team_epoch, counter;
    dev_buf<u32> len_ok, d_status;                // sanitised slice lengths of the running batch; status word (KMP_STATUS_*)
    // kmp_batch_set_frame_flags: what the zstd compress batches queued from now on write around their blocks (KMP_FRAME_*); frame_cks: the
    // running batch's checksums, one word per slice (the XXH64 pass of a batch with KMP_FRAME_CHECKSUM fills it)
    u32 frame_flags = 0; dev_buf<u32> frame_cks;
    u32 table_layout = 0;                         // which of the arena's layouts holds the table pieces (1 .. 8; 0: no arena)
    float place_ms = 0; u32 place_tried = 0;      // the team tables' placement: probe time of the region kept, candidates tried
    float table_reads_per_s = 0, table_pairs_per_s = 0;     // random loads / load + store pairs per second over this context's team tables (k_table_probe at creation; 0 = not measured)
    // level 3, batches of more than half the team slots: one launch of each kernel or two chunks?  Tried once each on the
    // context's first two such batches (whole-step HIP events), then the faster stays -- the parse kernel's time differs
    // by 17 % between runs of the same box, and which setting wins depends on it.
    int tune_state = 0; int tune_pending = 0; u32 tune_pick = 0; float tune_ms[2] = { 0, 0 }; kmp_span tune;
    // zstd compress pipeline: entropy coding of chunk i (second stream) runs beside the match kernel of chunk i+1
    hip_stream st2; hip_event ev_join; u32 last_chunks = 0;
    // ... or, with one launch of each kernel, entropy sweeps on the second stream beside the parse (zstd_compress_dfast; KSweepRecords).
    // sweep_rec: the count, a counter per sweep (profiling), then done[n] and coded[n] of the running batch; ev_fork: where the
    // second stream starts, behind the batch's clears; last_sweeps: sweep launches of the last batch, the final one included (0: none)
    dev_buf<u32> sweep_rec; hip_event ev_fork; int can_wait_value = 0; u32 last_sweeps = 0;
    hip_event ev_pre[KMP_MAX_CHUNKS + 1];         // decoder: [0] where the caller's stream stands, [1 + i] piece i pre-decoded
    // profiling: each group of named events with its own valid flag.  match[i].end also marks where chunk i's entropy launch may start.
    int profiling = 0;
    kmp_span match[KMP_MAX_CHUNKS], entropy[KMP_MAX_CHUNKS]; u32 timed_chunks = 0; int zstd_timed = 0;
    kmp_span decode_t; int decode_timed = 0;
    kmp_span deflate_t; int deflate_timed = 0;
    struct { hip_event chains, best, best_done, parse, encode, encode_done; } dfl_mark; int dfl_marked = 0;   // the first piece's stages (kmp_deflate_last_kernel_ms)
    // the parts added on first use (null: absent)
    std::unique_ptr<table_part> flat, t4, chain_t4;
    std::unique_ptr<lazy_part> lz;
    std::unique_ptr<lazy_big_part> lzb;
    std::unique_ptr<dict_part> dict[KMP_DICT_SLOTS]; u64 dict_tick = 0;
    std::unique_ptr<ddict_part> ddict;
    std::unique_ptr<pre_seq_part> pre_seq; std::unique_ptr<pre_lit_part> pre_lit;
    u32 pre_slices = 0, pre_blk_cap = 0; int pre_tried = 0;      // entries the staging holds (a larger batch is decoded in pieces); pre_tried: do not try again
    std::unique_ptr<dfl_lazy_part> dfl; std::unique_ptr<dfl_fast_part> dflf; int dfl_ftried = 0;
    // frames of several blocks (max_slice_bytes above 128 KiB): per-slice state carried between the block rounds
    int big = 0; int big_G = 0; dev_buf<KFrameState> fstate; dev_buf<u32> hufct, big_tables, remaining, big_counters; u32 last_rounds = 0;
    u32 cus = 0;                                  // compute units of the device
    // one batch at a time per context: a batch queued on another stream waits for the previous one's last kernel
    hip_event ev_done; int have_done = 0;
    // ... or its pieces did, each on a stream of its own (kmp_zstd_compress_batch_pieces): the next batch waits for all of them
    hip_event ev_piece[KMP_MAX_PIECES]; u32 pieces_pending = 0;
    // experiment switches, read from the environment once, when the context is created
    struct { u32 chunks, match_flags, entropy_pad, first_permille, fast_first_permille, entropy_flags, decode_flags, decode_pad, big_rounds, big_spw,
                 dfl_chunk, dfl_chain_waves, dfl_serial, dfl_flags, decode_pre, decode_sort, decode_pieces, decode_stage_slices, inflate_pre, inflate_pieces, autotune, match_v2, fuse, sweeps, sweep_min; } knob = {};
};

// The batch entry points' argument check.  fn: the name the message carries (an entry point may report for the one it serves).
// args_present: a context and whatever else must be there even for an empty batch (ok), every array of a non-empty batch;
// args_count: n against the context; batch_args: both.  The halves stand alone where an entry point has a check of its own between them.
static inline int args_present(const char* fn, bool ok, u32 n, std::initializer_list<const void*> arrays)
{
    for (const void* p : arrays) if (n && !p) ok = false;
    if (!ok) { g_last_error = std::string(fn) + ": null argument"; return KMP_ERR_ARG; }
    return KMP_OK;
}
static inline int args_count(const char* fn, const kmp_batch_ctx* c, u32 n)
{
    if (n > c->max_slices) { g_last_error = std::string(fn) + ": n exceeds the context's max_slices"; return KMP_ERR_CAPACITY; }
    return KMP_OK;
}
static inline int batch_args(const char* fn, const kmp_batch_ctx* c, u32 n, std::initializer_list<const void*> arrays, bool ok = true)
{
    KMP_TRY(args_present(fn, c && ok, n, arrays));
    return args_count(fn, c, n);
}

// a context's owner (the host engines, the streaming contexts): kmp_batch_destroy on the context's device
struct batch_deleter { void operator()(kmp_batch_ctx* c) const { kmp_batch_destroy(c); } };
using batch_ptr = std::unique_ptr<kmp_batch_ctx, batch_deleter>;

// --------------------------------------------------------------------------
// host functions shared between the translation units
// --------------------------------------------------------------------------
// A batch begins: it waits for the previous batch of this context (whatever stream that ran on), and its kernels get
// the sanitised lengths (k_len_guard).  A batch ends: oversized slices lose their frames, the event is recorded.
int batch_wait_previous(kmp_batch_ctx* c, hipStream_t st);
int batch_begin(kmp_batch_ctx* c, hipStream_t st, const u32* d_in_len, u32 n, u32 cap);
int batch_end(kmp_batch_ctx* c, hipStream_t st, const u32* d_in_len, u32 n, u32 cap, u32* d_out_len, const KSliceMeta* meta);
// a context whose arena is packed (the engines of the host-memory batch: kmp_coalesce.h)
int batch_create_packed(kmp_batch_ctx** out, int device, uint32_t max_slices, uint32_t max_slice_bytes);
// staging of the pre-decode kernels (shared by the zstd decoder and inflate), allocated on first use
u32 env_pre_min_batch();
void ensure_pre_staging(kmp_batch_ctx* c);
// lane slots of the lane-per-entry kernels in order of size: key / rank / permutation (the zstd pre-decoders' counting sort;
// len_shift = 0: keyed by the frames' sequence counts, else by entry bytes >> len_shift)
// ... with the keys (0 .. 255) and their histogram already there: bucket starts + permutation, largest keys first
int size_sort_keys(kmp_batch_ctx* c, hipStream_t st, u32 m, u32* key, u32* hist, u32* perm);
int size_sort(kmp_batch_ctx* c, hipStream_t st, const u8* src, const u64* in_off, const u32* in_len, u32 m, u32* key, u32* hist, u32* perm, u32 len_shift);
// a level-3 batch in pieces, each on a stream of its own (kmp_zstd_compress_batch_pieces = begin + every piece + end)
int pieces_begin(kmp_batch_ctx* c, u32 pieces, void* const* hip_streams);
int piece_enqueue(kmp_batch_ctx* c, u32 p, u32 pieces, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n,
                  void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, hipStream_t st);
// The end of a batch in pieces, on every way out once pieces_begin has succeeded: the pieces not queued (p >= queued) mark where
// their streams stand, and the next batch waits for every piece.  The batch's kernel timings are not the per-chunk ones.
struct pieces_end {
    kmp_batch_ctx* c; u32 pieces; void* const* streams; u32 queued;
    pieces_end(pieces_end const&) = delete;
    pieces_end& operator=(pieces_end const&) = delete;
    ~pieces_end()
    {
        for (u32 p = queued; p < pieces; p++) (void)hipEventRecord(c->ev_piece[p], (hipStream_t)streams[p]);
        c->have_done = 0; c->pieces_pending = pieces; c->last_chunks = pieces; c->zstd_timed = 0;
    }
};
// frames out of the strided device layout straight into registered host memory (device-visible address h_dst_dev)
int scatter_frames(kmp_batch_ctx* c, hipStream_t st, const u8* d_src, const u64* d_in_off, u32* d_len, u32 n, u8* h_dst_dev, const u64* d_h_off, const u32* d_h_cap, u32* d_status);
// frames of several blocks (kmp_batch.hip); stream: KFrameArgs.stream
int zstd_compress_big(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                      uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, hipStream_t st, u32 stream, u32 strategy, u32 tail_direct = 0, u32 fast_step0 = 0, bool level4 = false);
int dict_header_state(const unsigned char* dict, size_t dict_size, int for_decoder);       // 1: a well-formed dictionary in zstd's own format, 0: raw content, -1: the magic with a damaged header
int inflate_batch_impl(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n,
                       void* d_dst, const uint64_t* d_out_off, const uint32_t* d_out_cap, uint32_t* d_out_len, int32_t* d_status,
                       int format, int window_bits, void* hip_stream);
int deflate_batch_impl(kmp_batch_ctx* c, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                       uint32_t n, void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len, u32 format, void* hip_stream, int level = 6,
                       int window_bits = 15, int mem_level = 8);
