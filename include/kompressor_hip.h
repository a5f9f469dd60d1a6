/*
 * kompressor_hip.h -- C ABI of libkompressor_hip.so, the MI355X (gfx950) backend
 * that plugs in underneath Kompressor's SliceTransform / ZstdCompressor /
 * ZstdDecompressor API.
 *
 * Part 1 mirrors, one to one, what the reference's JNI layer
 * (kompressor-zstd--nativelib/src/jvmCommonMain/jni/Wrapper.cpp) calls in
 * libzstd, with the same return-code convention (size_t, errors are
 * (size_t)-code with libzstd 1.5.7's code numbering), so that Wrapper.cpp can
 * be re-pointed at this library without touching the Kotlin side
 * (INTEGRATION.md shows the binding).
 *
 * Part 2 is the batched device-pointer API (no reference equivalent: the
 * reference compresses one slice per JNI call); it is what part 1 runs with
 * n = 1 and what bench.py measures.
 *
 * Plain pointers and sizes only.  Thread rules follow the reference
 * (SURVEY.md section 8b): a context is used by one thread at a time; different
 * contexts may be used concurrently; free may come from any thread.
 */
#ifndef KOMPRESSOR_HIP_H
#define KOMPRESSOR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMP_API __attribute__((visibility("default")))

/* ------------------------------------------------------------------------ */
/* Part 1: streaming-compatible single-slice API                             */
/* ------------------------------------------------------------------------ */
typedef struct kmp_zstd_cctx kmp_zstd_cctx;
typedef struct kmp_zstd_dctx kmp_zstd_dctx;

/* end_op values == ZSTD_EndDirective (Wrapper.cpp:112 passes e_end / e_continue) */
#define KMP_ZSTD_e_continue 0
#define KMP_ZSTD_e_flush    1
#define KMP_ZSTD_e_end      2

/* parameter ids == ZSTD_cParameter (kompressor-zstd--nativelib/src/commonMain/kotlin/
 * com/ensody/kompressor/zstd/ZstdParameter.kt:3-24; only 100 is ever set,
 * ZstdCompressor.jvm.kt:21) */
#define KMP_ZSTD_c_compressionLevel 100
/* ... and the three that shape a frame's header and trailer without touching its blocks (values 0 or 1) */
#define KMP_ZSTD_c_contentSizeFlag  200   /* default 1; 0: no Frame_Content_Size, a window descriptor instead of the single-segment flag */
#define KMP_ZSTD_c_checksumFlag     201   /* default 0; 1: the low 32 bits of the content's XXH64 behind the last block */
#define KMP_ZSTD_c_dictIDFlag       202   /* default 1; 0: no Dictionary_ID field in frames parsed against a formatted dictionary */

/* replaces ZSTD_createCCtx            (Wrapper.cpp:10-17)  */
KMP_API kmp_zstd_cctx* kmp_zstd_create_cctx(void);
/* replaces ZSTD_freeCCtx              (Wrapper.cpp:19-27)  */
KMP_API size_t kmp_zstd_free_cctx(kmp_zstd_cctx* cctx);
/* replaces ZSTD_CCtx_setParameter     (Wrapper.cpp:29-39). Levels -131072 .. -1 and 1 .. 10 (0 = default = 3) run on the GPU where
 * kmp_zstd_compress_batch_level serves them (dictionaries: level 3 only; levels 5 .. 10: streams of up to 2 MiB, or one closing call of
 * at most 128 KiB -- 9 and 10 above 16 KiB --, or of up to 2 MiB when the call's output slice has room for kmp_zstd_compress_bound of it; what
 * is not served surfaces when the stream closes); levels 11 and up return (size_t)-40 "Unsupported parameter".
 * Ids 200 .. 202 (above) take 0 or 1 and return the value set, as libzstd does -- not 0; any other value returns (size_t)-42 "Parameter
 * is out of bound" (libzstd 1.5.7 itself takes every nonzero value as 1).  They hold for every frame the context writes from then on,
 * whatever path it takes, and like the level they are refused with (size_t)-60 once input has been fed.  Every other id returns
 * (size_t)-40. */
KMP_API size_t kmp_zstd_cctx_set_parameter(kmp_zstd_cctx* cctx, int param, int value);
/* replaces ZSTD_CCtx_loadDictionary   (Wrapper.cpp:41-56). Served: dictionaries of 8 .. 130 560 bytes for slices <= 128 KiB, raw content
 * or zstd's own format (magic EC30A437: what `zstd --train` / ZDICT_trainFromBuffer write -- its Huffman and FSE tables, repeat offsets
 * and ID are loaded as libzstd's ZSTD_loadCEntropy does; a damaged header surfaces at the first frame as "Dictionary is corrupted");
 * a dictionary outside that size range returns (size_t)-40. */
KMP_API size_t kmp_zstd_cctx_load_dictionary(kmp_zstd_cctx* cctx, const void* dict, size_t dict_size);
/* replaces ZSTD_compressStream2       (Wrapper.cpp:75-121, call at :112).
 * Same buffer semantics as ZSTD_inBuffer / ZSTD_outBuffer: `*_size` is the
 * end-exclusive index, `*_pos` the cursor, both into the whole array
 * (Wrapper.cpp:101-110).  Returns 0 when the frame is completely flushed,
 * >0 = bytes still to flush, or an error code.
 * The frame is the one libzstd 1.5.7 writes under the same calls, which above 128 KiB depends on them: when the call
 * that ends the input (e_end) finds libzstd's staging buffer empty and room for ZSTD_compressBound of what it brought,
 * the caller's memory is compressed in place (ZSTD_compress2's frame); otherwise -- the reference's driver, whose output
 * slices hold max(8192, n / 10) bytes -- the input is staged in chunks of 128 KiB (kmp_zstd_compress_batch_reference),
 * and data that arrived with e_continue makes it a streaming frame (no content size).  Input is collected until e_end;
 * streams up to 1 GiB at every served level (beyond a level's window -- 512 KiB at level 1 and the negative levels, 1 MiB
 * at level 2, 2 MiB at levels 3 and 4 -- the window slides as libzstd's does).
 * Levels 5 .. 10, no dictionary: data that arrived with e_continue makes a streaming frame of up to 2 MiB in all (the unknown-size
 * parameters at every length; closed with or without data); a single closing call (e_end, nothing staged) is served up to 128 KiB and,
 * in place, from 128 KiB + 1 to 2 MiB when its output slice has room for kmp_zstd_compress_bound.  Still refused with "Unsupported
 * parameter": streams beyond 2 MiB, a loaded dictionary, and the one remaining step -- the single closing call of more than 128 KiB whose
 * output slice lacks room for the bound (libzstd stages it; kmp_zstd_compress_batch_reference writes exactly those frames meanwhile). */
KMP_API size_t kmp_zstd_compress_stream(kmp_zstd_cctx* cctx,
                                        void* dst, size_t dst_size, size_t* dst_pos,
                                        const void* src, size_t src_size, size_t* src_pos,
                                        int end_op);

/* replaces ZSTD_createDCtx            (Wrapper.cpp:123-130) */
KMP_API kmp_zstd_dctx* kmp_zstd_create_dctx(void);
/* replaces ZSTD_freeDCtx              (Wrapper.cpp:132-140) */
KMP_API size_t kmp_zstd_free_dctx(kmp_zstd_dctx* dctx);
/* replaces ZSTD_DCtx_loadDictionary   (Wrapper.cpp:58-73): raw-content dictionaries and dictionaries in zstd's own format (their tables
 * stand behind a frame's first block: tree-less literals and "repeat" sequence tables refer to them; a frame that names another
 * dictionary's ID fails with "Dictionary mismatch"); a damaged header of that format returns (size_t)-64 as libzstd's DDict creation does */
KMP_API size_t kmp_zstd_dctx_load_dictionary(kmp_zstd_dctx* dctx, const void* dict, size_t dict_size);
/* replaces ZSTD_decompressStream      (Wrapper.cpp:142-187, call at :178).
 * Returns 0 when a frame is completely decoded and flushed, otherwise a
 * hint (>0) or an error code.  A frame is decoded when all of it has arrived; content up to 1 GiB. */
KMP_API size_t kmp_zstd_decompress_stream(kmp_zstd_dctx* dctx,
                                          void* dst, size_t dst_size, size_t* dst_pos,
                                          const void* src, size_t src_size, size_t* src_pos);

/* zlib twin of the above (kompressor-zlib--nativelib/src/jvmCommonMain/jni/Wrapper.cpp):
 * createCompressor :10-26 (deflateInit2), freeCompressor :28-38 (deflateEnd), compressStream :40-82
 * (deflate, call at :73).  Same cursor semantics; the return value is zlib's: Z_OK 0, Z_STREAM_END 1,
 * Z_BUF_ERROR -5 are benign for the Kotlin side (ZlibCompressor.jvm.kt:49-56).  The GPU path implements
 * levels 1 .. 9 (-1 = 6: zlib's deflate_fast for 1 .. 3, deflate_slow for 4 .. 9, each byte-identical to zlib's output),
 * windowBits as deflateInit2 takes it: -15 .. -9 (ZlibFormat.Raw), 9 .. 15 (ZlibFormat.Zlib: CMF / FLG header by window and
 * level -- 78 01 / 5E / 9C / DA with a 32 KiB window -- + Adler-32; 8 is taken as 9, as zlib does) or 25 .. 31 (ZlibFormat.Gzip:
 * 10-byte header, CRC-32 + ISIZE), memLevel 1 .. 9, strategy 0, streams up to 1 GiB (the stream is compressed when the caller
 * finishes it); other settings (level 0, windowBits 8 without the zlib wrapper -- an error in zlib too --, other strategies)
 * make create return NULL.  (A decompressor created with a smaller window than the stream's still decodes it: the window
 * declared to inflateInit2 is not enforced.) */
typedef struct kmp_zlib_cstream kmp_zlib_cstream;
typedef struct kmp_zlib_dstream kmp_zlib_dstream;
KMP_API kmp_zlib_cstream* kmp_zlib_create_compressor(int level, int window_bits, int mem_level, int strategy);
KMP_API int kmp_zlib_free_compressor(kmp_zlib_cstream* stream);
KMP_API int kmp_zlib_compress_stream(kmp_zlib_cstream* stream,
                                     void* dst, size_t dst_size, size_t* dst_pos,
                                     const void* src, size_t src_size, size_t* src_pos,
                                     int finish);
/* createDecompressor :84-98 (inflateInit2), freeDecompressor :100-110 (inflateEnd), decompressStream :112-153
 * (inflate, call at :144).  windowBits -15..-8 = raw, 8..15 = zlib wrapper (Adler-32 verified), 24..31 = gzip
 * (CRC-32 and length verified), 40..47 = zlib or gzip by the header (ZlibFormat.AutoDetectZlibGzip).  The stream is decoded when the
 * caller passes finish (the one-shot driver always does); any block types, any compression level. */
KMP_API kmp_zlib_dstream* kmp_zlib_create_decompressor(int window_bits);
KMP_API int kmp_zlib_free_decompressor(kmp_zlib_dstream* stream);
KMP_API int kmp_zlib_decompress_stream(kmp_zlib_dstream* stream,
                                       void* dst, size_t dst_size, size_t* dst_pos,
                                       const void* src, size_t src_size, size_t* src_pos,
                                       int finish);

/* replace ZSTD_isError / ZSTD_getErrorName (Wrapper.cpp:189-196) */
KMP_API unsigned kmp_zstd_is_error(size_t code);
KMP_API const char* kmp_zstd_get_error_name(size_t code);

/* ZSTD_compressBound */
KMP_API size_t kmp_zstd_compress_bound(size_t src_size);

/* ------------------------------------------------------------------------ */
/* Part 2: batched device API                                                */
/* ------------------------------------------------------------------------ */
typedef struct kmp_batch_ctx kmp_batch_ctx;

#define KMP_OK             0
#define KMP_ERR_HIP       (-1)   /* a HIP call failed: kmp_last_error() has the text */
#define KMP_ERR_ARG       (-2)
#define KMP_ERR_CAPACITY  (-3)   /* n or slice size beyond what the context was created for */
#define KMP_ERR_KERNEL    (-4)   /* a kernel guard tripped (never expected) */

/* Per-slice lengths are device data, so what the host cannot check before it launches is reported afterwards: the
 * slice gets d_out_len[i] = 0 (a frame or stream is never empty) and the context's status word collects these bits. */
#define KMP_STATUS_SLICE_TOO_LARGE 1u   /* a d_in_len[i] above the context's max_slice_bytes (DEFLATE: above 64 KiB) */
#define KMP_STATUS_KERNEL_GUARD    2u   /* a parser's loop guard tripped (never expected) */
#define KMP_STATUS_LEVEL_SIZE      4u   /* the level is not served at a slice's size (level 4: up to 16 KiB on a context for slices above 128 KiB, and 128 - 256 KiB as a staged frame; levels 9, 10: 8 bytes .. 16 KiB; levels 5 .. 10: above 2 MiB): out_len 0 */

#define KMP_MAX_SLICE_BYTES (128u * 1024u)        /* one block per frame: the batched fast path */
#define KMP_MAX_BIG_SLICE_BYTES (1u << 30)       /* frames of several blocks (context created with max_slice_bytes above
                                                  * 128 KiB); beyond the level-3 window (2 MiB) it slides as libzstd's does */

/* Workspace for up to max_slices slices of up to max_slice_bytes each on HIP
 * device `device`.  team_lanes: lanes of a wave that cooperate on one slice in
 * the match kernel (4, 8, 16, 32 or 64; 0 = default). */
KMP_API int kmp_batch_create(kmp_batch_ctx** out, int device, uint32_t max_slices,
                             uint32_t max_slice_bytes, int team_lanes);
/* ... with options.  struct_bytes = sizeof(kmp_batch_options) (versioning).  team_lanes: as above.
 * table_span_gib: the address span, in GiB, over which a context with 4 GiB or more of level-3 team tables lays out its
 * workspace arena (-1 = the environment's KMP_TABLE_SPAN_GIB, else 100; 0 = packed).  The parser's table traffic runs 11 % faster
 * over 72 GiB or more of span than inside a few dozen (DESIGN.md section 5a'); the gaps are memory the context holds and does not
 * use, so the span is bounded by half of the device's free memory at creation, and kmp_batch_memory says what was taken.
 * table_retry: 1 = when the arena measures slow whatever the layout and the device has room for a second one, try one more and
 * keep the faster (the other is freed before the call returns: the one transient allocation creation can make); 0 = never
 * (-1 = KMP_TABLE_RETRY, else 0). */
typedef struct kmp_batch_options { uint32_t struct_bytes; int team_lanes; int table_span_gib; int table_retry; } kmp_batch_options;
KMP_API int kmp_batch_create_ex(kmp_batch_ctx** out, int device, uint32_t max_slices, uint32_t max_slice_bytes,
                                const kmp_batch_options* opts);
/* Device memory the context holds right now, by part, in bytes (sets allocated on a first use count once they exist): arena =
 * the one allocation of a large context (arena_used = its parts without the span's gaps), workspace = the separate allocations of
 * a small one plus the per-team / per-slice words, other_tables = the flat tables of levels 1 / 2 / the dictionary parser, level
 * 4's sets and a dictionary's tables, block_chain = the per-slice state of contexts for slices above 128 KiB, decode_staging =
 * what the pre-decoders leave (shared by the zstd decoder and inflate), deflate_workspace = link / match / symbol arrays. */
typedef struct kmp_batch_memory_info { uint32_t struct_bytes; uint32_t reserved; size_t arena, arena_used, workspace, other_tables, block_chain, decode_staging, deflate_workspace, total; } kmp_batch_memory_info;
KMP_API int kmp_batch_memory(kmp_batch_ctx* ctx, kmp_batch_memory_info* info);
KMP_API void kmp_batch_destroy(kmp_batch_ctx* ctx);
/* Status bits (KMP_STATUS_*) raised by the batches run on this context since the last call; waits for `hip_stream`,
 * then clears them.  Returns KMP_OK, KMP_ERR_CAPACITY (a slice was too large) or KMP_ERR_KERNEL; *bits may be NULL.
 * A context runs one batch at a time: a batch queued on another stream waits for the previous one's last kernel. */
KMP_API int kmp_batch_status(kmp_batch_ctx* ctx, uint32_t* bits, void* hip_stream);
/* What the zstd compress calls write around a frame's blocks.  The flags hold for every zstd compress export run on the context
 * afterwards -- kmp_zstd_compress_batch, _level, _dict, _dict_level, _stream, _reference and _pieces --; a fresh context has flags 0
 * and writes ZSTD_compress2's default frames.  The setter does not wait: a batch takes the flags at the time it is queued.  Unknown
 * bits return KMP_ERR_ARG.  The blocks of a frame are the same bytes under every flag set, a frame with its checksum still fits
 * kmp_zstd_compress_bound(len) + 8, and the decoders verify the checksum (status 22).  A batch with KMP_FRAME_CHECKSUM runs one XXH64
 * pass over its slices in front of its other kernels (a quad of lanes per slice, so a single very long slice is hashed at one quad's
 * rate).  The seekable and BGZF containers ignore the flags: their frames stay as their formats specify them. */
#define KMP_FRAME_CHECKSUM        1u   /* ZSTD_c_checksumFlag = 1 */
#define KMP_FRAME_NO_CONTENT_SIZE 2u   /* ZSTD_c_contentSizeFlag = 0 (streaming frames never have one: nothing changes there) */
#define KMP_FRAME_NO_DICT_ID      4u   /* ZSTD_c_dictIDFlag = 0 (a raw-content dictionary, or none: nothing changes) */
KMP_API int kmp_batch_set_frame_flags(kmp_batch_ctx* ctx, uint32_t flags);
KMP_API uint32_t kmp_batch_frame_flags(kmp_batch_ctx* ctx);

/* zstd level-3 frames for n independent slices.  All pointers are device
 * pointers; slice i is d_src[d_in_off[i] .. +d_in_len[i]); its frame goes to
 * d_dst + d_out_off[i] (room for kmp_zstd_compress_bound(len) + 8 bytes) and its
 * size to d_out_len[i].  Asynchronous on `hip_stream` (a hipStream_t, may be 0).
 * The frames are the ones ZSTD_compress2 writes into a buffer of ZSTD_compressBound bytes.  Up to 128 KiB (one block)
 * that is also what the reference's ZstdCompressor(3).transform(ByteArray) returns; above, see
 * kmp_zstd_compress_batch_reference. */
KMP_API int kmp_zstd_compress_batch(kmp_batch_ctx* ctx,
                                    const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                    uint32_t n,
                                    void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len,
                                    void* hip_stream);

/* The same batch in `pieces` (1 .. 8) parts that run side by side, part p on hip_streams[p]: what a caller whose slices arrive over
 * PCIe (or from another rank) uses to overlap the copies with the kernels.  Part p covers the slices kmp_batch_piece_range(n, pieces, p)
 * names; its kernels are queued behind whatever the caller has queued on hip_streams[p] (the copy that brings those slices in) and the
 * caller queues what takes the part's frames away behind them (kmp_compact_batch on the part's range, the copy out).  The parts own
 * disjoint parts of the context's team slots and workspace, so a later part joins the earlier ones on the device instead of waiting for
 * them: the device fills up as the batch arrives.  d_in_off / d_in_len / d_out_off must be complete when the call is made (they are
 * small); frames are bit for bit kmp_zstd_compress_batch's.  Level 3, slices up to 128 KiB.  The next batch on the context, on whatever
 * stream, waits for all parts. */
KMP_API void kmp_batch_piece_range(uint32_t n, uint32_t pieces, uint32_t piece, uint32_t* first, uint32_t* count);
KMP_API int kmp_zstd_compress_batch_pieces(kmp_batch_ctx* ctx,
                                           const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                           uint32_t n,
                                           void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len,
                                           uint32_t pieces, void* const* hip_streams);

/* Streaming frames: what libzstd writes when a slice arrives through ZSTD_e_continue calls (finish = false:
 * SliceTransformRawSource.kt:32-55, BaseSliceTransformContentEncoder.kt:23-54) and is closed with ZSTD_e_end -- the size
 * is unknown when the frame starts: window 2^21, no content size in the header, the input taken in chunks of 128 KiB.
 * empty_end != 0: the closing call brought no data (then a stream that stops on a chunk boundary ends with an empty
 * block).  Any length the context holds (beyond 2 MiB + 128 KiB libzstd's staging buffer wraps: the lap before becomes
 * an older segment and the blocks are parsed by its extDict variant, restated here); the context must have been created
 * with max_slice_bytes above 128 KiB.
 * kmp_zstd_compress_stream produces these frames by itself when data arrived with KMP_ZSTD_e_continue. */
KMP_API int kmp_zstd_compress_batch_stream(kmp_batch_ctx* ctx,
                                           const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                           uint32_t n,
                                           void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len,
                                           int empty_end, void* hip_stream);
/* ... at level 3 (or 0: the call above), 4, 2, 1 or a negative level -- the reference's Ktor ZstdContentEncoder streams at
 * level 1 (kompressor-zstd-ktor ZstdContentEncoder.kt:11).  Levels 1 and below have a window of 2^19, level 2 of 2^20:
 * a longer stream is parsed as libzstd parses it once its staging buffer (window + 128 KiB) has wrapped -- blocks that
 * still reach into the lap before by its extDict variant of the "fast" parser (ZSTD_compressBlock_fast_extDict_generic),
 * restated in zstd_match_fast.h.  Any length the context holds. */
KMP_API int kmp_zstd_compress_batch_stream_level(kmp_batch_ctx* ctx,
                                                 const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                                 uint32_t n,
                                                 void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len,
                                                 int empty_end, int level, void* hip_stream);
/* The frames Kompressor's ZstdCompressor(level).transform(ByteArray) returns, for slices of any size the context holds.
 * Its driver (SliceTransform.kt:33-56) hands ZSTD_compressStream2 (Wrapper.cpp:112) output slices of max(8192, n / 10)
 * bytes: from 128 KiB + 1 on that is less than ZSTD_compressBound(n), so libzstd does not compress the array in place
 * but stages it in chunks of 128 KiB -- the block pre-splitter sees one chunk at a time, and beyond the window + 128 KiB
 * the staging buffer wraps and the window slides.  Frames differ from kmp_zstd_compress_batch's
 * wherever the pre-splitter cuts; up to 128 KiB they are the same.  Levels -131072 .. -1 and 1 .. 4 (0 = 3), any size the
 * context holds; levels 5 .. 10 up to 2 MiB (one block up to 128 KiB, staged frames above; a larger slice is refused per slice: out_len 0,
 * KMP_STATUS_LEVEL_SIZE; 9 and 10 up to 16 KiB as in kmp_zstd_compress_batch_level).  out_chunk: size of the caller's output slices if it is not the reference's (0 = max(8192, n / 10)). */
KMP_API int kmp_zstd_compress_batch_reference(kmp_batch_ctx* ctx,
                                              const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                              uint32_t n,
                                              void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len,
                                              int level, uint32_t out_chunk, void* hip_stream);
/* One-shot frames at another compression level: 1 and 2 (libzstd's one-table "fast" strategy) for slices of any size the
 * context holds (one block up to 128 KiB, frames of several blocks above; the window follows the slice size as
 * ZSTD_getCParams(level, n, 0) sets it, and a slice beyond the level's largest window is parsed with the window sliding);
 * 3 (or 0) = kmp_zstd_compress_batch.  Frames are the ones libzstd 1.5.7 writes at that level.
 * Negative levels (-131072 .. -1: libzstd's "fast" strategy on row 0 of its parameter tables, a step of 1 - level, literals
 * left uncompressed) are served like level 1.
 * Level 4 is served where libzstd runs it as "double-fast": slices above 16 KiB up to 128 KiB (window <= 17, chain 17, hash 17,
 * minimum match 4; ZSTD_getCParams(4, n, 0)), slices above 256 KiB (window <= 21, chain 18, hash 18, minimum match 5: contexts created
 * for slices above 128 KiB, per-slice tables of 2 MiB allocated by the first such batch) and streams of any size (kmp_zstd_compress_batch_stream_level).  Its tables (1 MiB per team: 64 GiB beside a 65 536-slice context, less when the device has less room; KMP_L4_TEAMS caps it) are allocated by
 * the first level-4 batch of a context.  Level 4 up to 16 KiB is strategy "greedy": those slices of a batch go through the kernels of levels
 * 5 .. 10; a slice of more than 128 KiB up to 256 KiB (greedy again, several blocks) is refused like an oversized one (out_len 0,
 * KMP_STATUS_LEVEL_SIZE).
 * Levels 5 .. 10 are libzstd's strategies "greedy" (5; 4 up to 16 KiB), "lazy" (6; 5 up to 16 KiB) and "lazy2" (7 .. 10; 6 .. 8 up to
 * 16 KiB) over its row-based match finder (windows above 2^14: the finder a library built for 128-bit vectors uses, as the reference's JNI
 * library is) or its hash chains (slices up to 16 KiB): served for slices of one block (<= 128 KiB) and, on a context created
 * for slices above 128 KiB, as frames of several blocks for slices of 128 KiB + 1 .. 2 MiB: the frames ZSTD_compress2 writes into a buffer
 * of ZSTD_compressBound bytes (row tables, repeat offsets and entropy tables carried from block to block, the strategies' pre-splitter).  On
 * such a context the slices of a batch up to 128 KiB come out as on the one-block path; a slice above 2 MiB is refused per slice (out_len 0,
 * KMP_STATUS_LEVEL_SIZE: libzstd's parameters are pinned up to there), the rest of the batch is compressed.  At
 * levels 9 and 10 a slice of 8 bytes .. 16 KiB is strategy "btlazy2": refused as above.  The first batch at these levels allocates their
 * workspace (16 bytes per position of up to 16 384 slices; on a context for larger slices also libzstd's own row tables, 5 bytes << hashLog
 * -- 2.5 MiB a slice up to 256 KiB, 20 MiB at 2 MiB -- for the slices in flight: what 8 GiB hold, 4 096 at most, KMP_LAZY_BIG_SLICES caps
 * it; a larger batch goes through in pieces).  The same kernel family writes these levels' streams (kmp_zstd_compress_batch_stream_level:
 * 0 .. 2 MiB under the unknown-size parameters, table slots of 5 bytes << the level's hashLog whatever the length -- 2.5 MiB at levels 5 and
 * 6, 20 MiB at level 10; a part made with smaller slots is made once more) and the reference driver's staged frames
 * (kmp_zstd_compress_batch_reference).  Not served at these levels: slices above 2 MiB, dictionaries. */
KMP_API int kmp_zstd_compress_batch_level(kmp_batch_ctx* ctx,
                                          const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                          uint32_t n,
                                          void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len,
                                          int level, void* hip_stream);
/* same with a dictionary shared by all n slices (what ZstdCompressor(level, dictionary) does per slice:
 * ZSTD_CCtx_loadDictionary, Wrapper.cpp:41-56, then the one-shot compress): frames are the ones libzstd 1.5.7 writes --
 * its CDict is built here on the host once per dictionary; slices up to 16 KiB are parsed against the attached CDict,
 * larger ones against its copied tables.  h_dict is HOST memory, 8 .. 130 560 bytes; slices <= 128 KiB.
 * The dictionary is raw content, or -- when it starts with the magic EC30A437 -- in zstd's own format (ZDICT / `zstd --train`): then
 * matches are searched in its content part, the block is coded against its entropy tables (literals with its Huffman table when that
 * is cheaper or the input is small, sequence tables it marks complete reused below 1 000 sequences), a frame starts with its repeat
 * offsets and names its ID.  KMP_ERR_ARG when the magic is there and the header behind it is damaged. */
KMP_API int kmp_zstd_compress_batch_dict(kmp_batch_ctx* ctx,
                                         const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                         uint32_t n,
                                         void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len,
                                         const void* h_dict, uint32_t dict_size,
                                         void* hip_stream);
/* same at a level (what ZstdCompressor(level, dictionary) does: ZSTD_CCtx_setParameter, Wrapper.cpp:29-39, then the above).  Level 0 or 3:
 * kmp_zstd_compress_batch_dict, bit for bit.  Levels 1, 2 and -131072 .. -1 (strategy "fast"): libzstd 1.5.7's frames again -- its CDict at
 * these levels is one table, sized by the level's row for the dictionary alone (negative levels: row 0); slices up to 8 KiB are parsed
 * against the attached CDict (ZSTD_compressBlock_fast_dictMatchState_generic), larger ones against its copied table
 * (ZSTD_compressBlock_fast_extDict_generic); a negative level searches every -level-th position and leaves literals uncompressed.  The
 * same envelope: h_dict is HOST memory, 8 .. 130 560 bytes, raw content or zstd's own format (as above, KMP_ERR_ARG for a damaged header);
 * slices <= 128 KiB.  A context keeps the CDicts of the last four (dictionary, level class) pairs it was called with -- the classes: 3,
 * 1, 2, negative --, so batches that alternate between them build nothing anew.  Levels 4 and up with a dictionary: KMP_ERR_ARG. */
KMP_API int kmp_zstd_compress_batch_dict_level(kmp_batch_ctx* ctx,
                                               const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                               uint32_t n,
                                               void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len,
                                               const void* h_dict, uint32_t dict_size,
                                               int level, void* hip_stream);

/* Inverse: n zstd frames -> n slices.  Frame i is d_src[d_in_off[i] .. +d_in_len[i]);
 * its content goes to d_dst + d_out_off[i] (capacity d_out_cap[i]); d_out_len[i]
 * receives the decoded size and d_status[i] 0 or a libzstd error code (20 =
 * corruption, 70 = destination too small, 72 = source size wrong / truncated / a compressed block above min(window, 128 KiB),
 * 10 = no zstd magic, 14 = unsupported frame parameter, 22 = checksum wrong or cut short, 24 = four literal streams for fewer than
 * 6 literals ...).  An entry may hold several frames back to back, with skippable frames
 * between them: their contents are concatenated, as ZSTD_decompress does; an empty entry decodes to nothing.
 * Nothing outside [d_in_off[i], +d_in_len[i]) is read and nothing outside [d_out_off[i], +d_out_cap[i]) is
 * written, whatever the bytes of the entry are (tests/fuzz_decoders.py).  A caller that does not know the sizes gets d_out_cap and
 * d_out_off from kmp_zstd_frame_info_batch + kmp_batch_layout below. */
KMP_API int kmp_zstd_decompress_batch(kmp_batch_ctx* ctx,
                                      const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                      uint32_t n,
                                      void* d_dst, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                                      uint32_t* d_out_len, uint32_t* d_status,
                                      void* hip_stream);
/* same with a dictionary shared by all n frames (reference: ZstdDecompressor(dictionary), Wrapper.cpp:58-73, test ZstdTest.kt:49-65).
 * Raw content: d_dict[0 .. dict_size) is the history before the first byte of every frame.  zstd's own format (magic EC30A437): the
 * content part is that history, and the tables, repeat offsets and ID in front of it are what ZSTD_loadDEntropy makes of them (the
 * dictionary's first 2 KiB are read back to the host once per dictionary).  status 32 ("Dictionary mismatch") for a frame whose header
 * names another ID -- with a raw-content dictionary or none: any ID. */
KMP_API int kmp_zstd_decompress_batch_dict(kmp_batch_ctx* ctx,
                                           const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                           uint32_t n,
                                           void* d_dst, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                                           uint32_t* d_out_len, uint32_t* d_status,
                                           const void* d_dict, uint32_t dict_size,
                                           void* hip_stream);

/* What the entries of a batch declare about themselves, without decoding them: the batched form of libzstd's ZSTD_findDecompressedSize,
 * ZSTD_decompressBound and ZSTD_findFrameCompressedSize, for callers whose frames lie in device memory and whose sizes did not travel
 * with them.  Entry i is d_src[d_in_off[i] .. +d_in_len[i]), walked frame by frame as ZSTD_decompressBound walks it: skippable frames
 * (magic 0x184D2A5?), zstd frames header by header and block header by block header; nothing is decoded and no byte outside the entry
 * is read, whatever its bytes and wherever it lies.  The answers are libzstd 1.5.7's, damaged and short entries included
 * (tests/golden/zstd_frame_info_golden.json).  An empty entry is content 0, bound 0, status 0, frames 0. */
#define KMP_CONTENT_UNKNOWN (~0ull)
typedef struct {
    uint64_t content;   /* ZSTD_findDecompressedSize of the entry: the exact total, or KMP_CONTENT_UNKNOWN when a frame declares none
                         * (~0ull - 1, the library's ZSTD_CONTENTSIZE_ERROR, when the total of the declared sizes wraps 64 bits) */
    uint64_t bound;     /* ZSTD_decompressBound of the entry: declared size where there is one, else blocks x min(window, 128 KiB), summed */
    uint32_t status;    /* 0, or libzstd's error code for the first frame that ZSTD_findFrameCompressedSize rejects: 10 no known magic,
                         * 14 reserved bit / skippable size that wraps, 16 window above 2^31, 20 reserved block type, 72 the entry ends
                         * inside a header, a block or a checksum.  Then content and bound are 0. */
    uint32_t frames;    /* zstd frames in the entry (skippable ones not counted; with a status: those in front of the rejected one) */
    uint32_t dict_id;   /* the first zstd frame's dictionary ID, 0 = none */
    uint32_t flags;     /* bit 0: some frame carries a checksum; bit 1: the entry holds a skippable frame; bit 2: it holds a frame in the
                         * format of zstd 0.5, 0.6 or 0.7 (magic 0xFD2FB525 .. 27), which a libzstd built with legacy support -- the
                         * binary 1.5.7 is -- sizes like any other and which is counted in `frames`; the decoders here answer 10 for it */
} kmp_zstd_frame_info;  /* 32 bytes */
/* d_info[i] (device memory of the caller's, n entries, 8-byte aligned) receives entry i's answers: one kernel, a lane per entry,
 * asynchronous on hip_stream -- no allocation, no host wait, nothing of the context's decode staging is touched (a context that has
 * never decoded stays as small as it was).  n up to the context's max_slices; n == 0 is KMP_OK. */
KMP_API int kmp_zstd_frame_info_batch(kmp_batch_ctx* ctx, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n,
                                      kmp_zstd_frame_info* d_info, void* hip_stream);
/* The layout of a decode made of those answers, on the device: d_out_cap[i] = bound[i] -- or 0 where status[i] != 0 or the bound does
 * not fit the ABI's 32-bit capacities (the decoder then reports the entry itself: its own error for a damaged one, 70 for one too
 * large) --, d_out_off[i] = the sum of the capacities in front of it, each rounded up to `align` (a power of two from 1 to 4096, else
 * KMP_ERR_ARG), d_total[0] = the sum over all n: what the destination must hold, d_total[1] = the entries given capacity 0 for one of
 * the two reasons.  One kernel, asynchronous, deterministic; the arrays are what kmp_zstd_decompress_batch takes.  A caller reads
 * d_total[0] back once (the one host wait, forced by the allocation), or decodes into a destination it knows to be large enough
 * without any.  The kernel reads `bound` (offset 8) and `status` (offset 16, tested against 0) only: it takes a kmp_inflate_info
 * array (below) by a pointer cast, for the layout of kmp_inflate_batch. */
KMP_API int kmp_batch_layout(kmp_batch_ctx* ctx, const kmp_zstd_frame_info* d_info, uint32_t n, uint32_t align,
                             uint64_t* d_out_off, uint32_t* d_out_cap, uint64_t* d_total /* [2] */, void* hip_stream);
/* The same inspection of entries in HOST memory: the same code compiled for the host, no GPU touched, no context needed (a batch of
 * 8 192 entries or more is spread over up to 16 threads). */
KMP_API int kmp_zstd_frame_info_host(const void* h_src, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                     kmp_zstd_frame_info* info);

/* Raw DEFLATE (RFC 1951) streams as zlib level 6 / windowBits 15 / memLevel 8 / strategy 0 writes
 * them: the batched form of deflateInit2(6, Z_DEFLATED, -15, 8, 0) + deflate(Z_FINISH)
 * (reference: kompressor-zlib--nativelib/src/jvmCommonMain/jni/Wrapper.cpp:20,73; Kotlin
 * ZlibCompressor(ZlibFormat.Raw, 6)).  Slices up to the context's max_slice_bytes (64 KiB at least; above 64 KiB zlib's
 * 32 KiB window slides, and a context made for such slices takes them through its kernels in 64 KiB spans: the call then waits
 * once on hip_stream, to read the batch's longest slice back, before it enqueues the rest); stream i goes to
 * d_dst + d_out_off[i] (room for kmp_deflate_bound(len), which covers all three formats: stored blocks of 5 + n
 * bytes per 65 535, the 18 bytes of a gzip header and trailer), its size to d_out_len[i]. */
KMP_API size_t kmp_deflate_bound(size_t src_size);
KMP_API int kmp_deflate_compress_batch(kmp_batch_ctx* ctx,
                                       const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                       uint32_t n,
                                       void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len,
                                       void* hip_stream);
/* same, with the RFC 1950 zlib wrapper (what ZlibFormat.Zlib at the default level produces) */
KMP_API int kmp_zlib_compress_batch(kmp_batch_ctx* ctx,
                                    const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                    uint32_t n,
                                    void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len,
                                    void* hip_stream);
/* same, with the RFC 1952 gzip wrapper (ZlibFormat.Gzip -> windowBits + 16, ZlibFormat.kt:41-44): the 10-byte header
 * zlib writes on Linux (no name, MTIME 0, XFL 0, OS 3), CRC-32 and ISIZE trailer */
KMP_API int kmp_gzip_compress_batch(kmp_batch_ctx* ctx,
                                    const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                    uint32_t n,
                                    void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len,
                                    void* hip_stream);
/* The three above at another of zlib's levels (1 .. 9, -1 = 6; ZlibCompressor(level = ...),
 * ZlibCompressor.jvm.kt:19-30 -> deflateInit2, Wrapper.cpp:20).  4 .. 9 (deflate_slow): the level's good_length / max_lazy /
 * nice_length / max_chain (4: 4 4 16 16, 5: 8 16 32 32, 6: 8 16 128 128, 7: 8 32 128 256, 8: 32 128 258 1024,
 * 9: 32 258 258 4096) drive the same kernels.  1 .. 3 (deflate_fast; 1: 4 4 8 4, 2: 4 5 16 8, 3: 4 6 32 32): one kernel that
 * parses and keeps its hash chains a lane per slice.  The zlib header's level flags (78 01 / 78 5E / 78 9C / 78 DA) and gzip's
 * XFL (4 at level 1, 2 at level 9) follow.  format: 0 raw, 1 zlib, 2 gzip.  Level 0 (stored) is not served: KMP_ERR_ARG. */
KMP_API int kmp_deflate_compress_batch_level(kmp_batch_ctx* ctx,
                                             const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                             uint32_t n,
                                             void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len,
                                             int format, int level, void* hip_stream);
/* ... and with the other two settings the Kotlin constructor passes to deflateInit2 (ZlibCompressor(format, compressionLevel,
 * windowBits, memLevel): ZlibCompressor.jvm.kt:7-17, ZlibFormat.kt:32-57; Wrapper.cpp:20): window_bits 9 .. 15 -- the window is
 * 1 << window_bits bytes, matches reach back (1 << window_bits) - 262, the zlib header's CMF byte says so; 8 is taken as 9 with
 * the zlib wrapper and refused without it, as zlib does -- and mem_level 1 .. 9: the hash has mem_level + 7 bits and a block is
 * closed after (1 << (mem_level + 6)) - 1 symbols.  Here window_bits is the plain number and `format` names the wrapper (the
 * sign / + 16 encoding of deflateInit2 is the streaming entry point's, kmp_zlib_create_compressor).  Stream i needs room for
 * kmp_deflate_bound_params(len, window_bits, mem_level): zlib's deflateBound for settings other than the default ones (an eighth
 * more than the data).  KMP_ERR_ARG for anything else. */
KMP_API size_t kmp_deflate_bound_params(size_t src_size, int window_bits, int mem_level);
KMP_API int kmp_deflate_compress_batch_params(kmp_batch_ctx* ctx,
                                              const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len,
                                              uint32_t n,
                                              void* d_dst, const uint64_t* d_out_off, uint32_t* d_out_len,
                                              int format, int level, int window_bits, int mem_level, void* hip_stream);
/* inflate: n streams -> d_dst + d_out_off[i] (capacity d_out_cap[i]); format 0 = raw deflate, 1 = zlib,
 * 2 = gzip, 3 = zlib or gzip decided per stream by its first bytes (ZlibFormat.AutoDetectZlibGzip,
 * ZlibFormat.kt:52-55); checksums are verified;
 * d_status[i] = 0, -3 (Z_DATA_ERROR) or -5 (Z_BUF_ERROR: capacity too small or input truncated).
 * Runs as two kernels when the context's staging is there (allocated on the first call, shared with the zstd decoder:
 * streams whose output fits the context's max_slice_bytes are decoded a lane per stream and executed a wave per stream;
 * the others -- and every stream with stored blocks or an error -- by one wave per stream); any n. */
KMP_API int kmp_inflate_batch(kmp_batch_ctx* ctx,
                              const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n,
                              void* d_dst, const uint64_t* d_out_off, const uint32_t* d_out_cap,
                              uint32_t* d_out_len, int32_t* d_status, int format, void* hip_stream);
/* How large the entries of a batch of DEFLATE streams decode to, for callers who do not know (a DEFLATE stream declares no size: raw
 * and zlib streams carry none, gzip's ISIZE stands at the end and is mod 2^32).  Entry i is walked block by block and Huffman code by
 * Huffman code, a lane per stream -- stored, fixed and dynamic blocks, the zlib header, the gzip header with FEXTRA / FNAME / FCOMMENT /
 * FHCRC --, nothing is written but d_info[i], and no byte outside the entry is read, whatever its bytes and wherever it lies.  Accepted
 * is what zlib's inflate accepts as one complete stream that fills the entry (tests/golden/inflate_info_golden.json) -- except that
 * the Adler-32 / CRC-32 VALUES of the trailers are NOT verified (there is no output to sum): kmp_inflate_batch, run afterwards,
 * reports them.  gzip's ISIZE is checked against the size mod 2^32, and a header CRC (FHCRC) against the header. */
typedef struct {
    uint64_t content;   /* bytes the entry decodes to (may exceed 32 bits: 1 032 x the entry at most) */
    uint64_t bound;     /* = content: what kmp_batch_layout reads */
    int32_t  status;    /* 0, -3 (Z_DATA_ERROR) or -5 (Z_BUF_ERROR: the entry ends before its last block does, or is too short to hold
                         * its wrapper: 6 bytes zlib, 18 gzip); then content = bound = 0, and so is every field below */
    uint32_t blocks;    /* DEFLATE blocks walked */
    uint32_t flags;     /* bit 0 a stored block, bit 1 a fixed-Huffman block, bit 2 a dynamic block, bit 3 the entry is gzip
                         * (format 2, or 3 detected), bit 4 its gzip header has optional fields (FEXTRA / FNAME / FCOMMENT / FHCRC) */
    uint32_t window_bits; /* zlib wrapper: CINFO + 8; otherwise 0 */
} kmp_inflate_info;     /* 32 bytes; laid out so that kmp_batch_layout takes the array unchanged */
/* format 0 .. 3 as in kmp_inflate_batch (else KMP_ERR_ARG).  d_info: device memory of the caller's, n entries, 8-byte aligned.  One
 * kernel, asynchronous on hip_stream: no allocation, no host wait, nothing of the context's decode staging is touched (kmp_batch_memory
 * answers the same before and after, on a context that has never decoded).  n up to the context's max_slices; n == 0 is KMP_OK.
 * Then: kmp_batch_layout((const kmp_zstd_frame_info*)d_info, ...) -> d_out_off / d_out_cap -> kmp_inflate_batch. */
KMP_API int kmp_inflate_info_batch(kmp_batch_ctx* ctx, const void* d_src, const uint64_t* d_in_off, const uint32_t* d_in_len, uint32_t n,
                                   kmp_inflate_info* d_info, int format, void* hip_stream);
/* ms4[0..3] = k_deflate_chains, k_deflate_best, k_deflate_parse, k_deflate_encode of the last batch */
KMP_API int kmp_deflate_last_kernel_ms(kmp_batch_ctx* ctx, float* ms4);

/* Dense packing helper: copies frame i from d_src + d_in_off[i] (d_len[i] bytes) to
 * d_dst + d_out_off[i], where d_out_off is the exclusive prefix sum of d_len that
 * this call also computes (d_out_off has n+1 entries; the last is the total). */
KMP_API int kmp_compact_batch(kmp_batch_ctx* ctx, const void* d_src, const uint64_t* d_in_off,
                              const uint32_t* d_len, uint32_t n, void* d_dst, uint64_t* d_out_off,
                              void* hip_stream);

/* zstd's seekable container (contrib/seekable_format upstream; no reference counterpart: the reference compresses one slice per call):
 * ONE large buffer cut into independent frames of frame_bytes each, compressed as a batch -- the fast path -- and followed by a seek
 * table, one skippable frame that lists every frame's compressed size, decompressed size and, with KMP_SEEKABLE_CHECKSUMS, the low 32
 * bits of XXH64 (seed 0) of its content.  Any zstd decoder decodes the container as an ordinary .zst (it skips the table); a seekable
 * reader fetches a byte range by decoding only the frames that cover it.  All fields little-endian:
 *   seek table = 5E 2A 4D 18 | Frame_Size u32 = n * entry_bytes + 9 | entries | Number_Of_Frames u32 | Descriptor u8 | B1 EA 92 8F
 *   entry      = Compressed_Size u32 | Decompressed_Size u32 | [Checksum u32]      Descriptor: bit 7 checksums, bits 6..2 must be 0
 * The frames are bit for bit those kmp_zstd_compress_batch_level writes for the chunks (libzstd 1.5.7's), so the whole container is
 * determined byte for byte by (input, frame_bytes, level, flags). */
#define KMP_SEEKABLE_CHECKSUMS 1u
/* room a container of src_size bytes needs: kmp_zstd_compress_bound of every chunk, plus the table (0: frame_bytes outside 1 .. 131 072) */
KMP_API size_t kmp_zstd_seekable_bound(size_t src_size, uint32_t frame_bytes, uint32_t flags);
/* device scratch (8-byte aligned) the compress call wants from its caller: the frames at bound-sized strides before they are packed,
 * and the chunks' offset, length and checksum arrays.  The context allocates nothing for this feature: kmp_batch_memory answers the
 * same before and after (a level's own first-use workspace, as kmp_zstd_compress_batch_level documents it for levels 4 .. 8, is that call's). */
KMP_API size_t kmp_zstd_seekable_scratch(size_t src_size, uint32_t frame_bytes);
/* d_src[0 .. src_size) -> the container at d_dst (dst_cap >= kmp_zstd_seekable_bound, else KMP_ERR_CAPACITY).  Asynchronous on
 * hip_stream, no host wait: plan, the batch at `level`, XXH64 of every chunk (with checksums), kmp_compact_batch's packing, the table.
 * frame_bytes: 1 .. 131 072 (else KMP_ERR_ARG) and at most the context's max_slice_bytes; the chunks, ceil(src_size / frame_bytes), at
 * most its max_slices (else KMP_ERR_CAPACITY: rounds over a larger buffer are not served).  level: -131072 .. 8 (0 = 3), the levels
 * kmp_zstd_compress_batch_level serves at every size up to 128 KiB; 9 and 10 are KMP_ERR_ARG (a short last chunk would be refused).
 * d_result (device, 8-byte aligned): [0] = the container's size, or 0 when a chunk got no frame; [1] = the context's KMP_STATUS_* bits as
 * they stand.  An empty input gives the 17 bytes of a table without entries. */
KMP_API int kmp_zstd_seekable_compress(kmp_batch_ctx* ctx, const void* d_src, size_t src_size, uint32_t frame_bytes, int level, uint32_t flags,
                                       void* d_dst, size_t dst_cap, void* d_scratch, size_t scratch_bytes, uint64_t* d_result /* [2] */,
                                       void* hip_stream);
/* What a container's table says.  status is libzstd's number: 0 good; 10 ("Unknown frame descriptor") a magic is missing or the blob
 * is shorter than 17 bytes; 20 ("Data corruption detected") a reserved descriptor bit, a table larger than the blob or with more than
 * 2^27 entries, a Frame_Size that disagrees, an entry above 1 GiB of content, or compressed sizes that do not sum to the table's
 * offset.  With a status every other field is 0. */
typedef struct {
    uint64_t content;         /* decompressed bytes of the whole container */
    uint64_t table_off;       /* where the frames end and the table begins */
    uint32_t frames;          /* entries (an entry of decompressed size 0 may stand for a skippable frame inside the file) */
    uint32_t max_frame;       /* the largest decompressed size of an entry: what a context must hold to read it */
    uint32_t max_compressed;  /* the largest compressed size */
    uint32_t flags;           /* KMP_SEEKABLE_CHECKSUMS */
    uint32_t status;
    uint32_t reserved;
} kmp_seekable_stat;          /* 40 bytes */
typedef struct kmp_seekable kmp_seekable;
/* Validates the table of d_blob[0 .. blob_size) (device memory) on the device, then makes the ONE host wait of this feature: it reads
 * the answer and the table back (12 bytes per frame with checksums, 8 without; a table beyond 256 KiB takes a second copy) and keeps the
 * prefix sums of both sizes in the handle, on the host and -- as the arrays kmp_zstd_decompress_batch takes -- on the device (28 bytes per
 * frame, owned by the handle).  A damaged table still gives a handle (KMP_OK): stat tells, and reads are refused.  A handle serves one
 * stream at a time and must be closed before its context is destroyed. */
KMP_API int kmp_zstd_seekable_open(kmp_batch_ctx* ctx, const void* d_blob, size_t blob_size, kmp_seekable** out, void* hip_stream);
KMP_API void kmp_zstd_seekable_close(kmp_seekable* h);
KMP_API int kmp_zstd_seekable_stat(const kmp_seekable* h, kmp_seekable_stat* stat);
/* The same validation of a blob in HOST memory: the same code compiled for the host, no GPU touched, no context needed.  frame_off /
 * content_off (each may be NULL): the prefix sums of the compressed / decompressed sizes, frames + 1 entries each, written when the
 * status is 0 and prefix_cap >= frames + 1. */
KMP_API int kmp_zstd_seekable_index_host(const void* h_blob, size_t blob_size, kmp_seekable_stat* stat,
                                         uint64_t* frame_off, uint64_t* content_off, size_t prefix_cap);
/* bytes a read of [lo, hi) writes: the covering frames whole (hi is cut at the content's end; 0 for an empty range or one past the end) */
KMP_API size_t kmp_zstd_seekable_read_bound(const kmp_seekable* h, uint64_t lo, uint64_t hi);
/* ... and how many frames cover it (0 for such a range): the statuses a read writes; *first (may be NULL) = the first one's index */
KMP_API uint32_t kmp_zstd_seekable_read_frames(const kmp_seekable* h, uint64_t lo, uint64_t hi, uint32_t* first);
/* Decodes the frames that cover [lo, hi), whole and back to back, into d_dst (dst_cap >= kmp_zstd_seekable_read_bound, else
 * KMP_ERR_CAPACITY) with kmp_zstd_decompress_batch on the handle's context; *skip = lo minus the first covering frame's start, so the
 * bytes asked for are d_dst[*skip .. *skip + hi - lo).  The covering frames come from the handle's host index: nothing is read back and
 * the call is asynchronous.  More covering frames than the context's max_slices go through in rounds.  d_status (device, one uint32 per
 * covering frame: kmp_zstd_seekable_read_frames says how many) receives 0 or libzstd's error code.  verify != 0 on a
 * container with checksums: every decoded frame's XXH64 is compared with its entry on the device; a mismatch makes that frame's status
 * 22 ("Restored data doesn't match checksum"), a decoded size other than the entry's 20.  d_blob: the container the handle was opened
 * over.  An empty range or one past the end is KMP_OK with nothing written; a handle whose status is not 0 is KMP_ERR_ARG.  Frames
 * larger than the context's max_slice_bytes (foreign containers) are decoded as far as kmp_zstd_decompress_batch decodes them. */
KMP_API int kmp_zstd_seekable_read(kmp_seekable* h, const void* d_blob, uint64_t lo, uint64_t hi, int verify, void* d_dst, size_t dst_cap,
                                   uint64_t* skip, uint32_t* d_status, void* hip_stream);

/* BGZF containers (SAM specification 4.1; bgzip, htslib, Bio.bgzf; no reference counterpart: the reference compresses one slice per
 * call): the zlib twin of the seekable container.  ONE large buffer cut into blocks of block_bytes each, every block a gzip member of its
 * own whose extra field carries the member's size, then an empty member as the end-of-file marker.  Any gzip reader (gunzip, Python's gzip)
 * reads the container as ordinary multi-member gzip; a BGZF reader fetches a byte range by decoding only the members that cover it.  All
 * fields little-endian:
 *   member = 1f 8b 08 04 | MTIME 00000000 | XFL 00 | OS ff | XLEN 0006 | 'B' 'C' 02 00 | BSIZE u16 = member bytes - 1
 *            | raw DEFLATE payload | CRC32 u32 | ISIZE u32
 *   marker = 1f8b08040000000000ff0600424302001b0003000000000000000000          (28 bytes)
 * The payloads are bit for bit those kmp_deflate_compress_batch_level(format 0, level) writes for the blocks (zlib 1.2.11's
 * deflateInit2(level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY)), so the whole container is determined byte for byte by (input, block_bytes,
 * level). */
#define KMP_BGZF_NO_EOF 1u     /* leave the marker out: rounds over a larger buffer are concatenated by the caller (BGZF files concatenate) */
/* room a container of src_size bytes needs: kmp_deflate_bound + 8 of every block, plus the marker (0: block_bytes outside 1 .. 65 280) */
KMP_API size_t kmp_bgzf_bound(size_t src_size, uint32_t block_bytes, uint32_t flags);
/* device scratch (8-byte aligned) the compress call wants from its caller: the members at bound-sized strides before they are packed and
 * the blocks' offset and length arrays.  The context allocates nothing for this feature beyond the DEFLATE workspace the batch call
 * itself takes on its first use. */
KMP_API size_t kmp_bgzf_scratch(size_t src_size, uint32_t block_bytes);
/* d_src[0 .. src_size) -> the container at d_dst (dst_cap >= kmp_bgzf_bound, else KMP_ERR_CAPACITY).  Asynchronous on hip_stream, no host
 * wait: plan, the raw DEFLATE batch at `level` (1 .. 9, -1 = 6; else KMP_ERR_ARG), header, CRC-32 and ISIZE around every payload,
 * kmp_compact_batch's packing, the marker.  block_bytes: 1 .. 65 280 (else KMP_ERR_ARG; 65 280 is htslib's) and at most the context's
 * max_slice_bytes; the blocks, ceil(src_size / block_bytes), at most its max_slices (else KMP_ERR_CAPACITY: cut a larger buffer into
 * rounds with KMP_BGZF_NO_EOF on all but the last and concatenate).  d_result (device, 8-byte aligned): [0] = the container's size, or 0
 * when a block got no member; [1] = the context's KMP_STATUS_* bits as they stand.  An empty input gives the marker alone, or nothing
 * with KMP_BGZF_NO_EOF. */
KMP_API int kmp_bgzf_compress(kmp_batch_ctx* ctx, const void* d_src, size_t src_size, uint32_t block_bytes, int level, uint32_t flags,
                              void* d_dst, size_t dst_cap, void* d_scratch, size_t scratch_bytes, uint64_t* d_result /* [2] */, void* hip_stream);
/* What following the members from offset 0 finds.  status is zlib's number: 0 good; -3 (Z_DATA_ERROR) a head that is no BGZF member's
 * (magic, XLEN below 6, a subfield past XLEN, BC missing, doubled or of another length than 2, a BSIZE too small for its own header, an
 * ISIZE above 65 536); -5 (Z_BUF_ERROR) the blob ends inside a member, or is empty.  With a status every other field is 0. */
typedef struct {
    uint64_t content;         /* decompressed bytes of the whole container */
    uint32_t blocks;          /* members, empty ones and the marker included */
    uint32_t max_block;       /* the largest ISIZE */
    uint32_t max_compressed;  /* the largest member */
    uint32_t flags;           /* bit 0: the last member is the end-of-file marker; bit 1: some member has extra subfields besides BC */
    int32_t  status;
    uint32_t reserved;
} kmp_bgzf_stat;              /* 32 bytes */
typedef struct kmp_bgzf kmp_bgzf;
/* Finds the members of d_blob[0 .. blob_size) (device memory) on the device.  BGZF has no table: a serial reader follows the size fields
 * from offset 0, one dependent memory read per member.  This call reads the blob once in parallel, tests a member's head wherever the
 * magic stands (candidates, false ones inside compressed data included), links every candidate to the one its size points at, and marks
 * the chain from offset 0 by pointer doubling.  Two host waits: the candidates' count (the tables are allocated to it), then the stat and
 * the prefix sums of both sizes, kept in the handle on the host and, as the arrays kmp_inflate_batch takes, on the device (36 bytes per
 * member).  Above 2^20 candidates (or a blob of 64 GiB) the members are followed by one lane instead.  Either way the answer is the
 * serial walk's, byte for byte.  A damaged blob still gives a handle (KMP_OK): stat tells, and reads are refused.  A handle serves one
 * stream at a time and must be closed before its context is destroyed. */
KMP_API int kmp_bgzf_open(kmp_batch_ctx* ctx, const void* d_blob, size_t blob_size, kmp_bgzf** out, void* hip_stream);
KMP_API void kmp_bgzf_close(kmp_bgzf* h);
KMP_API int kmp_bgzf_stat_of(const kmp_bgzf* h, kmp_bgzf_stat* stat);
/* The serial walk over a blob in HOST memory: the same code compiled for the host, no GPU touched, no context needed.  member_off /
 * content_off (each may be NULL): where every member starts in the blob / in the content, blocks + 1 entries each (the last: the blob's
 * size, the content's), written when the status is 0 and prefix_cap >= blocks + 1. */
KMP_API int kmp_bgzf_index_host(const void* h_blob, size_t blob_size, kmp_bgzf_stat* stat, uint64_t* member_off, uint64_t* content_off, size_t prefix_cap);
/* bytes a read of [lo, hi) writes: the covering members whole (hi is cut at the content's end; 0 for an empty range or one past the end) */
KMP_API size_t kmp_bgzf_read_bound(const kmp_bgzf* h, uint64_t lo, uint64_t hi);
/* ... and how many members cover it (0 for such a range): the statuses a read writes; *first (may be NULL) = the first one's index */
KMP_API uint32_t kmp_bgzf_read_blocks(const kmp_bgzf* h, uint64_t lo, uint64_t hi, uint32_t* first);
/* Decodes the members that cover [lo, hi), whole and back to back, into d_dst (dst_cap >= kmp_bgzf_read_bound, else KMP_ERR_CAPACITY):
 * their raw payloads go through kmp_inflate_batch (format 0) on the handle's context with the ISIZEs as capacities -- a gzip member with
 * an extra field would miss that call's two-kernel path --, then every trailer is checked on the device.  *skip = lo minus the first
 * covering member's start: the bytes asked for are d_dst[*skip .. *skip + hi - lo).  Nothing is read back, the call is asynchronous;
 * more covering members than the context's max_slices go through in rounds.  d_status (device, one int32 per covering member:
 * kmp_bgzf_read_blocks says how many): 0, or zlib's number as kmp_inflate_batch gives it; a member that decoded cleanly to another size
 * than its ISIZE gets -3, and with verify != 0 one whose CRC-32 differs from its trailer -3 as well.  d_blob: the container the handle was
 * opened over.  An empty range or one past the end is KMP_OK with nothing written; a handle whose status is not 0 is KMP_ERR_ARG. */
KMP_API int kmp_bgzf_read(kmp_bgzf* h, const void* d_blob, uint64_t lo, uint64_t hi, int verify, void* d_dst, size_t dst_cap,
                          uint64_t* skip, int32_t* d_status, void* hip_stream);
/* BGZF's virtual offset of content position content_pos: the start of the member that holds it << 16 | its offset inside the member's
 * content.  content_pos == the content's size gives the blob's size << 16; beyond it, or a handle with a status, ~0. */
KMP_API uint64_t kmp_bgzf_tell(const kmp_bgzf* h, uint64_t content_pos);

/* Per-kernel device time of the last batch call, measured with HIP events on the
 * launch stream (0 = off, 1 = on).  kmp_batch_last_kernel_ms synchronises. */
KMP_API int kmp_batch_set_profiling(kmp_batch_ctx* ctx, int on);
/* which: 0 = zstd_match, 1 = zstd_entropy (mean over the launches of the last compress batch), 2 = zstd_decode.
 * A large level-3 batch is entropy-coded by sweeps that run beside the parse and a final one behind it (kmp_batch_last_sweeps):
 * for such a batch 1 is the final sweep alone -- the entropy time that is still exposed, not the coding time of the whole batch. */
KMP_API int kmp_batch_last_kernel_ms(kmp_batch_ctx* ctx, int which, float* ms);
/* kmp_zstd_compress_batch cuts a large batch into chunks so that k_zstd_entropy of one chunk runs beside
 * k_zstd_match of the next (second HIP stream inside the context; the caller's stream still sees the whole
 * batch finished).  Returns how many launches of each kernel the last batch used. */
KMP_API int kmp_batch_last_chunks(kmp_batch_ctx* ctx);
/* Entropy sweeps of the last level-3 batch: k_zstd_entropy launches that code the slices the parse has finished while it is
 * still running, and a final one behind it.  Returns how many were launched, the final one included (0: the batch was coded by
 * plain launches; -1: error), and with profiling on writes the slices each coded into coded[0 .. min(cap, return)), in launch
 * order.  Synchronises with the batch. */
KMP_API int kmp_batch_last_sweeps(kmp_batch_ctx* ctx, uint32_t* coded, uint32_t cap);
/* A context for slices above 128 KiB compresses block by block (libzstd decides each block's size from the bytes
 * produced so far): block rounds of the last batch. */
KMP_API int kmp_batch_last_rounds(kmp_batch_ctx* ctx);
/* diagnostic (no reference counterpart): milliseconds of blocks x 256 threads x iters random 4-byte read + write pairs over the
 * device region [d_region, d_region + bytes) -- the access pattern of the level-3 parser's tables.  The rate differs between
 * regions of one device's HBM (tools/region_probe.py). */
KMP_API int kmp_debug_probe_region(void* d_region, size_t bytes, uint32_t blocks, uint32_t iters, float* ms, void* hip_stream);

/* The batch for callers that hold HOST memory (the JVM): slices h_src[in_off[i] .. + in_len[i]) of at most 128 KiB in, frames at
 * h_dst[out_off[i] ..) out (out_cap[i] bytes of room: kmp_zstd_compress_bound(in_len[i]) always suffices), out_len[i] = frame
 * size (0 with KMP_ERR_CAPACITY when the room was too small).  Levels -131072 .. 4 (0 = 3): what kmp_zstd_compress_batch_level serves
 * for one-block slices -- the frames are what ZstdCompressor(level) returns for each slice on its own; a level-4 batch's slices of
 * 16 KiB or less (that level's "greedy" size class) come back with out_len 0 and the call returns KMP_ERR_CAPACITY after every other
 * slice has been compressed.  out_len is written for every slice whatever the return value.
 * A small batch goes through pinned staging and one device batch.  A large level-3 batch (more than 2 * KMP_HOST_BATCH_SLICES slices)
 * goes through the pipelined bulk compressor: eight pieces that run side by side on the device (kmp_zstd_compress_batch_pieces), each
 * piece's copy in, kernels and copy out overlapping the others'.  Memory the caller has made page-stable -- kmp_host_register, or its
 * own pinned allocation -- is read and written by the device directly; pageable memory goes through pinned staging filled and emptied
 * by KMP_HOST_BULK_WORKERS host threads.  jni/zstd/BatchWrapper.cpp binds the calls for direct ByteBuffers.  Reference counterpart:
 * none -- the reference compresses one slice per call (ZstdWrapper.kt:35-46); this is the call a maintainer adds to hand the GPU a batch.
 * kmp_zstd_compress_stream itself coalesces the closing calls of concurrent contexts into such batches (KMP_COALESCE=0: off;
 * KMP_COALESCE_US: the gather window, default 150 microseconds; KMP_COALESCE_MAX: slices per batch, default 256). */
KMP_API int kmp_zstd_compress_host_batch(int device, int level, const void* h_src, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                         void* h_dst, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len);
/* frames in, content out (out_cap[i] = room, at most 128 KiB); status[i] = libzstd's error number for entry i, 0 = fine */
KMP_API int kmp_zstd_decompress_host_batch(int device, const void* h_src, const uint64_t* in_off, const uint32_t* in_len, uint32_t n,
                                           void* h_dst, const uint64_t* out_off, const uint32_t* out_cap, uint32_t* out_len, uint32_t* status);
/* Page-stable caller memory: pins [ptr, ptr + bytes) and maps it for the device (hipHostRegister), so that the host-batch calls read
 * slices from it and write frames into it over PCIe without a staging copy -- what the reference's JNI layer borrows and releases
 * around every call (GetByteArrayElements / ReleaseByteArrayElements, Wrapper.cpp:92-118), borrowed once for a buffer that outlives
 * many calls: a direct ByteBuffer a Kotlin caller reuses.  Unregister before the memory is freed. */
KMP_API int kmp_host_register(void* ptr, size_t bytes);
KMP_API int kmp_host_unregister(void* ptr);
/* Gives back what the host-batch calls and the coalescer of the streaming entry points hold on `device` (-1: every device): pinned
 * staging, device buffers, batch contexts.  The next call that needs them makes them again.  Not while such a call is running. */
KMP_API int kmp_host_engines_release(int device);

/* diagnostic (no reference counterpart): random 4-byte loads per second, and load + store-into-the-same-word pairs per second,
 * over the context's level-3 team tables where they lie, measured once when the context was created (both 0 for a context
 * whose tables are below 4 GiB).  bench.py prices the parser's measured memory requests with them. */
KMP_API int kmp_batch_table_rates(kmp_batch_ctx* ctx, float* reads_per_s, float* pairs_per_s);

/* diagnostic: the per-slice parser records (32 bytes each: sequences, literal bytes, trailing literals, long-length info, status and
 * two spare words -- with KMP_MATCH_FLAGS bit 8 the device's 100 MHz clock when the slice was finished) of the last one-block
 * zstd batch, copied to host memory after the device has gone idle */
KMP_API int kmp_debug_copy_meta(kmp_batch_ctx* ctx, void* h_dst, uint32_t n);

KMP_API const char* kmp_last_error(void);
KMP_API const char* kmp_version(void);

#ifdef __cplusplus
}
#endif
#endif
