"""Batched device API over torch CUDA(ROCm) tensors.  torch is plumbing here:
device memory and streams.  All compute happens in libkompressor_hip.so."""
import ctypes

import torch

from . import _lib


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def compress_bound(n: int) -> int:
    return _lib.load().kmp_zstd_compress_bound(n)


def compress_host_batch(slices, level=3, device=0):
    """kmp_zstd_compress_host_batch: slices held in HOST memory (a list of bytes-like objects of at most 128 KiB) -> their
    frames, through pinned staging and the device batch (the call jni/zstd/BatchWrapper.cpp binds for the JVM)."""
    import numpy as np
    lib = _lib.load()
    n = len(slices)
    lens = np.array([len(s) for s in slices], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    if n > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    src = np.frombuffer(b"".join(bytes(s) for s in slices) + b"\0", dtype=np.uint8)
    caps = np.array([compress_bound(int(l)) for l in lens], dtype=np.uint32)
    ooff = np.zeros(n, dtype=np.uint64)
    if n > 1:
        ooff[1:] = np.cumsum(caps[:-1], dtype=np.uint64)
    dst = np.empty(int(caps.sum()) + 1, dtype=np.uint8)
    olen = np.zeros(n, dtype=np.uint32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)          # noqa: E731
    rc = lib.kmp_zstd_compress_host_batch(device, level, p(src), p(offs), p(lens), n, p(dst), p(ooff), p(caps), p(olen))
    if rc != 0:
        raise RuntimeError(f"kmp_zstd_compress_host_batch failed ({rc}): {_lib.last_error()}")
    return [dst[int(ooff[i]):int(ooff[i]) + int(olen[i])].tobytes() for i in range(n)]


def frame_info_host(frames):
    """kmp_zstd_frame_info_host: what each entry's frames declare (ZSTD_findDecompressedSize, ZSTD_decompressBound, the first error
    of ZSTD_findFrameCompressedSize), parsed on the host, no GPU touched.  -> a numpy structured array with the fields of
    kmp_zstd_frame_info: content, bound, status, frames, dict_id, flags."""
    import numpy as np
    lib = _lib.load()
    n = len(frames)
    lens = np.array([len(f) for f in frames], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    if n > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    src = np.frombuffer(b"".join(bytes(f) for f in frames) + b"\0", dtype=np.uint8)
    info = np.zeros(n, dtype=np.dtype([("content", "<u8"), ("bound", "<u8"), ("status", "<u4"), ("frames", "<u4"), ("dict_id", "<u4"), ("flags", "<u4")]))
    p = lambda a: ctypes.c_void_p(a.ctypes.data)          # noqa: E731
    rc = lib.kmp_zstd_frame_info_host(p(src), p(offs), p(lens), n, p(info))
    if rc != 0:
        raise RuntimeError(f"kmp_zstd_frame_info_host failed ({rc}): {_lib.last_error()}")
    return info


def decompress_host_batch(frames, caps=None, device=0):
    """kmp_zstd_decompress_host_batch: frames in host memory -> (contents, statuses); caps[i] = room for entry i (<= 128 KiB).
    caps=None: the room is each entry's bound, read off its frames (frame_info_host); an entry that fails the inspection raises
    RuntimeError with libzstd's name for the error."""
    import numpy as np
    lib = _lib.load()
    n = len(frames)
    if caps is None:
        info = frame_info_host(frames)
        for i in range(n):
            if info["status"][i]:
                name = lib.kmp_zstd_get_error_name((1 << 64) - int(info["status"][i])).decode()
                raise RuntimeError(f"decompress_host_batch: entry {i} of {n}: {name}")
        if n and int(info["bound"].max()) >= (1 << 32):
            raise RuntimeError("decompress_host_batch: an entry's bound is 4 GiB or more")
        caps = info["bound"]
    lens = np.array([len(f) for f in frames], dtype=np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    if n > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    src = np.frombuffer(b"".join(bytes(f) for f in frames) + b"\0", dtype=np.uint8)
    caps = np.array(caps, dtype=np.uint32)
    ooff = np.zeros(n, dtype=np.uint64)
    if n > 1:
        ooff[1:] = np.cumsum(caps[:-1], dtype=np.uint64)
    dst = np.empty(int(caps.sum()) + 1, dtype=np.uint8)
    olen = np.zeros(n, dtype=np.uint32)
    st = np.zeros(n, dtype=np.uint32)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)          # noqa: E731
    rc = lib.kmp_zstd_decompress_host_batch(device, p(src), p(offs), p(lens), n, p(dst), p(ooff), p(caps), p(olen), p(st))
    if rc != 0:
        raise RuntimeError(f"kmp_zstd_decompress_host_batch failed ({rc}): {_lib.last_error()}")
    return [dst[int(ooff[i]):int(ooff[i]) + int(olen[i])].tobytes() for i in range(n)], [int(x) for x in st]


def host_register(array):
    """kmp_host_register over a numpy array's memory (pins it and maps it for the device); unregister with host_unregister before
    the array goes away."""
    rc = _lib.load().kmp_host_register(ctypes.c_void_p(array.ctypes.data), array.nbytes)
    if rc != 0:
        raise RuntimeError(f"kmp_host_register failed ({rc}): {_lib.last_error()}")


def host_unregister(array):
    rc = _lib.load().kmp_host_unregister(ctypes.c_void_p(array.ctypes.data))
    if rc != 0:
        raise RuntimeError(f"kmp_host_unregister failed ({rc}): {_lib.last_error()}")


def host_engines_release(device=-1):
    """kmp_host_engines_release: the pinned staging, device buffers and contexts behind the host-batch calls and the coalescer."""
    rc = _lib.load().kmp_host_engines_release(device)
    if rc != 0:
        raise RuntimeError(f"kmp_host_engines_release failed ({rc}): {_lib.last_error()}")


class SeekableReader:
    """A seekable zstd container in device memory, opened by ZstdBatch.open_seekable (kmp_zstd_seekable_open: the table is validated on
    the device and read back once).  frames / content_size / checksums / max_frame are the table's; status is libzstd's number for a
    table that was rejected (10 or 20: then every read raises)."""

    def __init__(self, batch, blob):
        self.batch, self.blob = batch, blob
        h = ctypes.c_void_p()
        rc = batch.lib.kmp_zstd_seekable_open(batch._h, _ptr(blob), blob.numel(), ctypes.byref(h), batch._stream())
        if rc != 0:
            raise RuntimeError(f"kmp_zstd_seekable_open failed ({rc}): {batch._err()}")
        self._h = h
        st = _lib.SeekableStat()
        batch.lib.kmp_zstd_seekable_stat(h, ctypes.byref(st))
        self.status, self.frames, self.content_size, self.max_frame = int(st.status), int(st.frames), int(st.content), int(st.max_frame)
        self.checksums = bool(st.flags & 1)

    def close(self):
        if getattr(self, "_h", None):
            self.batch.lib.kmp_zstd_seekable_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def read_frames(self, lo, hi, verify=True):
        """kmp_zstd_seekable_read, queued with no host wait: the frames covering [lo, hi) decoded whole into one buffer.
        -> (dst, skip, status): the bytes asked for are dst[skip : skip + hi - lo]; status: int32 device tensor, one per covering frame
        (0, libzstd's error code, 22 for a checksum that does not match under verify)."""
        lib, b = self.batch.lib, self.batch
        if self.status:
            raise RuntimeError(f"the container's seek table was rejected (status {self.status})")
        need = lib.kmp_zstd_seekable_read_bound(self._h, lo, hi)
        m = lib.kmp_zstd_seekable_read_frames(self._h, lo, hi, None)
        dst = torch.empty(need + 64, dtype=torch.uint8, device=b.device)
        status = torch.zeros(max(m, 1), dtype=torch.int32, device=b.device)
        skip = ctypes.c_uint64()
        rc = lib.kmp_zstd_seekable_read(self._h, _ptr(self.blob), lo, hi, 1 if verify else 0, _ptr(dst), need, ctypes.byref(skip), _ptr(status), b._stream())
        if rc != 0:
            raise RuntimeError(f"kmp_zstd_seekable_read failed ({rc}): {b._err()}")
        return dst, int(skip.value), status[:m]

    def read(self, lo, hi, verify=True):
        """Bytes [lo, hi) of the content (hi is cut at the content's end): a uint8 device tensor view of exactly that many bytes.
        verify: on a container with checksums, compare every decoded frame's XXH64 with its entry.  Reads the frames' statuses back
        (a host wait) and raises on a nonzero one."""
        if self.status:
            raise RuntimeError(f"the container's seek table was rejected (status {self.status})")
        hi = min(hi, self.content_size)
        if lo >= hi:
            return torch.empty(0, dtype=torch.uint8, device=self.batch.device)
        dst, skip, status = self.read_frames(lo, hi, verify)
        bad = torch.nonzero(status).flatten().tolist()
        if bad:
            codes = status.tolist()
            raise RuntimeError(f"seekable read [{lo}, {hi}): frame status " + ", ".join(f"+{i}: {codes[i]}" for i in bad[:8]))
        return dst[skip:skip + hi - lo]

    def read_all(self, verify=True):
        return self.read(0, self.content_size, verify)


class BgzfReader:
    """A BGZF container in device memory, opened by ZstdBatch.open_bgzf (kmp_bgzf_open: the members are found on the device, the stat and
    both prefix sums read back).  stat: the _lib.BgzfStat; status is zlib's number for a blob that was rejected (-3 or -5: then every
    read raises)."""

    def __init__(self, batch, blob):
        self.batch, self.blob = batch, blob
        h = ctypes.c_void_p()
        rc = batch.lib.kmp_bgzf_open(batch._h, _ptr(blob) if blob.numel() else None, blob.numel(), ctypes.byref(h), batch._stream())
        if rc != 0:
            raise RuntimeError(f"kmp_bgzf_open failed ({rc}): {batch._err()}")
        self._h = h
        self.stat = _lib.BgzfStat()
        batch.lib.kmp_bgzf_stat_of(h, ctypes.byref(self.stat))
        self.status, self.blocks, self.content_size = int(self.stat.status), int(self.stat.blocks), int(self.stat.content)

    def close(self):
        if getattr(self, "_h", None):
            self.batch.lib.kmp_bgzf_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def tell(self, pos):
        """BGZF's virtual offset of content position pos (kmp_bgzf_tell): member start << 16 | offset inside the member's content"""
        v = self.batch.lib.kmp_bgzf_tell(self._h, pos)
        if v == (1 << 64) - 1:
            raise ValueError(f"position {pos} lies outside the content, or the blob was rejected")
        return v

    def read_blocks(self, lo, hi, verify=True):
        """kmp_bgzf_read, queued with no host wait: the members covering [lo, hi) decoded whole into one buffer.
        -> (dst, skip, status): the bytes asked for are dst[skip : skip + hi - lo]; status: int32 device tensor, one per covering member
        (0, zlib's number, -3 for a size or -- under verify -- a CRC-32 that does not match the trailer)."""
        lib, b = self.batch.lib, self.batch
        if self.status:
            raise RuntimeError(f"the BGZF blob was rejected (status {self.status})")
        need = lib.kmp_bgzf_read_bound(self._h, lo, hi)
        m = lib.kmp_bgzf_read_blocks(self._h, lo, hi, None)
        dst = torch.empty(need + 64, dtype=torch.uint8, device=b.device)
        status = torch.zeros(max(m, 1), dtype=torch.int32, device=b.device)
        skip = ctypes.c_uint64()
        rc = lib.kmp_bgzf_read(self._h, _ptr(self.blob), lo, hi, 1 if verify else 0, _ptr(dst), need, ctypes.byref(skip), _ptr(status), b._stream())
        if rc != 0:
            raise RuntimeError(f"kmp_bgzf_read failed ({rc}): {b._err()}")
        return dst, int(skip.value), status[:m]

    def read(self, lo, hi, verify=True):
        """Bytes [lo, hi) of the content (hi is cut at the content's end): a uint8 device tensor view of exactly that many bytes.
        verify: compare every decoded member's CRC-32 with its trailer.  Reads the members' statuses back (a host wait) and raises on a
        nonzero one."""
        if self.status:
            raise RuntimeError(f"the BGZF blob was rejected (status {self.status})")
        hi = min(hi, self.content_size)
        if lo >= hi:
            return torch.empty(0, dtype=torch.uint8, device=self.batch.device)
        dst, skip, status = self.read_blocks(lo, hi, verify)
        bad = torch.nonzero(status).flatten().tolist()
        if bad:
            codes = status.tolist()
            raise RuntimeError(f"BGZF read [{lo}, {hi}): member status " + ", ".join(f"+{i}: {codes[i]}" for i in bad[:8]))
        return dst[skip:skip + hi - lo]

    def read_all(self, verify=True):
        return self.read(0, self.content_size, verify)


class ZstdBatch:
    """Owns the device workspace for batches of up to `max_slices` slices of up to
    `max_slice_bytes` bytes (<= 128 KiB) on one GPU."""

    def __init__(self, max_slices, max_slice_bytes=65536, device=None, team_lanes=0, ablations=False, table_span_gib=None, table_retry=None):
        """table_span_gib / table_retry: kmp_batch_options (None = the environment's KMP_TABLE_SPAN_GIB / KMP_TABLE_RETRY, else the
        library's defaults: a span of 100 GiB bounded by half of the free memory, no second arena)."""
        # ablations=True: the library's ablation build (tests and A/B tools only: kompressor_amd/_lib.py load_ablations)
        self.lib = _lib.load_ablations() if ablations else _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("kompressor_amd needs a ROCm GPU (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.max_slices = max_slices
        self.max_slice_bytes = max_slice_bytes
        h = ctypes.c_void_p()
        opts = _lib.BatchOptions(ctypes.sizeof(_lib.BatchOptions), team_lanes, -1 if table_span_gib is None else int(table_span_gib),
                                 -1 if table_retry is None else int(table_retry))
        rc = self.lib.kmp_batch_create_ex(ctypes.byref(h), self.device.index, max_slices, max_slice_bytes, ctypes.byref(opts))
        if rc != 0:
            raise RuntimeError(f"kmp_batch_create failed ({rc}): {self._err()}")
        self._h = h
        self.out_stride = (compress_bound(max_slice_bytes) + 8 + 63) & ~63

    def _err(self):
        return self.lib.kmp_last_error().decode()

    def close(self):
        if getattr(self, "_h", None):
            self.lib.kmp_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def status(self):
        """Waits for the batches queued so far and returns (rc, bits): KMP_STATUS_* bits raised on the device since the
        last call (1 = a slice longer than the context holds, 2 = a parser guard tripped, 4 = a slice of 16 KiB or less in a
        level-4 batch); such slices have out_len 0."""
        bits = ctypes.c_uint32()
        rc = self.lib.kmp_batch_status(self._h, ctypes.byref(bits), self._stream())
        return rc, bits.value

    def memory(self):
        """kmp_batch_memory: device bytes the context holds right now, by part (a dict)."""
        m = _lib.BatchMemoryInfo(); m.struct_bytes = ctypes.sizeof(m)
        if self.lib.kmp_batch_memory(self._h, ctypes.byref(m)) != 0:
            raise RuntimeError(self._err())
        return {k: int(getattr(m, k)) for k, _ in m._fields_[2:]}

    def table_rates(self):
        """(random loads per second, load + store pairs per second) over this context's level-3 team tables, measured at creation."""
        r, q = ctypes.c_float(), ctypes.c_float()
        if self.lib.kmp_batch_table_rates(self._h, ctypes.byref(r), ctypes.byref(q)) != 0:
            raise RuntimeError(self._err())
        return r.value, q.value

    def set_profiling(self, on=True):
        self.lib.kmp_batch_set_profiling(self._h, 1 if on else 0)

    def last_kernel_ms(self, which):
        ms = ctypes.c_float()
        rc = self.lib.kmp_batch_last_kernel_ms(self._h, which, ctypes.byref(ms))
        if rc != 0:
            raise RuntimeError(self._err())
        return ms.value

    def last_chunks(self):
        """Launches of each zstd compress kernel in the last batch."""
        return int(self.lib.kmp_batch_last_chunks(self._h))

    def last_sweeps(self):
        """Slices coded by each entropy sweep of the last level-3 batch, in launch order, the final sweep last (counted with
        profiling on, else zeros); [] when the batch was coded by plain launches."""
        buf = (ctypes.c_uint32 * 32)()
        k = int(self.lib.kmp_batch_last_sweeps(self._h, buf, 32))
        if k < 0:
            raise RuntimeError(self._err())
        return [int(buf[i]) for i in range(min(k, 32))]

    def _check(self, what):
        """check=True of compress / deflate: wait for the batch and raise on a status bit (a slice longer than the context
        holds, a parser guard) instead of handing back frames of length 0."""
        rc, bits = self.status()
        if rc != 0:
            raise RuntimeError(f"{what}: status bits {bits:#x} ({rc}): {self._err()}")

    FRAME_CHECKSUM, FRAME_NO_CONTENT_SIZE, FRAME_NO_DICT_ID = 1, 2, 4          # KMP_FRAME_*

    def set_frame_flags(self, flags):
        """kmp_batch_set_frame_flags: what the zstd compress batches queued from now on write around their blocks (FRAME_* bits)."""
        rc = self.lib.kmp_batch_set_frame_flags(self._h, flags)
        if rc != 0:
            raise ValueError(f"kmp_batch_set_frame_flags failed ({rc}): {self._err()}")

    def frame_flags(self):
        return int(self.lib.kmp_batch_frame_flags(self._h))

    def compress(self, src, in_off, in_len, dst=None, out_off=None, out_len=None, dictionary=None, level=3, streaming=None, reference=False, check=False,
                 checksum=False, content_size=True, dict_id=True):
        """src: uint8 device tensor; in_off int64, in_len int32 device tensors (n each).  dictionary: bytes of a
        dictionary shared by all slices (host memory; raw content, or zstd's own format -- magic EC30A437 -- with its tables,
        repeat offsets and ID; levels 1, 2, 3 and the negative ones, slices up to 128 KiB; its tables are built once per dictionary and
        level class -- 3, 1, 2, negative -- and the context keeps the last four).
        level: 3 (default); 1 / 2 / a negative level at any size the context holds (with a dictionary: up to 128 KiB); 4 up to 128 KiB and above
        256 KiB; 5 .. 10 (libzstd's greedy / lazy / lazy2 parsers) for slices up to 128 KiB and, on a context created for larger slices, up to
        2 MiB (frames of several blocks, as ZSTD_compress2 writes them) -- at 9 and 10 a slice of 8 bytes .. 16 KiB is another strategy and
        comes back refused (out_len 0, status bit 4), as do a slice above 2 MiB at levels 5 .. 10 and, with reference=True, a level-4 slice between 128 and 256 KiB (one-shot frames of that size are served: libzstd's "greedy" row, on
        the chain kernel of levels 5 .. 10).
        streaming: None = one-shot frames; "data" / "empty" = the frames of slices that arrived through finish = false
        calls, closed by a call with / without data (context created for slices above 128 KiB; levels 1 to 4 and the negative ones at
        any length, 5 .. 10 for streams of 0 .. 2 MiB -- a longer one comes back refused: out_len 0, status bit 4).
        reference: the frames ZstdCompressor(level).transform(bytes) returns -- above 128 KiB the reference's output slices
        make libzstd stage the input in 128 KiB chunks, so they differ from ZSTD_compress2's (the default here) wherever
        the block pre-splitter cuts (no dictionary); up to 128 KiB both are the same.  Levels 5 .. 10: up to 2 MiB, as above.
        checksum / content_size / dict_id: libzstd's checksumFlag (the low 32 bits of the content's XXH64 behind the last block),
        contentSizeFlag (False: no content size in the header, a window descriptor instead; decode such frames with out_cap) and dictIDFlag
        (False: a formatted dictionary's ID is left out).  Given here they hold for this call: the context's flags (set_frame_flags) are put
        back before it returns; left at their defaults the call writes what the context's flags say.
        Returns (dst, out_off, out_len): frame i = dst[out_off[i] : out_off[i] + out_len[i]]."""
        n = in_len.numel()
        if dst is None:
            dst = torch.empty(n * self.out_stride + 64, dtype=torch.uint8, device=self.device)
        if out_off is None:
            out_off = torch.arange(n, dtype=torch.int64, device=self.device) * self.out_stride
        if out_len is None:
            out_len = torch.zeros(n, dtype=torch.int32, device=self.device)
        flags = (self.FRAME_CHECKSUM if checksum else 0) | (0 if content_size else self.FRAME_NO_CONTENT_SIZE) | (0 if dict_id else self.FRAME_NO_DICT_ID)
        if flags:
            held = self.frame_flags()
            self.set_frame_flags(flags)
            try:                    # (a batch takes the flags when it is queued: they can go back at once)
                return self.compress(src, in_off, in_len, dst, out_off, out_len, dictionary, level, streaming, reference, check)
            finally:
                self.set_frame_flags(held)
        if reference and streaming is None:
            if dictionary is not None:
                raise ValueError("reference=True is served without a dictionary")
            rc = self.lib.kmp_zstd_compress_batch_reference(self._h, _ptr(src), _ptr(in_off), _ptr(in_len), n,
                                                            _ptr(dst), _ptr(out_off), _ptr(out_len), level, 0, self._stream())
        elif streaming is not None:
            rc = self.lib.kmp_zstd_compress_batch_stream_level(self._h, _ptr(src), _ptr(in_off), _ptr(in_len), n,
                                                               _ptr(dst), _ptr(out_off), _ptr(out_len), 1 if streaming == "empty" else 0, level, self._stream())
        elif dictionary is not None:
            if level > 3:
                raise ValueError("levels 4 .. 10 are served without a dictionary")
            rc = self.lib.kmp_zstd_compress_batch_dict_level(self._h, _ptr(src), _ptr(in_off), _ptr(in_len), n,
                                                             _ptr(dst), _ptr(out_off), _ptr(out_len), bytes(dictionary), len(dictionary), level, self._stream())
        elif level not in (0, 3):
            rc = self.lib.kmp_zstd_compress_batch_level(self._h, _ptr(src), _ptr(in_off), _ptr(in_len), n,
                                                        _ptr(dst), _ptr(out_off), _ptr(out_len), level, self._stream())
        else:
            rc = self.lib.kmp_zstd_compress_batch(self._h, _ptr(src), _ptr(in_off), _ptr(in_len), n,
                                                  _ptr(dst), _ptr(out_off), _ptr(out_len), self._stream())
        if rc != 0:
            raise RuntimeError(f"kmp_zstd_compress_batch failed ({rc}): {self._err()}")
        if check:
            self._check("kmp_zstd_compress_batch")
        return dst, out_off, out_len

    def compress_seekable(self, src, frame_bytes=65536, level=3, checksums=True):
        """One buffer (uint8 device tensor) -> a seekable zstd container (kmp_zstd_seekable_compress): independent frames of frame_bytes
        (1 .. 131 072, at most the context's max_slice_bytes; at most max_slices of them) at `level` (-131072 .. 8), then the seek table
        with, by default, each frame's XXH64 checksum.  Any zstd decoder decodes the result; open_seekable reads byte ranges of it.
        Returns a uint8 device tensor trimmed to the container: the one host wait is the .item() that reads its size to trim it."""
        n = src.numel()
        flags = 1 if checksums else 0
        cap = self.lib.kmp_zstd_seekable_bound(n, frame_bytes, flags)
        need = self.lib.kmp_zstd_seekable_scratch(n, frame_bytes)
        if cap == 0:
            raise ValueError("frame_bytes must be 1 .. 131072")
        dst = torch.empty(cap + 64, dtype=torch.uint8, device=self.device)
        scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=self.device)
        result = torch.zeros(2, dtype=torch.int64, device=self.device)
        rc = self.lib.kmp_zstd_seekable_compress(self._h, _ptr(src) if n else None, n, frame_bytes, level, flags, _ptr(dst), cap, _ptr(scratch), need,
                                                 _ptr(result), self._stream())
        if rc != 0:
            raise RuntimeError(f"kmp_zstd_seekable_compress failed ({rc}): {self._err()}")
        size = int(result[0].item())
        if size == 0:
            raise RuntimeError(f"kmp_zstd_seekable_compress: a chunk got no frame (status bits {int(result[1].item()):#x})")
        return dst[:size]

    def open_seekable(self, blob):
        """A SeekableReader over a container in device memory (uint8 tensor; it must stay alive while the reader is used)."""
        return SeekableReader(self, blob)

    def compress_bgzf(self, src, block_bytes=65280, level=6, eof=True):
        """One buffer (uint8 device tensor) -> a BGZF container (kmp_bgzf_compress): a gzip member per block of block_bytes (1 .. 65 280,
        at most the context's max_slice_bytes; at most max_slices of them) at zlib's `level` (1 .. 9, -1 = 6), then the end-of-file
        marker unless eof is False (rounds over a larger buffer: concatenate them, the last one with eof).  gunzip and every BGZF reader
        decode the result; open_bgzf reads byte ranges of it.  Returns a uint8 device tensor trimmed to the container: the one host
        wait is the .item() that reads its size to trim it."""
        n = src.numel()
        flags = 0 if eof else 1
        cap = self.lib.kmp_bgzf_bound(n, block_bytes, flags)
        need = self.lib.kmp_bgzf_scratch(n, block_bytes)
        if need == 0:
            raise ValueError("block_bytes must be 1 .. 65280")
        dst = torch.empty(cap + 64, dtype=torch.uint8, device=self.device)
        scratch = torch.empty((need + 7) // 8, dtype=torch.int64, device=self.device)
        result = torch.zeros(2, dtype=torch.int64, device=self.device)
        rc = self.lib.kmp_bgzf_compress(self._h, _ptr(src) if n else None, n, block_bytes, level, flags, _ptr(dst), cap, _ptr(scratch), need,
                                        _ptr(result), self._stream())
        if rc != 0:
            raise RuntimeError(f"kmp_bgzf_compress failed ({rc}): {self._err()}")
        size = int(result[0].item())
        if size == 0 and (n or eof):
            raise RuntimeError(f"kmp_bgzf_compress: a block got no member (status bits {int(result[1].item()):#x})")
        return dst[:size]

    def open_bgzf(self, blob):
        """A BgzfReader over a BGZF container in device memory (uint8 tensor; it must stay alive while the reader is used)."""
        return BgzfReader(self, blob)

    def piece_range(self, n, pieces, piece):
        """(first, count) of part `piece` of an n-slice batch cut into `pieces` (kmp_batch_piece_range)."""
        a, b = ctypes.c_uint32(), ctypes.c_uint32()
        self.lib.kmp_batch_piece_range(n, pieces, piece, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    def compress_pieces(self, src, in_off, in_len, dst, out_off, out_len, streams):
        """kmp_zstd_compress_batch_pieces: the level-3 batch in len(streams) parts that run side by side, part p queued on the torch
        stream streams[p] behind whatever the caller queued there (the copy that brings the part's slices in)."""
        n = in_len.numel()
        arr = (ctypes.c_void_p * len(streams))(*[s.cuda_stream for s in streams])
        rc = self.lib.kmp_zstd_compress_batch_pieces(self._h, _ptr(src), _ptr(in_off), _ptr(in_len), n, _ptr(dst), _ptr(out_off), _ptr(out_len), len(streams), arr)
        if rc != 0:
            raise RuntimeError(f"kmp_zstd_compress_batch_pieces failed ({rc}): {self._err()}")
        return dst, out_off, out_len

    def compact_piece(self, src, in_off, lens, first, count, dst, offs, stream):
        """Dense packing of one part on `stream`: frames first .. first + count of the strided layout go to dst (a buffer of the part's
        own) back to back; offs (int64, count + 1 entries) receives the exclusive scan, offs[count] the part's bytes."""
        rc = self.lib.kmp_compact_batch(self._h, _ptr(src), ctypes.c_void_p(in_off.data_ptr() + 8 * first), ctypes.c_void_p(lens.data_ptr() + 4 * first), count,
                                        _ptr(dst), _ptr(offs), ctypes.c_void_p(stream.cuda_stream))
        if rc != 0:
            raise RuntimeError(f"kmp_compact_batch failed ({rc}): {self._err()}")

    def _frame_info_raw(self, src, in_off, in_len):
        """kmp_zstd_frame_info_batch -> the n x 32 bytes of kmp_zstd_frame_info as an int64 tensor of n x 4 (queued, no host wait)"""
        n = in_len.numel()
        info = torch.empty((n, 4), dtype=torch.int64, device=self.device)
        rc = self.lib.kmp_zstd_frame_info_batch(self._h, _ptr(src), _ptr(in_off), _ptr(in_len), n, _ptr(info), self._stream())
        if rc != 0:
            raise RuntimeError(f"kmp_zstd_frame_info_batch failed ({rc}): {self._err()}")
        return info

    def frame_info(self, src, in_off, in_len):
        """What each entry's frames declare, read on the device without decoding (kmp_zstd_frame_info_batch: the batched
        ZSTD_findDecompressedSize / ZSTD_decompressBound / ZSTD_findFrameCompressedSize; no host wait).  Returns a dict of device
        tensors over the n entries (views of one buffer): content and bound (int64; an unknown content size, ~0 in C, reads -1),
        status (0 or libzstd's error code: then content and bound are 0), frames, dict_id, flags (int32; bit 0 a checksum, bit 1 a
        skippable frame, bit 2 a frame in a format of zstd 0.5 .. 0.7)."""
        info = self._frame_info_raw(src, in_off, in_len)
        w = info.view(torch.int32)                      # n x 8 words
        return {"content": info[:, 0], "bound": info[:, 1], "status": w[:, 4], "frames": w[:, 5], "dict_id": w[:, 6], "flags": w[:, 7]}

    def layout(self, info, align=1):
        """kmp_batch_layout over the tensor _frame_info_raw returns: (out_off int64, out_cap int32, total int64[2]) on the device, no
        host wait: capacities = bounds (0 for a rejected entry or a bound of 4 GiB and more), offsets = their running sum with each
        rounded up to align, total[0] = the bytes a destination needs, total[1] = the entries given capacity 0 for those reasons."""
        n = info.shape[0]
        out_off = torch.empty(n, dtype=torch.int64, device=self.device)
        out_cap = torch.empty(n, dtype=torch.int32, device=self.device)
        total = torch.empty(2, dtype=torch.int64, device=self.device)
        rc = self.lib.kmp_batch_layout(self._h, _ptr(info), n, align, _ptr(out_off), _ptr(out_cap), _ptr(total), self._stream())
        if rc != 0:
            raise RuntimeError(f"kmp_batch_layout failed ({rc}): {self._err()}")
        return out_off, out_cap, total

    def decompress(self, src, in_off, in_len, out_cap=None, dst=None, out_off=None, dictionary=None, align=1):
        """Frames -> slices.  out_cap: int32 device tensor of per-frame capacities.  dictionary: uint8 device tensor
        with a raw-content dictionary shared by all frames.  Returns (dst, out_off, out_len, status).
        out_cap=None: the sizes are read off the frames on the device (frame_info, then layout with `align`: a power of two up to
        4096 that every out_off is a multiple of); the one host wait is reading the total back to allocate dst.  An entry whose
        inspection fails (or whose bound is 4 GiB or more) gets capacity 0, and the decoder's own status for it is nonzero.
        Frames without a declared size get their bound: blocks x min(window, 128 KiB)."""
        n = in_len.numel()
        if out_cap is None:
            if dst is not None or out_off is not None:
                raise ValueError("out_cap=None lays the destination out itself: pass neither dst nor out_off")
            out_off, out_cap, total = self.layout(self._frame_info_raw(src, in_off, in_len), align)
            dst = torch.empty(int(total[0].item()) + 64, dtype=torch.uint8, device=self.device)
        elif align != 1:
            raise ValueError("align belongs to out_cap=None (with out_cap given, out_off is the caller's)")
        if out_off is None:
            out_off = torch.cumsum(out_cap.to(torch.int64), 0) - out_cap.to(torch.int64)
        if dst is None:
            total = int(out_cap.to(torch.int64).sum().item())
            dst = torch.empty(total + 64, dtype=torch.uint8, device=self.device)
        out_len = torch.zeros(n, dtype=torch.int32, device=self.device)
        status = torch.zeros(n, dtype=torch.int32, device=self.device)
        if dictionary is not None:
            rc = self.lib.kmp_zstd_decompress_batch_dict(self._h, _ptr(src), _ptr(in_off), _ptr(in_len), n,
                                                         _ptr(dst), _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status),
                                                         _ptr(dictionary), dictionary.numel(), self._stream())
        else:
            rc = self.lib.kmp_zstd_decompress_batch(self._h, _ptr(src), _ptr(in_off), _ptr(in_len), n,
                                                    _ptr(dst), _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status),
                                                    self._stream())
        if rc != 0:
            raise RuntimeError(f"kmp_zstd_decompress_batch failed ({rc}): {self._err()}")
        return dst, out_off, out_len, status

    _FORMATS = {"raw": 0, "zlib": 1, "gzip": 2, "auto": 3}

    def _inflate_info_raw(self, src, in_off, in_len, fmt):
        """kmp_inflate_info_batch -> the n x 32 bytes of kmp_inflate_info as an int64 tensor of n x 4 (queued, no host wait)"""
        n = in_len.numel()
        info = torch.empty((n, 4), dtype=torch.int64, device=self.device)
        rc = self.lib.kmp_inflate_info_batch(self._h, _ptr(src), _ptr(in_off), _ptr(in_len), n, _ptr(info), fmt, self._stream())
        if rc != 0:
            raise RuntimeError(f"kmp_inflate_info_batch failed ({rc}): {self._err()}")
        return info

    def inflate_info(self, src, in_off, in_len, format="raw"):   # noqa: A002
        """How large each DEFLATE stream decodes to, walked on the device without decoding (kmp_inflate_info_batch; no host wait).
        Returns a dict of device tensors over the n entries (views of one buffer): content and bound (int64, equal), status (int32:
        0, -3 or -5; then every other field is 0), blocks, flags (bit 0 a stored block, 1 a fixed one, 2 a dynamic one, 3 gzip, 4 a
        gzip header with optional fields), window_bits (int32).  The trailers' Adler-32 / CRC-32 values are not verified: inflate
        reports them."""
        info = self._inflate_info_raw(src, in_off, in_len, self._FORMATS[format])
        w = info.view(torch.int32)                      # n x 8 words
        return {"content": info[:, 0], "bound": info[:, 1], "status": w[:, 4], "blocks": w[:, 5], "flags": w[:, 6], "window_bits": w[:, 7]}

    def inflate(self, src, in_off, in_len, out_cap=None, zlib_wrapper=False, dst=None, out_off=None, format=None, align=1):   # noqa: A002
        """n DEFLATE streams -> slices; format "raw" / "zlib" / "gzip" / "auto" (zlib or gzip per stream).
        Returns (dst, out_off, out_len, status).
        out_cap=None: the sizes are found on the device (inflate_info, then layout with `align`: a power of two up to 4096 that every
        out_off is a multiple of); the one host wait is reading the total back to allocate dst.  An entry the sizing pass rejects (or
        that decodes to 4 GiB or more) gets capacity 0, and the decoder's own status for it is nonzero."""
        fmt = self._FORMATS[format] if format is not None else (1 if zlib_wrapper else 0)
        n = in_len.numel()
        if out_cap is None:
            if dst is not None or out_off is not None:
                raise ValueError("out_cap=None lays the destination out itself: pass neither dst nor out_off")
            out_off, out_cap, total = self.layout(self._inflate_info_raw(src, in_off, in_len, fmt), align)
            dst = torch.empty(int(total[0].item()) + 64, dtype=torch.uint8, device=self.device)
        elif align != 1:
            raise ValueError("align belongs to out_cap=None (with out_cap given, out_off is the caller's)")
        if out_off is None:
            out_off = torch.cumsum(out_cap.to(torch.int64), 0) - out_cap.to(torch.int64)
        if dst is None:
            dst = torch.empty(int(out_cap.to(torch.int64).sum().item()) + 64, dtype=torch.uint8, device=self.device)
        out_len = torch.zeros(n, dtype=torch.int32, device=self.device)
        status = torch.zeros(n, dtype=torch.int32, device=self.device)
        rc = self.lib.kmp_inflate_batch(self._h, _ptr(src), _ptr(in_off), _ptr(in_len), n, _ptr(dst), _ptr(out_off), _ptr(out_cap),
                                        _ptr(out_len), _ptr(status), fmt, self._stream())
        if rc != 0:
            raise RuntimeError(f"kmp_inflate_batch failed ({rc}): {self._err()}")
        return dst, out_off, out_len, status

    def deflate(self, src, in_off, in_len, dst=None, out_off=None, out_len=None, zlib_wrapper=False, format=None, level=6, check=False,   # noqa: A002
                window_bits=15, mem_level=8):
        """DEFLATE streams (zlib level 6 -- or any other level 1 .. 9: deflate_fast 1 .. 3, deflate_slow 4 .. 9 --; windowBits 9 .. 15 and
        memLevel 1 .. 9 as deflateInit2 takes them, 15 and 8 by default), format "raw" / "zlib" / "gzip", for slices up to the context's
        max_slice_bytes (64 KiB at least)."""
        fmt = self._FORMATS[format] if format is not None else (1 if zlib_wrapper else 0)
        if fmt == 3:
            raise ValueError("Compression can't be used with auto-detection")       # ZlibFormat.kt:28
        n = in_len.numel()
        params = (window_bits, mem_level) != (15, 8)
        stride = (self.lib.kmp_deflate_bound_params(max(self.max_slice_bytes, 65536), window_bits, mem_level) + 63) & ~63
        if dst is None:
            dst = torch.empty(n * stride + 64, dtype=torch.uint8, device=self.device)
        if out_off is None:
            out_off = torch.arange(n, dtype=torch.int64, device=self.device) * stride
        if out_len is None:
            out_len = torch.zeros(n, dtype=torch.int32, device=self.device)
        if params:
            rc = self.lib.kmp_deflate_compress_batch_params(self._h, _ptr(src), _ptr(in_off), _ptr(in_len), n, _ptr(dst), _ptr(out_off), _ptr(out_len),
                                                            fmt, level, window_bits, mem_level, self._stream())
        elif level in (-1, 6):
            fn = (self.lib.kmp_deflate_compress_batch, self.lib.kmp_zlib_compress_batch, self.lib.kmp_gzip_compress_batch)[fmt]
            rc = fn(self._h, _ptr(src), _ptr(in_off), _ptr(in_len), n, _ptr(dst), _ptr(out_off), _ptr(out_len), self._stream())
        else:
            rc = self.lib.kmp_deflate_compress_batch_level(self._h, _ptr(src), _ptr(in_off), _ptr(in_len), n, _ptr(dst), _ptr(out_off), _ptr(out_len),
                                                           fmt, level, self._stream())
        if rc != 0:
            raise RuntimeError(f"kmp_deflate_compress_batch failed ({rc}): {self._err()}")
        if check:
            self._check("kmp_deflate_compress_batch")
        return dst, out_off, out_len

    def deflate_kernel_ms(self):
        ms = (ctypes.c_float * 4)()
        if self.lib.kmp_deflate_last_kernel_ms(self._h, ms) != 0:
            raise RuntimeError(self._err())
        # the four stages of the first workspace piece; which kernels they are depends on the level and the slice size:
        #   prepare: k_deflate_sort + the heaviest-first order (slices <= 64 KiB, levels >= 4) | k_deflate_chains (longer slices)
        #   search : nothing                                                                  | k_deflate_best
        #   parse  : k_deflate_lazy                                                           | k_deflate_parse;  levels 1 .. 3: k_deflate_fast
        #   encode : k_deflate_encode
        return dict(zip(("prepare", "search", "parse", "encode"), (float(x) for x in ms)))

    def compact_into(self, src, in_off, lens, dst, offs):
        """Dense packing into caller-owned buffers, no host round trip: frame i goes to dst[offs[i] : offs[i] + lens[i]],
        offs (int64, n + 1 entries) = exclusive scan of lens, offs[n] = total bytes.  dst must hold sum(lens) bytes."""
        n = lens.numel()
        if offs.numel() < n + 1:
            raise ValueError("offs needs n + 1 entries")
        rc = self.lib.kmp_compact_batch(self._h, _ptr(src), _ptr(in_off), _ptr(lens), n, _ptr(dst), _ptr(offs), self._stream())
        if rc != 0:
            raise RuntimeError(f"kmp_compact_batch failed ({rc}): {self._err()}")
        return dst, offs

    def compact(self, src, in_off, lens):
        """Dense packing of n frames; returns (dst, offsets[n+1])."""
        n = lens.numel()
        offs = torch.empty(n + 1, dtype=torch.int64, device=self.device)
        total_cap = int(lens.to(torch.int64).sum().item())
        dst = torch.empty(total_cap + 64, dtype=torch.uint8, device=self.device)
        rc = self.lib.kmp_compact_batch(self._h, _ptr(src), _ptr(in_off), _ptr(lens), n, _ptr(dst), _ptr(offs), self._stream())
        if rc != 0:
            raise RuntimeError(f"kmp_compact_batch failed ({rc}): {self._err()}")
        return dst, offs
