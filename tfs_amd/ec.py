"""ctypes binding of include/tfs_ec.h -- the GPU erasure code.

Mirrors tfs::dataserver::ErasureCode (src/dataserver/erasure_code.h): config(dn,
pn, erased) then encode(size) / decode(size) over dn + pn member buffers.  The
region work runs in libtfs_crc.so's gfx950 kernels; no CPU fallback.
"""
import ctypes

import numpy as np

from . import crc as _crc

TFS_EXIT_NO_MEMORY = -16000
TFS_EXIT_DATA_INVALID = -16001
TFS_EXIT_SIZE_INVALID = -16002
TFS_EXIT_MATRIX_INVALID = -16003
TFS_EXIT_NO_ENOUGH_DATA = -16004
UNIT = 1024  # ws_ * ps_ (erasure_code.cpp:33-34)
READ_RANGE = 1  # TFS_EC_READ_RANGE
READ_JOB_DTYPE = np.dtype([("file_id", "<u8"), ("out_offset", "<u8"), ("offset", "<i4"), ("size", "<i4"),
                           ("flags", "<u4"), ("reserved", "<u4")])  # tfs_ec_read_job
assert READ_JOB_DTYPE.itemsize == 32
# tfs_ec_reply_job (include/tfs_ec_read.h): a tfs_read_job, then the refuse mask
REPLY_JOB_DTYPE = np.dtype(_crc.READ_JOB_DTYPE.descr + [("refuse_flags", "<u4"), ("reserved", "<u4")])
assert REPLY_JOB_DTYPE.itemsize == 56
EXPORTED = ["tfs_ec_config", "tfs_ec_free", "tfs_ec_encode_device", "tfs_ec_encode", "tfs_ec_decode_device",
            "tfs_ec_decode", "tfs_ec_read_degraded_device", "tfs_ec_read_degraded", "tfs_ec_read_traffic",
            "tfs_ec_read_reply_device", "tfs_ec_read_reply",
            "tfs_ec_marshal_begin", "tfs_ec_marshal_encode_device", "tfs_ec_marshal_encode", "tfs_ec_marshal_finish",
            "tfs_ec_marshal_free",
            "tfs_ec_reinstate_begin", "tfs_ec_reinstate_decode_device", "tfs_ec_reinstate_decode",
            "tfs_ec_reinstate_finish", "tfs_ec_reinstate_free",
            "tfs_ec_scrub_begin", "tfs_ec_scrub_check_device", "tfs_ec_scrub_check", "tfs_ec_scrub_finish",
            "tfs_ec_scrub_free", "tfs_ec_locate_device", "tfs_ec_locate", "tfs_ec_locate_set_piece",
            "tfs_ec_update_device", "tfs_ec_update", "tfs_ec_update_set_piece",
            "tfs_ec_frames_cap", "tfs_ec_marshal_frames_device", "tfs_ec_marshal_frames",
            "tfs_ec_reinstate_frames_device", "tfs_ec_reinstate_frames",
            "tfs_ec_fetch_cap", "tfs_ec_fetch_expect", "tfs_ec_fetch_parse", "tfs_ec_marshal_task_device",
            "tfs_ec_marshal_task", "tfs_ec_reinstate_task_device", "tfs_ec_reinstate_task"]
MAX_MEMBERS = 12  # TFS_EC_MAX_MEMBERS
# tfs_ec_frames_cfg (include/tfs_ec_frames.h)
FRAMES_CFG_DTYPE = np.dtype([("frame_len", "<i4"), ("frame_stride", "<u4"), ("version", "<i2"), ("reserved", "<i2"),
                             ("block_id", "<u4", (MAX_MEMBERS,)), ("pad", "<u4"), ("packet_id", "<u8", (MAX_MEMBERS,))])
assert FRAMES_CFG_DTYPE.itemsize == 160 and FRAMES_CFG_DTYPE.fields["packet_id"][1] == 64
# tfs_ec_fetch_cfg, tfs_ec_fetch_result (include/tfs_ec_fetch.h)
FETCH_CFG_DTYPE = np.dtype([("in_stride", "<u4"), ("reserved", "<u4")])
FETCH_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n", "<u4"), ("data_file_size", "<i4"), ("crc", "<u4")])
assert FETCH_CFG_DTYPE.itemsize == 8 and FETCH_RESULT_DTYPE.itemsize == 16
FETCH_HEAD, FETCH_OVERHEAD = 28, 32  # TFS_EC_FETCH_HEAD, TFS_EC_FETCH_OVERHEAD
LOCATE_CLEAN, LOCATE_PARITY, LOCATE_DATA, LOCATE_NONE = 0, 1, 2, 3  # TFS_EC_LOCATE_*
LOCATE_CONFIRMED = 1  # TFS_EC_LOCATE_CONFIRMED
LOCATE_RESULT_DTYPE = np.dtype([("kind", "i1"), ("member", "i1"), ("parity", "<u2"), ("diff_bytes", "<u2"),
                                ("flags", "u1"), ("reserved", "u1")])  # tfs_ec_locate_result
assert LOCATE_RESULT_DTYPE.itemsize == 8
_SIG = set()


def lib(L=None):
    """The library of a context (ctx.L: the product, or the measurement build
    for the TFS_EC_VARIANT forms), with the tfs_ec_* signatures set."""
    L = L or _crc.lib()
    if id(L) not in _SIG:
        vp, i32 = ctypes.c_void_p, ctypes.c_int
        for name, res, args in [
                ("tfs_ec_config", i32, [vp, i32, i32, vp, ctypes.POINTER(vp)]),
                ("tfs_ec_free", i32, [vp]),
                ("tfs_ec_encode_device", i32, [vp, vp, vp, i32, vp]),
                ("tfs_ec_encode", i32, [vp, vp, vp, i32]),
                ("tfs_ec_decode_device", i32, [vp, vp, vp, i32, vp]),
                ("tfs_ec_decode", i32, [vp, vp, vp, i32]),
                ("tfs_ec_read_degraded_device", i32,
                 [vp, vp, vp, i32, i32, vp, ctypes.c_uint32, vp, ctypes.c_uint64, vp, vp, vp, vp]),
                ("tfs_ec_read_degraded", i32,
                 [vp, vp, vp, i32, i32, vp, ctypes.c_uint32, vp, ctypes.c_uint64, vp, vp, vp]),
                ("tfs_ec_read_traffic", i32, [vp, vp, vp]),
                ("tfs_ec_read_reply_device", i32,
                 [vp, vp, vp, i32, i32, vp, ctypes.c_uint32, vp, ctypes.c_uint64, vp, vp, vp]),
                ("tfs_ec_read_reply", i32, [vp, vp, vp, i32, i32, vp, ctypes.c_uint32, vp, ctypes.c_uint64, vp, vp]),
                ("tfs_ec_marshal_begin", i32, [vp, vp, vp, vp, i32, ctypes.POINTER(vp)]),
                ("tfs_ec_marshal_encode_device", i32, [vp, vp, i32, i32, vp]),
                ("tfs_ec_marshal_encode", i32, [vp, vp, i32, i32]),
                ("tfs_ec_marshal_finish", i32, [vp, vp, vp, vp]),
                ("tfs_ec_marshal_free", i32, [vp]),
                ("tfs_ec_reinstate_begin", i32, [vp, vp, vp, vp, i32, ctypes.POINTER(vp)]),
                ("tfs_ec_reinstate_decode_device", i32, [vp, vp, i32, i32, vp]),
                ("tfs_ec_reinstate_decode", i32, [vp, vp, i32, i32]),
                ("tfs_ec_reinstate_finish", i32, [vp, vp, vp, vp]),
                ("tfs_ec_reinstate_free", i32, [vp]),
                ("tfs_ec_scrub_begin", i32, [vp, vp, vp, vp, i32, ctypes.POINTER(vp)]),
                ("tfs_ec_scrub_check_device", i32, [vp, vp, i32, i32, vp]),
                ("tfs_ec_scrub_check", i32, [vp, vp, i32, i32]),
                ("tfs_ec_scrub_finish", i32, [vp, vp, vp, vp, vp, vp]),
                ("tfs_ec_scrub_free", i32, [vp]),
                ("tfs_ec_locate_device", i32, [vp, vp, i32, vp, ctypes.c_uint32, vp, vp, vp]),
                ("tfs_ec_locate", i32, [vp, vp, i32, vp, ctypes.c_uint32, vp, vp]),
                ("tfs_ec_locate_set_piece", i32, [vp, ctypes.c_uint32]),
                ("tfs_ec_update_device", i32, [vp, i32, vp, i32, vp, ctypes.c_uint32, vp, vp, vp]),
                ("tfs_ec_update", i32, [vp, i32, vp, i32, vp, ctypes.c_uint32, vp, vp]),
                ("tfs_ec_update_set_piece", i32, [vp, ctypes.c_uint32]),
                ("tfs_ec_frames_cap", ctypes.c_uint64, [vp, i32]),
                ("tfs_ec_marshal_frames_device", i32, [vp, vp, vp, vp, ctypes.c_uint64, i32, i32, vp]),
                ("tfs_ec_marshal_frames", i32, [vp, vp, vp, vp, ctypes.c_uint64, i32, i32]),
                ("tfs_ec_reinstate_frames_device", i32, [vp, vp, vp, vp, ctypes.c_uint64, i32, i32, vp]),
                ("tfs_ec_reinstate_frames", i32, [vp, vp, vp, vp, ctypes.c_uint64, i32, i32]),
                ("tfs_ec_fetch_cap", ctypes.c_uint64, [vp, vp, i32]),
                ("tfs_ec_fetch_expect", ctypes.c_int32, [vp, i32, i32, i32, i32, i32]),
                ("tfs_ec_fetch_parse", i32, [vp, ctypes.c_uint32, vp, vp]),
                ("tfs_ec_marshal_task_device", i32, [vp, vp, vp, vp, vp, ctypes.c_uint64, vp, i32, i32, vp]),
                ("tfs_ec_marshal_task", i32, [vp, vp, vp, vp, vp, ctypes.c_uint64, vp, i32, i32]),
                ("tfs_ec_reinstate_task_device", i32, [vp, vp, vp, vp, vp, ctypes.c_uint64, vp, i32, i32, vp]),
                ("tfs_ec_reinstate_task", i32, [vp, vp, vp, vp, vp, ctypes.c_uint64, vp, i32, i32])]:
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _SIG.add(id(L))
    return L


def frames_cfg(frame_len, block_id=(), packet_id=(), frame_stride=0, version=2, reserved=0):
    """One tfs_ec_frames_cfg as a FRAMES_CFG_DTYPE array of one; block_id / packet_id by member index."""
    c = np.zeros(1, FRAMES_CFG_DTYPE)
    c["frame_len"], c["frame_stride"], c["version"], c["reserved"] = frame_len, frame_stride, version, reserved
    c["block_id"][0, :len(block_id)] = block_id
    c["packet_id"][0, :len(packet_id)] = packet_id
    return c


def frames_cap(cfg, length, L=None):
    """tfs_ec_frames_cap: the bytes one member's out must hold for a call of `length` bytes."""
    c = np.ascontiguousarray(cfg, dtype=FRAMES_CFG_DTYPE).reshape(-1)[:1]
    return int(lib(L).tfs_ec_frames_cap(c.ctypes.data, int(length)))


def _addr(d):
    if d is None or isinstance(d, int):
        return d
    if isinstance(d, np.ndarray):
        return d.ctypes.data
    return d.ptr  # DeviceBuffer, PinnedBuffer


def _frames_call(fn, h, cfg, members, out, out_cap, offset, length, *stream):
    c = None if cfg is None else np.ascontiguousarray(cfg, dtype=FRAMES_CFG_DTYPE).reshape(-1)[:1]
    mp = None if members is None else (ctypes.c_void_p * len(members))(*[_addr(m) for m in members])
    op = None if out is None else (ctypes.c_void_p * len(out))(*[_addr(o) for o in out])
    return fn(h, None if c is None else c.ctypes.data, mp, op, out_cap, offset, length, *stream)


def fetch_cfg(in_stride=0, reserved=0):
    """One tfs_ec_fetch_cfg as a FETCH_CFG_DTYPE array of one."""
    c = np.zeros(1, FETCH_CFG_DTYPE)
    c["in_stride"], c["reserved"] = in_stride, reserved
    return c


def fetch_cap(cfg, fcfg, length, L=None):
    """tfs_ec_fetch_cap: the bytes one member's in must hold for a call of `length` bytes, counted from in[i]."""
    c = None if cfg is None else np.ascontiguousarray(cfg, dtype=FRAMES_CFG_DTYPE).reshape(-1)[:1]
    f = None if fcfg is None else np.ascontiguousarray(fcfg, dtype=FETCH_CFG_DTYPE).reshape(-1)[:1]
    return int(lib(L).tfs_ec_fetch_cap(None if c is None else c.ctypes.data, None if f is None else f.ctypes.data,
                                       int(length)))


def fetch_expect(sizes, dn, total, member, offset, requested, L=None):
    """tfs_ec_fetch_expect: the n the frame at `offset` of `member`, asked for `requested` bytes, must carry."""
    sz = None if sizes is None else np.ascontiguousarray(sizes, dtype=np.int32)
    return int(lib(L).tfs_ec_fetch_expect(None if sz is None else sz.ctypes.data, dn, total, member, offset, requested))


def fetch_parse(frame, L=None):
    """tfs_ec_fetch_parse over host bytes: (rc, n, data_file_size)."""
    b = np.frombuffer(bytes(frame), np.uint8)
    n, dfs = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = lib(L).tfs_ec_fetch_parse(b.ctypes.data if b.size else None, b.size, ctypes.addressof(n), ctypes.addressof(dfs))
    return rc, n.value, dfs.value


def _task_call(fn, h, cfg, fcfg, inp, out, out_cap, results, offset, length, *stream):
    c = None if cfg is None else np.ascontiguousarray(cfg, dtype=FRAMES_CFG_DTYPE).reshape(-1)[:1]
    f = None if fcfg is None else np.ascontiguousarray(fcfg, dtype=FETCH_CFG_DTYPE).reshape(-1)[:1]
    ip = None if inp is None else (ctypes.c_void_p * len(inp))(*[_addr(m) for m in inp])
    op = None if out is None else (ctypes.c_void_p * len(out))(*[_addr(o) for o in out])
    return fn(h, None if c is None else c.ctypes.data, None if f is None else f.ctypes.data, ip, op, out_cap,
              _addr(results), offset, length, *stream)


class ErasureCode:
    """ErasureCode::config + encode/decode.  `rc` holds config's status."""

    def __init__(self, ctx, dn, pn, erased=None):
        self.ctx, self.dn, self.pn = ctx, dn, pn
        h = ctypes.c_void_p()
        e = None if erased is None else (ctypes.c_int * (dn + pn))(*erased)
        self.L = lib(ctx.L)
        self.rc = self.L.tfs_ec_config(ctx.handle, dn, pn, e, ctypes.byref(h))
        self.h = h

    @staticmethod
    def _ptrs(members):
        return (ctypes.c_void_p * len(members))(*[m if isinstance(m, int) or m is None else m.ctypes.data
                                                  for m in members])

    @staticmethod
    def _size(size):
        if not -(1 << 31) <= int(size) < (1 << 31):
            raise ValueError("ErasureCode sizes are C int (erasure_code.h): %d" % size)
        return int(size)

    @staticmethod
    def _sizes(sizes, n):
        return None if sizes is None else (ctypes.c_int * n)(*sizes)

    def encode(self, members, size, sizes=None):
        """Host members (numpy uint8 arrays, written in place for parity)."""
        return self.L.tfs_ec_encode(self.h, self._ptrs(members), self._sizes(sizes, len(members)), self._size(size))

    def decode(self, members, size, sizes=None):
        return self.L.tfs_ec_decode(self.h, self._ptrs(members), self._sizes(sizes, len(members)), self._size(size))

    def encode_device(self, d_members, size, sizes=None, stream=None):
        p = (ctypes.c_void_p * len(d_members))(*[d if isinstance(d, int) or d is None else d.ptr for d in d_members])
        return self.L.tfs_ec_encode_device(self.h, p, self._sizes(sizes, len(d_members)), self._size(size), stream)

    def decode_device(self, d_members, size, sizes=None, stream=None):
        p = (ctypes.c_void_p * len(d_members))(*[d if isinstance(d, int) or d is None else d.ptr for d in d_members])
        return self.L.tfs_ec_decode_device(self.h, p, self._sizes(sizes, len(d_members)), self._size(size), stream)

    @staticmethod
    def read_jobs(metas=None, out_offsets=None, ranges=None):
        """READ_JOB_DTYPE array: record jobs from RawMeta entries (file_id, offset,
        size), or range jobs from (offset, size) pairs.  Without out_offsets the
        covering ranges are packed one after the other; returns (jobs, bytes of out)."""
        if ranges is not None:
            j = np.zeros(len(ranges), READ_JOB_DTYPE)
            j["offset"] = [r[0] for r in ranges]
            j["size"] = [r[1] for r in ranges]
            j["flags"] = READ_RANGE
        else:
            m = np.ascontiguousarray(metas, dtype=_crc.META_DTYPE)
            j = np.zeros(len(m), READ_JOB_DTYPE)
            for f in ("file_id", "offset", "size"):
                j[f] = m[f]
        off, size = j["offset"].astype(np.int64), j["size"].astype(np.int64)
        cover = np.maximum(((off + size + UNIT - 1) // UNIT - off // UNIT) * UNIT, 0)
        if out_offsets is None:
            j["out_offset"] = np.concatenate(([0], np.cumsum(cover)[:-1])) if len(j) else []
            return j, int(cover.sum())
        j["out_offset"] = out_offsets
        return j, int((j["out_offset"].astype(np.int64) + cover).max()) if len(j) else 0

    def read_degraded(self, members, size, target, jobs, out, sizes=None):
        """Host form: rebuild the jobs' covering units of the erased data member
        `target` into `out` (numpy uint8).  Returns (crc, status, n_bad, rc)."""
        j = np.ascontiguousarray(jobs, dtype=READ_JOB_DTYPE)
        n = len(j)
        crc, st, nbad = np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(1, np.uint32)
        rc = self.L.tfs_ec_read_degraded(self.h, self._ptrs(members), self._sizes(sizes, len(members)),
                                         self._size(size), target, j.ctypes.data, n, out.ctypes.data, out.size,
                                         crc.ctypes.data, st.ctypes.data, nbad.ctypes.data)
        return crc, st, int(nbad[0]), rc

    def read_degraded_device(self, d_members, size, target, d_jobs, n, d_out, out_cap, d_crc, d_status, d_nbad=None,
                             sizes=None, stream=None):
        """Device form (asynchronous on `stream`): everything is a DeviceBuffer or a
        device address; erased members may be None."""
        def a(d):
            return d if isinstance(d, int) or d is None else d.ptr
        p = (ctypes.c_void_p * len(d_members))(*[a(d) for d in d_members])
        return self.L.tfs_ec_read_degraded_device(self.h, p, self._sizes(sizes, len(d_members)), self._size(size),
                                                  target, a(d_jobs), n, a(d_out), out_cap, a(d_crc), a(d_status),
                                                  a(d_nbad), stream)

    @staticmethod
    def reply_jobs(read_jobs, refuse_flags=0):
        """REPLY_JOB_DTYPE array from crc.READ_JOB_DTYPE jobs (src_offset: the record's RawMeta.offset in the
        lost member) and the FileInfo.flag_ bits that refuse a first fragment (one value, or one per job)."""
        r = np.ascontiguousarray(read_jobs, dtype=_crc.READ_JOB_DTYPE)
        j = np.zeros(len(r), REPLY_JOB_DTYPE)
        for f in _crc.READ_JOB_DTYPE.names:
            j[f] = r[f]
        j["refuse_flags"] = refuse_flags
        return j

    def read_reply(self, members, size, target, jobs, out, sizes=None):
        """tfs_ec_read_reply, host form: the sealed reply frames of `jobs` (REPLY_JOB_DTYPE) over the erased data
        member `target`, rebuilt from `members` and verified in the same pass, written into `out` (numpy uint8, or
        a PinnedBuffer, which is written in place).  Returns (results, n_bad, rc): results a crc.READ_RESULT_DTYPE
        array; rc is TFS_EXIT_CHECK_CRC_ERROR when any job failed."""
        j = np.ascontiguousarray(jobs, dtype=REPLY_JOB_DTYPE)
        n = len(j)
        res, nbad = np.zeros(n, _crc.READ_RESULT_DTYPE), np.zeros(1, np.uint32)
        o, olen = (out.ctypes.data, out.size) if isinstance(out, np.ndarray) else (out.ptr, out.nbytes)
        rc = self.L.tfs_ec_read_reply(self.h, self._ptrs(members), self._sizes(sizes, len(members)), self._size(size),
                                      target, j.ctypes.data, n, o, olen, res.ctypes.data, nbad.ctypes.data)
        return res, int(nbad[0]), rc

    def read_reply_device(self, d_members, size, target, jobs, d_out, out_cap, d_results, d_nbad=None, sizes=None,
                          stream=None):
        """tfs_ec_read_reply_device, asynchronous on `stream`: members, d_out, d_results (16 bytes a job) and d_nbad
        are DeviceBuffers or device addresses (erased members may be None); `jobs` is a host REPLY_JOB_DTYPE array."""
        def a(d):
            return d if isinstance(d, int) or d is None else d.ptr
        j = np.ascontiguousarray(jobs, dtype=REPLY_JOB_DTYPE)
        p = (ctypes.c_void_p * len(d_members))(*[a(d) for d in d_members])
        return self.L.tfs_ec_read_reply_device(self.h, p, self._sizes(sizes, len(d_members)), self._size(size), target,
                                               j.ctypes.data, len(j), a(d_out), out_cap, a(d_results), a(d_nbad), stream)

    def locate(self, members, size, units=None, want_fixed=True):
        """tfs_ec_locate, host form: which data member is wrong in each listed 1 KiB unit of a
        family whose members (numpy uint8 arrays of `size` bytes, data then parity) are all
        present, and that member's right bytes.  `units`: unit numbers (any order, repeats
        allowed); None: every unit, 0 .. size // 1024 - 1.  Returns (result, fixed, rc): result
        a LOCATE_RESULT_DTYPE array, fixed [n, 1024] uint8 (None unless want_fixed; only the
        rows of LOCATE_DATA results are written, the others stay 0)."""
        if units is None:
            u, n = None, max(int(size), 0) // UNIT
        else:
            u = np.ascontiguousarray(units, dtype=np.uint32)
            n = len(u)
        res = np.zeros(n, LOCATE_RESULT_DTYPE)
        fixed = np.zeros((n, UNIT), np.uint8) if want_fixed else None
        rc = self.L.tfs_ec_locate(self.h, self._ptrs(members), self._size(size), None if u is None else u.ctypes.data, n,
                                  res.ctypes.data, None if fixed is None else fixed.ctypes.data)
        return res, fixed, rc

    def locate_device(self, d_members, size, units, n, d_result, d_fixed=None, stream=None):
        """tfs_ec_locate_device, asynchronous on `stream`: members, d_result (n results) and
        d_fixed (n * 1024 bytes, or None) are DeviceBuffers or device addresses; `units` is a
        host list of n unit numbers, or None for units 0 .. n - 1."""
        def a(d):
            return d if isinstance(d, int) or d is None else d.ptr
        p = (ctypes.c_void_p * len(d_members))(*[a(d) for d in d_members])
        u = None if units is None else np.ascontiguousarray(units, dtype=np.uint32)
        assert u is None or len(u) >= n
        return self.L.tfs_ec_locate_device(self.h, p, self._size(size), None if u is None else u.ctypes.data, n,
                                           a(d_result), a(d_fixed), stream)

    def update(self, parity, size, member, a, b=None, units=None):
        """tfs_ec_update, host form: the in-place change of data member `member` carried into the
        stored parity.  `parity`: pn numpy uint8 arrays of `size` bytes, written in place, or None for
        a parity member the caller does not hold.  `a`, `b`: n * 1024 bytes each, the old and the new
        bytes of the changed units (either order); b None: `a` is the delta old ^ new itself.
        `units`: the n unit numbers (any order, none twice); None: units 0 .. n - 1.  Applied twice,
        an update is undone.  Returns rc."""
        a = np.ascontiguousarray(a, dtype=np.uint8)
        b = None if b is None else np.ascontiguousarray(b, dtype=np.uint8)
        u = None if units is None else np.ascontiguousarray(units, dtype=np.uint32)
        n = a.size // UNIT if u is None else len(u)
        assert a.size >= n * UNIT and (b is None or b.size >= n * UNIT)
        return self.L.tfs_ec_update(self.h, member, self._ptrs(parity), self._size(size), None if u is None else u.ctypes.data,
                                    n, a.ctypes.data, None if b is None else b.ctypes.data)

    def update_device(self, d_parity, size, member, d_a, d_b, units, n, stream=None):
        """tfs_ec_update_device, asynchronous on `stream`: the parity members (None: not bound), d_a and
        d_b (n * 1024 bytes each; d_b may be None) are DeviceBuffers or device addresses; `units` is a
        host list of n unit numbers, or None for units 0 .. n - 1."""
        def a(d):
            return d if isinstance(d, int) or d is None else d.ptr
        p = (ctypes.c_void_p * len(d_parity))(*[a(d) for d in d_parity])
        u = None if units is None else np.ascontiguousarray(units, dtype=np.uint32)
        assert u is None or len(u) >= n
        return self.L.tfs_ec_update_device(self.h, member, p, self._size(size), None if u is None else u.ctypes.data, n,
                                           a(d_a), a(d_b), stream)

    def read_traffic(self):
        """(bytes up, bytes down) of the latest host-form read_degraded or read_reply."""
        up, down = ctypes.c_uint64(), ctypes.c_uint64()
        self.L.tfs_ec_read_traffic(self.h, ctypes.byref(up), ctypes.byref(down))
        return up.value, down.value

    def free(self):
        # after the context is closed its device memory is gone with it: only drop the handle
        if self.h is not None and self.h.value and self.ctx.handle is not None and self.ctx.handle.value:
            self.L.tfs_ec_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MarshalSession:
    """tfs_ec_marshal_*: the parity of a family chunk by chunk, with every record of
    the data members verified from the bytes that feed the code.  `metas[i]` is data
    member i's index (META_DTYPE entries or (file_id, offset, size) tuples), `sizes[i]`
    its block_len, `total` the encode length.  `rc` holds begin's status."""

    def __init__(self, ec, metas, sizes, total):
        self.ec, self.L = ec, ec.L
        self.metas = [np.ascontiguousarray(m, dtype=_crc.META_DTYPE) for m in metas]
        self.n = sum(len(m) for m in self.metas)
        k = len(self.metas)
        mp = (ctypes.c_void_p * max(k, 1))(*[m.ctypes.data if len(m) else None for m in self.metas])
        nm = (ctypes.c_uint32 * max(k, 1))(*[len(m) for m in self.metas])
        h = ctypes.c_void_p()
        self.rc = self.L.tfs_ec_marshal_begin(ec.h, mp, nm, (ctypes.c_int * len(sizes))(*sizes), ErasureCode._size(total),
                                              ctypes.byref(h))
        self.h = h

    def encode(self, members, offset, length):
        """Host form: members[i] is the chunk [offset, offset + length) of member i
        (numpy uint8 arrays; the parity chunks are written)."""
        return self.L.tfs_ec_marshal_encode(self.h, ErasureCode._ptrs(members), offset, length)

    def encode_device(self, d_members, offset, length, stream=None):
        """Device form, asynchronous on `stream`: DeviceBuffers or device addresses of the chunks."""
        p = (ctypes.c_void_p * len(d_members))(*[d if isinstance(d, int) or d is None else d.ptr for d in d_members])
        return self.L.tfs_ec_marshal_encode_device(self.h, p, offset, length, stream)

    def frames(self, cfg, members, out, out_cap, offset, length):
        """tfs_ec_marshal_frames, host form: the chunk's parity as sealed WriteRawDataMessage frames, out[i]
        (numpy uint8 array or PinnedBuffer, by member index; read for the parity members only) receiving member
        i's frames.  `cfg`: frames_cfg()."""
        return _frames_call(self.L.tfs_ec_marshal_frames, self.h, cfg, members, out, out_cap, offset, length)

    def frames_device(self, cfg, d_members, d_out, out_cap, offset, length, stream=None):
        """tfs_ec_marshal_frames_device, asynchronous on `stream`: DeviceBuffers or device addresses."""
        return _frames_call(self.L.tfs_ec_marshal_frames_device, self.h, cfg, d_members, d_out, out_cap, offset, length,
                            stream)

    def task(self, cfg, fcfg, inp, out, out_cap, results, offset, length):
        """tfs_ec_marshal_task, host form: inp[i] holds data member i's RespReadRawDataMessage frames of the chunk
        (numpy uint8 array, PinnedBuffer or address), out[i] receives parity member i's sealed frames, `results` (a
        FETCH_RESULT_DTYPE array, [source][frame of the call]) the verdict on every incoming frame.  `cfg`:
        frames_cfg(); `fcfg`: fetch_cfg()."""
        return _task_call(self.L.tfs_ec_marshal_task, self.h, cfg, fcfg, inp, out, out_cap, results, offset, length)

    def task_device(self, cfg, fcfg, d_in, d_out, out_cap, d_results, offset, length, stream=None):
        """tfs_ec_marshal_task_device, asynchronous on `stream`: DeviceBuffers or device addresses."""
        return _task_call(self.L.tfs_ec_marshal_task_device, self.h, cfg, fcfg, d_in, d_out, out_cap, d_results, offset,
                          length, stream)

    def finish(self):
        """(crc, status, n_bad, rc): member 0's records, then member 1's, and so on."""
        crc, st, nbad = np.zeros(self.n, np.uint32), np.zeros(self.n, np.int32), np.zeros(1, np.uint32)
        rc = self.L.tfs_ec_marshal_finish(self.h, crc.ctypes.data, st.ctypes.data, nbad.ctypes.data)
        return crc, st, int(nbad[0]), rc

    def free(self):
        if self.h is not None and self.h.value and self.ec.h is not None and self.ec.ctx.handle is not None and \
                self.ec.ctx.handle.value:
            self.L.tfs_ec_marshal_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ReinstateSession:
    """tfs_ec_reinstate_*: the dead members of a family rebuilt chunk by chunk over the
    coder's decode plan (`ec` is configured with `erased`), with every record of every
    data member verified in the same pass -- the surviving ones from the bytes that feed
    the code, the rebuilt ones from the bytes it yields.  `metas[i]` is data member i's
    index (for a dead member the one a parity block keeps; none for an unused member),
    `sizes[i]` its block_len (a dead member's: the length its records are checked
    against), `total` the decode length.  `rc` holds begin's status."""

    def __init__(self, ec, metas, sizes, total):
        self.ec, self.L = ec, ec.L
        self.metas = [np.ascontiguousarray(m, dtype=_crc.META_DTYPE) for m in metas]
        self.n = sum(len(m) for m in self.metas)
        k = len(self.metas)
        mp = (ctypes.c_void_p * max(k, 1))(*[m.ctypes.data if len(m) else None for m in self.metas])
        nm = (ctypes.c_uint32 * max(k, 1))(*[len(m) for m in self.metas])
        h = ctypes.c_void_p()
        self.rc = self.L.tfs_ec_reinstate_begin(ec.h, mp, nm, (ctypes.c_int * len(sizes))(*sizes),
                                                ErasureCode._size(total), ctypes.byref(h))
        self.h = h

    def decode(self, members, offset, length):
        """Host form: members[i] is the chunk [offset, offset + length) of member i (numpy
        uint8 arrays; the chunks of the plan's outputs are written).  Members the plan
        neither reads nor rebuilds may be None."""
        return self.L.tfs_ec_reinstate_decode(self.h, ErasureCode._ptrs(members), offset, length)

    def decode_device(self, d_members, offset, length, stream=None):
        """Device form, asynchronous on `stream`: DeviceBuffers or device addresses of the chunks."""
        p = (ctypes.c_void_p * len(d_members))(*[d if isinstance(d, int) or d is None else d.ptr for d in d_members])
        return self.L.tfs_ec_reinstate_decode_device(self.h, p, offset, length, stream)

    def frames(self, cfg, members, out, out_cap, offset, length):
        """tfs_ec_reinstate_frames, host form: the chunk's rebuilt pieces as sealed WriteRawDataMessage frames,
        out[i] (numpy uint8 array or PinnedBuffer, by member index; read for the dead members only) receiving
        member i's frames.  `cfg`: frames_cfg()."""
        return _frames_call(self.L.tfs_ec_reinstate_frames, self.h, cfg, members, out, out_cap, offset, length)

    def frames_device(self, cfg, d_members, d_out, out_cap, offset, length, stream=None):
        """tfs_ec_reinstate_frames_device, asynchronous on `stream`: DeviceBuffers or device addresses."""
        return _frames_call(self.L.tfs_ec_reinstate_frames_device, self.h, cfg, d_members, d_out, out_cap, offset,
                            length, stream)

    def task(self, cfg, fcfg, inp, out, out_cap, results, offset, length):
        """tfs_ec_reinstate_task, host form: inp[i] holds survivor i's RespReadRawDataMessage frames of the chunk,
        out[i] receives dead member i's sealed frames, `results` (FETCH_RESULT_DTYPE, [source in the decode plan's
        order][frame of the call]) the verdict on every incoming frame."""
        return _task_call(self.L.tfs_ec_reinstate_task, self.h, cfg, fcfg, inp, out, out_cap, results, offset, length)

    def task_device(self, cfg, fcfg, d_in, d_out, out_cap, d_results, offset, length, stream=None):
        """tfs_ec_reinstate_task_device, asynchronous on `stream`: DeviceBuffers or device addresses."""
        return _task_call(self.L.tfs_ec_reinstate_task_device, self.h, cfg, fcfg, d_in, d_out, out_cap, d_results,
                          offset, length, stream)

    def finish(self):
        """(crc, status, n_bad, rc): data member 0's records, then member 1's, and so on."""
        crc, st, nbad = np.zeros(self.n, np.uint32), np.zeros(self.n, np.int32), np.zeros(1, np.uint32)
        rc = self.L.tfs_ec_reinstate_finish(self.h, crc.ctypes.data, st.ctypes.data, nbad.ctypes.data)
        return crc, st, int(nbad[0]), rc

    def free(self):
        if self.h is not None and self.h.value and self.ec.h is not None and self.ec.ctx.handle is not None and \
                self.ec.ctx.handle.value:
            self.L.tfs_ec_reinstate_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class ScrubSession:
    """tfs_ec_scrub_*: the stored parity of a family compared chunk by chunk with the code
    of its data members as read, with every record of the data members verified in the
    same pass; no member is written.  `metas[i]` is data member i's index, `sizes[i]` its
    block_len, `total` the encode length, as for MarshalSession.  `rc` holds begin's status."""

    def __init__(self, ec, metas, sizes, total):
        self.ec, self.L = ec, ec.L
        self.metas = [np.ascontiguousarray(m, dtype=_crc.META_DTYPE) for m in metas]
        self.n = sum(len(m) for m in self.metas)
        self.ntiles = max((int(total) + 4095) // 4096, 0)
        k = len(self.metas)
        mp = (ctypes.c_void_p * max(k, 1))(*[m.ctypes.data if len(m) else None for m in self.metas])
        nm = (ctypes.c_uint32 * max(k, 1))(*[len(m) for m in self.metas])
        h = ctypes.c_void_p()
        self.rc = self.L.tfs_ec_scrub_begin(ec.h, mp, nm, (ctypes.c_int * len(sizes))(*sizes), ErasureCode._size(total),
                                            ctypes.byref(h))
        self.h = h

    def check(self, members, offset, length):
        """Host form: members[i] is the chunk [offset, offset + length) of member i (numpy
        uint8 arrays, data and parity; none is written)."""
        return self.L.tfs_ec_scrub_check(self.h, ErasureCode._ptrs(members), offset, length)

    def check_device(self, d_members, offset, length, stream=None):
        """Device form, asynchronous on `stream`: DeviceBuffers or device addresses of the chunks."""
        p = (ctypes.c_void_p * len(d_members))(*[d if isinstance(d, int) or d is None else d.ptr for d in d_members])
        return self.L.tfs_ec_scrub_check_device(self.h, p, offset, length, stream)

    def finish(self):
        """(crc, status, n_bad, parity_units, tile_map, rc): the records as MarshalSession.finish
        has them; parity_units[p] the differing 1 KiB units of parity member p; tile_map[p][T]
        the four unit bits of tile T."""
        crc, st, nbad = np.zeros(self.n, np.uint32), np.zeros(self.n, np.int32), np.zeros(1, np.uint32)
        units = np.zeros(self.ec.pn, np.uint32)
        tmap = np.zeros((self.ec.pn, self.ntiles), np.uint8)
        rc = self.L.tfs_ec_scrub_finish(self.h, crc.ctypes.data, st.ctypes.data, nbad.ctypes.data, units.ctypes.data,
                                        tmap.ctypes.data)
        return crc, st, int(nbad[0]), units, tmap, rc

    def free(self):
        if self.h is not None and self.h.value and self.ec.h is not None and self.ec.ctx.handle is not None and \
                self.ec.ctx.handle.value:
            self.L.tfs_ec_scrub_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
