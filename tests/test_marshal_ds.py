"""MarshallingTask::do_marshalling through the dataserver harness (tfs_amd/dataserver.py
do_marshalling over tfs_ec_marshal_*): a family of real LogicBlock images is
marshalled in small chunks, the parity it wrote serves a degraded read of every
file of an erased member, and a source record that was corrupt before the
marshalling is named."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, ocrc
from tfs_amd.synth import synth_bytes

pytestmark = pytest.mark.gpu

FI = 36
CRC_ERR = -1010
K, M = 3, 2


def build_blocks(oracle):
    from tfs_amd.dataserver import LogicBlock
    blocks = []
    for i, lens in enumerate([(30000, 5, 70000, 1000, 12345, 100, 2000), (50001, 4095, 4096, 9), (777,) * 40 + (20000,)]):
        b = LogicBlock(300 + i)
        for fid, n in enumerate(lens, 1):
            p = synth_bytes(5000 * i + fid, n).tobytes()
            assert b.append(fid, p, ocrc(oracle, 0, p)) == 0
        blocks.append(b)
    return blocks


def sorted_index(b):
    m = b.metas()[0]
    return m[np.argsort(m["offset"], kind="stable")]


@pytest.mark.parametrize("chunk", [4096, 8192, 1 << 20])
def test_do_marshalling_then_degraded_read(gpu_ctx, oracle, chunk):
    import tfs_amd.dataserver as ds
    blocks = build_blocks(oracle)
    raws = [b.raw() for b in blocks]
    idx = [sorted_index(b) for b in blocks]
    total = (max(r.size for r in raws) + 1023) // 1024 * 1024
    assert len({r.size for r in raws}) == 3
    parity = [np.full(total, 0xA5, np.uint8) for _ in range(M)]
    ids = [300, 301, 302, 400, 401]
    rc, st, tot = ds.do_marshalling(gpu_ctx, ds.Family(K, M, ids, raws + parity), idx, chunk_len=chunk)
    assert rc == 0 and tot == total and [len(s) for s in st] == [len(m) for m in idx]
    assert all((s == 0).all() for s in st)
    # the parity is jerasure's code of the zero-extended members
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "liboracle_ec.so"))
    L.oracle_ec_encode.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    ms = []
    for r in raws:
        a = np.zeros(total, np.uint8)
        a[:r.size] = r
        ms.append(a)
    ms += [np.zeros(total, np.uint8) for _ in range(M)]
    assert L.oracle_ec_encode(K, M, (ctypes.c_void_p * (K + M))(*[a.ctypes.data for a in ms]), None, total) == 0
    assert all((parity[i] == ms[K + i]).all() for i in range(M))
    # one member erased: every file of it is served from the family
    lost = 0
    fam = ds.Family(K, M, ids, [None if i == lost else raws[i] for i in range(K)] + parity)
    fids = [int(x) for x in idx[lost]["file_id"]]
    rc, files, rst = ds.read_files_degrade(gpu_ctx, fam, 300 + lost, fids, idx[lost])
    assert rc == 0 and (rst == 0).all()
    for x, f in zip(idx[lost], files):
        assert f == raws[lost][int(x["offset"]):int(x["offset"]) + int(x["size"])].tobytes()


def test_do_marshalling_names_the_corrupt_record(gpu_ctx, oracle):
    import tfs_amd.dataserver as ds
    blocks = build_blocks(oracle)
    idx = [sorted_index(b) for b in blocks]
    victim = 2                                                  # the 70,000-byte file of member 0
    blocks[0].corrupt(int(idx[0][victim]["offset"]) + FI + 33333, 0x20)
    raws = [b.raw() for b in blocks]
    total = (max(r.size for r in raws) + 1023) // 1024 * 1024
    parity = [np.zeros(total, np.uint8) for _ in range(M)]
    rc, st, _ = ds.do_marshalling(gpu_ctx, ds.Family(K, M, [300, 301, 302, 400, 401], raws + parity), idx, chunk_len=8192)
    assert rc == 1
    assert st[0][victim] == CRC_ERR and int((st[0] != 0).sum()) == 1 and (st[1] == 0).all() and (st[2] == 0).all()
    # call-level: a chunk length that is no multiple of 4096, an index that is not sorted
    assert ds.do_marshalling(gpu_ctx, ds.Family(K, M, [300, 301, 302, 400, 401], raws + parity), idx, chunk_len=1024)[0] \
        == -1016
    assert ds.do_marshalling(gpu_ctx, ds.Family(K, M, [300, 301, 302, 400, 401], raws + parity),
                             [idx[0][::-1].copy(), idx[1], idx[2]], chunk_len=8192)[0] == -1016
