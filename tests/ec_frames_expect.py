"""Expected bytes of the erasure-code tasks' WriteRawDataMessage frames
(include/tfs_ec_frames.h), built from the oracles alone: the member's bytes come from
jerasure (oracle_ec_encode / oracle_ec_decode through the callers), each frame's header CRC
from oracle_crc over the whole body H || D || F with the seed TFS_PACKET_FLAG_V1.
Shared by the frame tests of the marshalling and reinstate sessions and of the
dataserver layer."""
import struct

import numpy as np

from conftest import ocrc

FLAG_V1 = 0x4E534654
PCODE = 35  # WRITE_RAW_DATA_MESSAGE
NORMAL, PARITY = 1, 2
HEAD, OVERHEAD = 56, 60
PREFILL = 0x5C


def frame_bytes(oracle, data, block_id, offset, pid, flag, version=2):
    """One sealed frame around `data` (bytes [offset, offset + len(data)) of the member)."""
    body = struct.pack("<IQIIIQ", block_id, 0, offset, len(data), 0, 0) + bytes(data) + struct.pack("<I", flag)
    crc = ocrc(oracle, FLAG_V1, body) if version >= 1 else 0
    return struct.pack("<IIhhQI", FLAG_V1, len(body), PCODE, version, pid & 0xFFFFFFFFFFFFFFFF, crc) + body


def member_frames(oracle, member, frame_len, block_id, packet_id, parity, version=2):
    """Every frame of one output member (numpy uint8, `total` bytes), in order."""
    out = []
    for k, off in enumerate(range(0, member.size, frame_len)):
        d = member[off:off + frame_len].tobytes()
        out.append(frame_bytes(oracle, d, block_id, off, packet_id + k, (PARITY if parity else NORMAL) if k == 0 else 0,
                               version))
    return out


def stride_of(frame_len, frame_stride=0):
    return frame_stride or frame_len + 64


def call_image(frames, k0, nf, stride, cap, prefill=PREFILL):
    """What one member's out holds after a call that made frames [k0, k0 + nf): frame j at j * stride, every
    other byte of the `cap` bytes at its prefill value."""
    img = np.full(cap, prefill, np.uint8)
    for j in range(nf):
        f = np.frombuffer(frames[k0 + j], np.uint8)
        img[j * stride:j * stride + f.size] = f
    return img


def need(frame_len, length, frame_stride=0):
    nf = (length + frame_len - 1) // frame_len
    return (nf - 1) * stride_of(frame_len, frame_stride) + OVERHEAD + length - (nf - 1) * frame_len


def data_of(image, frame_len, length, stride):
    """The D areas of a call's frames, joined."""
    nf = (length + frame_len - 1) // frame_len
    return np.concatenate([image[j * stride + HEAD:j * stride + HEAD + min(frame_len, length - j * frame_len)]
                           for j in range(nf)])
