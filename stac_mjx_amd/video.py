"""Video output of ``Stac.render``: an MJPEG-in-RIFF ``.avi`` writer (PIL JPEG frames), other formats through imageio.

``imageio`` (what the reference writes with, ``stac.py:645``) is optional here.  ``.avi`` is always written by
:func:`write_avi`; another suffix goes through ``imageio`` when it imports, else an ``.avi`` stand-in is written next to it
(like the ``.h5`` -> ``.npz`` stand-in of ``io.save_data_to_h5``) and the substitution is logged.
"""

from __future__ import annotations

import io as _io
import struct
from pathlib import Path

import numpy as np

RIFF_LIMIT = (1 << 32) - 1  # a RIFF chunk size is 32 bits; larger files would need OpenDML (not supported)
JPEG_QUALITY = 90


def _jpeg(frame: np.ndarray) -> bytes:
    from PIL import Image

    buf = _io.BytesIO()
    Image.fromarray(np.ascontiguousarray(frame, dtype=np.uint8), "RGB").save(buf, format="JPEG", quality=JPEG_QUALITY)
    return buf.getvalue()


def encode_jpegs(frames) -> list[bytes]:
    """JPEG bytes of every frame, encoded on the io thread pool (PIL releases the GIL while it encodes)."""
    from .io import _pool

    frames = list(frames)
    if len(frames) <= 1:
        return [_jpeg(f) for f in frames]
    with _pool() as pool:
        return list(pool.map(_jpeg, frames))


def _chunk(fourcc: bytes, data: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")


def _list(kind: bytes, data: bytes) -> bytes:
    return b"LIST" + struct.pack("<I", len(data) + 4) + kind + data


def write_avi(path, frames, fps: float, jpegs=None, size=None) -> Path:
    """Write ``frames`` ([H, W, 3] uint8 each) as an MJPEG AVI at ``fps``.  ``jpegs``: already encoded frames; with
    ``size=(width, height)`` they are all it needs and ``frames`` may be None."""
    path = Path(path)
    frames = list(frames) if frames is not None else []
    if size is not None and jpegs is not None:
        W, H = int(size[0]), int(size[1])
        jpegs = list(jpegs)
        if not jpegs:
            raise ValueError("write_avi: no frames")
    else:
        if not frames:
            raise ValueError("write_avi: no frames")
        H, W = frames[0].shape[:2]
        jpegs = encode_jpegs(frames) if jpegs is None else jpegs
    n = len(jpegs)
    us = int(round(1e6 / float(fps)))
    biggest = max(len(j) for j in jpegs)
    avih = struct.pack("<IIIIIIIIIIIIII", us, int(biggest * float(fps)), 0, 0x10, n, 0, 1, biggest, W, H, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", b"MJPG", 0, 0, 0, 0, 1000, int(round(float(fps) * 1000)), 0, n,
                       biggest, 0xFFFFFFFF, 0, 0, 0, W, H)
    strf = struct.pack("<IiiHH4sIiiII", 40, W, H, 1, 24, b"MJPG", W * H * 3, 0, 0, 0, 0)
    hdrl = _list(b"hdrl", _chunk(b"avih", avih) + _list(b"strl", _chunk(b"strh", strh) + _chunk(b"strf", strf)))
    movi_parts, index, off = [], [], 4  # offsets are relative to the 'movi' fourcc
    for j in jpegs:
        c = _chunk(b"00dc", j)
        index.append(struct.pack("<4sIII", b"00dc", 0x10, off, len(j)))
        movi_parts.append(c)
        off += len(c)
    movi = _list(b"movi", b"".join(movi_parts))
    idx1 = _chunk(b"idx1", b"".join(index))
    body = b"AVI " + hdrl + movi + idx1
    if len(body) > RIFF_LIMIT:
        raise ValueError(f"write_avi: {len(body)} bytes exceed the RIFF size limit ({RIFF_LIMIT}); write fewer frames per file")
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return path


def read_avi(path) -> dict:
    """Parse an AVI written by :func:`write_avi`: {"width", "height", "fps", "frames": [jpeg bytes], "index": [(offset, size)]}."""
    data = Path(path).read_bytes()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError("not an AVI file")
    out = {"frames": [], "index": []}
    pos, movi_at = 12, None
    while pos < len(data):
        fourcc, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        if fourcc == b"LIST":
            kind = data[pos + 8:pos + 12]
            if kind == b"hdrl":
                avih = data[pos + 20:pos + 20 + 56]
                us, _, _, _, n, _, _, _, W, H = struct.unpack("<10I", avih[:40])
                out.update(width=W, height=H, n_frames=n, us_per_frame=us)
                strh_at = data.index(b"strh", pos)
                sh = struct.unpack("<4s4sIHHIIII", data[strh_at + 8:strh_at + 8 + 32])
                out["fps"] = sh[7] / sh[6]
            elif kind == b"movi":
                movi_at = pos + 8
                p = pos + 12
                while p < pos + 8 + size:
                    cc, sz = data[p:p + 4], struct.unpack("<I", data[p + 4:p + 8])[0]
                    if cc == b"00dc":
                        out["frames"].append(data[p + 8:p + 8 + sz])
                    p += 8 + sz + (sz & 1)
            pos += 8 + size + (size & 1)
        else:
            if fourcc == b"idx1":
                for k in range(size // 16):
                    cc, fl, off, sz = struct.unpack("<4sIII", data[pos + 8 + 16 * k:pos + 24 + 16 * k])
                    out["index"].append((off, sz))
                    assert data[movi_at + off:movi_at + off + 4] == cc
            pos += 8 + size + (size & 1)
    return out


def write_video(save_path, frames, fps: float, log=print) -> Path:
    """``.avi``: :func:`write_avi`.  Other suffixes: imageio when it imports (the reference's writer), else an ``.avi``
    stand-in next to ``save_path``.  Returns the path written."""
    save_path = Path(save_path)
    if save_path.suffix.lower() != ".avi":
        try:
            import imageio
        except ImportError:
            out = save_path.with_suffix(".avi")
            log(f"imageio is not installed: writing {out} (MJPEG AVI) instead of {save_path}")
            return write_avi(out, frames, fps)
        with imageio.get_writer(save_path, fps=fps) as video:
            for f in frames:
                video.append_data(f)
        return save_path
    return write_avi(save_path, frames, fps)
