"""JPEG encoding of frames on the GPU: ``encode_jpegs_gpu`` over ``stac_jpeg_encode`` (csrc/stac_jpeg.hip).

The bytes are those of libjpeg (hence of ``PIL.Image.save(format="JPEG", quality=q, restart_marker_blocks=R)``) for the same
pixels: DESIGN.md "JPEG on the GPU".  Only the compressed stream crosses to the host.
"""

from __future__ import annotations

import ctypes as C

import torch

from .abi import _ptr, check, stream_ptr
from .abi import declare as bind  # noqa: F401  (the name callers of the raw library know: the whole table, idempotent)
from .engine import load_library
from .video import JPEG_QUALITY

HEADER_MAX = 640  # csrc/stac_jpeg.hpp: kJpegHeaderMax
FIRST_GUESS = 0.25  # the output buffer of a first attempt, as a fraction of the raw frames (rendered frames need about 0.01)


def default_restart_mcus(width: int) -> int:
    """One MCU row: a restart marker at the end of every 16 pixel rows."""
    return max(1, (int(width) + 15) // 16)


def jpeg_header(width: int, height: int, quality: int = JPEG_QUALITY, restart_mcus: int = 0) -> bytes:
    """SOI .. SOS of the file that the encoder writes for these settings (host only; ``restart_mcus=0``: no DRI segment)."""
    lib = load_library()
    buf = (C.c_uint8 * HEADER_MAX)()
    n = check(lib, "stac_jpeg_header", lib.stac_jpeg_header(int(width), int(height), int(quality), int(restart_mcus), buf, HEADER_MAX))
    return bytes(buf[:n])


def workspace_bytes(n: int, width: int, height: int, restart_mcus: int) -> int:
    lib = load_library()
    return int(check(lib, "stac_jpeg_workspace_bytes", lib.stac_jpeg_workspace_bytes(int(n), int(width), int(height), int(restart_mcus))))


def encode_raw(rgb: torch.Tensor, out: torch.Tensor, frame_offset: torch.Tensor, workspace: torch.Tensor, quality: int,
               restart_mcus: int, out_capacity: int | None = None):
    """One ``stac_jpeg_encode`` on the current stream of ``rgb``'s device; every tensor is the caller's."""
    lib = load_library()
    N, H, W, _ = rgb.shape
    cap = out.numel() if out_capacity is None else int(out_capacity)
    with torch.cuda.device(rgb.device):
        rc = lib.stac_jpeg_encode(N, W, H, int(quality), int(restart_mcus), _ptr(rgb), _ptr(out), cap, _ptr(frame_offset),
                                  _ptr(workspace), workspace.numel() * workspace.element_size(), stream_ptr(rgb.device))
    check(lib, "stac_jpeg_encode", rc)


class JpegEncoder:
    """Workspace and output buffer for frames of one size, reused from call to call (at most ``max_frames`` per call)."""

    def __init__(self, max_frames: int, width: int, height: int, quality: int = JPEG_QUALITY, restart_mcus: int | None = None,
                 device=None, out_bytes: int | None = None):
        self.max_frames, self.W, self.H, self.quality = int(max_frames), int(width), int(height), int(quality)
        self.R = default_restart_mcus(width) if restart_mcus is None else int(restart_mcus)
        if not 1 <= self.quality <= 100:
            raise ValueError(f"JPEG quality {quality} outside 1..100")
        if not 1 <= self.R <= 65535:
            raise ValueError(f"restart_mcus {restart_mcus} outside 1..65535")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        need = workspace_bytes(self.max_frames, self.W, self.H, self.R)
        self.workspace = torch.empty(max(need, 8) // 8 + 1, dtype=torch.int64, device=self.device)
        self.frame_offset = torch.empty(self.max_frames + 1, dtype=torch.int64, device=self.device)
        if out_bytes is None:
            out_bytes = self.first_guess(self.max_frames, self.W, self.H)
        self.out = torch.empty(int(out_bytes), dtype=torch.uint8, device=self.device)

    @staticmethod
    def first_guess(n: int, width: int, height: int) -> int:
        return int(n * (HEADER_MAX + 2) + FIRST_GUESS * n * width * height * 3) + 1024

    def encode(self, rgb: torch.Tensor) -> list[bytes]:
        if rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[3] != 3 or tuple(rgb.shape[1:3]) != (self.H, self.W):
            raise ValueError(f"rgb must be uint8 [N, {self.H}, {self.W}, 3], got {rgb.dtype} {tuple(rgb.shape)}")
        if rgb.device != self.device:
            raise ValueError(f"rgb is on {rgb.device}, the encoder on {self.device}")
        N = rgb.shape[0]
        if N > self.max_frames:
            raise ValueError(f"{N} frames for an encoder of {self.max_frames}")
        if N == 0:
            return []
        rgb = rgb.contiguous()
        while True:
            encode_raw(rgb, self.out, self.frame_offset, self.workspace, self.quality, self.R)
            off = self.frame_offset[: N + 1].cpu().tolist()  # waits for the call
            if off[N] <= self.out.numel():
                break
            self.out = torch.empty(off[N] + off[N] // 8, dtype=torch.uint8, device=self.device)  # true size known: one repeat
        data = self.out[: off[N]].cpu().numpy().tobytes()
        return [data[off[k]:off[k + 1]] for k in range(N)]


def encode_jpegs_gpu(rgb: torch.Tensor, quality: int = JPEG_QUALITY, restart_mcus: int | None = None) -> list[bytes]:
    """JPEG files of the frames ``rgb`` (CUDA uint8 [N, H, W, 3]), encoded on its device.  ``restart_mcus``: restart interval
    in MCUs of 16 x 16 pixels, 1..65535 (None: one MCU row).  The output buffer starts at a fraction of the raw size and the
    call is repeated when it was too small; only the frame offsets and the used bytes are copied to the host."""
    if not isinstance(rgb, torch.Tensor) or not rgb.is_cuda:
        raise ValueError("encode_jpegs_gpu needs a CUDA tensor (the PIL path is stac_mjx_amd.video.encode_jpegs)")
    if rgb.dim() != 4 or rgb.shape[3] != 3 or rgb.dtype != torch.uint8:
        raise ValueError(f"rgb must be uint8 [N, H, W, 3], got {rgb.dtype} {tuple(rgb.shape)}")
    N, H, W, _ = rgb.shape
    if N == 0:
        return []
    return JpegEncoder(N, W, H, quality, restart_mcus, rgb.device).encode(rgb)
