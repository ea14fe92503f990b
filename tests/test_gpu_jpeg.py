"""The GPU JPEG encoder (csrc/stac_jpeg.hip) against Pillow's bytes, at tolerance 0: small images of every edge shape at three
qualities and five restart intervals, batches of frames of unequal length, a scan whose size prefix sum spans several workgroups,
the capacity contract of stac_jpeg_encode, stale workspace / other stream / odd byte offset, and Stac.render(encoder="gpu") end
to end.  tests/test_jpeg_host.py shows (without a GPU) that tests/jpeg_ref.py states the same rule as Pillow."""

import numpy as np
import pytest
import torch

import jpeg_ref

pytestmark = pytest.mark.gpu

IMAGES = jpeg_ref.images()
QUALITIES = (35, 90, 100)
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def libjpeg_is_the_one_the_rule_was_written_for():
    """A different libjpeg build behind Pillow on this machine must show up as that, not as a kernel error."""
    img = IMAGES["tiny5x3"]
    assert jpeg_ref.encode(img, 90, 1) == jpeg_ref.pillow(img, 90, 1), "tests/jpeg_ref.py != Pillow: another libjpeg build?"


def restart_cases(W, H):
    mw, mh = (W + 15) // 16, (H + 15) // 16
    return (1, 3, 8, mw, mw * mh + 5)  # ..., one MCU row, more than all MCUs (DRI present, no marker)


def gpu(frames, q, R):
    from stac_mjx_amd.jpeg import encode_jpegs_gpu

    return encode_jpegs_gpu(torch.as_tensor(np.ascontiguousarray(frames)).to(DEV), q, R)


def first_difference(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))
    return f"lengths {len(a)} / {len(b)}, first difference at byte {int(d[0]) if len(d) else n}"


def assert_files(got, frames, q, R, what):
    assert len(got) == len(frames), what
    for k, f in enumerate(frames):
        want = jpeg_ref.pillow(f, q, R)
        assert got[k] == want, f"{what} frame {k} q={q} R={R}: {first_difference(got[k], want)}"


@pytest.mark.parametrize("name", list(IMAGES))
def test_small_parity(name):
    img = IMAGES[name]
    H, W = img.shape[:2]
    for q in QUALITIES:
        for R in restart_cases(W, H):
            assert_files(gpu(img[None], q, R), [img], q, R, name)


@pytest.mark.parametrize("W,H", [(97, 61), (50, 40), (100, 36)])
def test_batch_of_unequal_frames(W, H):
    rng = np.random.default_rng(W)
    yy, xx = np.mgrid[0:H, 0:W]
    frames = np.stack([rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
                       np.stack([(xx * 3) % 256, (yy * 5) % 256, (xx + 2 * yy) % 256], -1).astype(np.uint8),
                       np.full((H, W, 3), 31, np.uint8)])
    for q in QUALITIES:
        for R in restart_cases(W, H):
            got = gpu(frames, q, R)
            assert len({len(g) for g in got}) == 3
            assert_files(got, frames, q, R, f"batch {W}x{H}")


def test_default_restart_interval_is_one_mcu_row():
    from stac_mjx_amd.jpeg import default_restart_mcus, encode_jpegs_gpu
    from stac_mjx_amd.video import JPEG_QUALITY

    img = IMAGES["smooth130x90"]
    assert default_restart_mcus(130) == 9
    assert_files(encode_jpegs_gpu(torch.as_tensor(img[None]).to(DEV)), [img], JPEG_QUALITY, 9, "defaults")
    assert encode_jpegs_gpu(torch.empty((0, 8, 8, 3), dtype=torch.uint8, device=DEV)) == []


def test_large_scan():
    """1089 intervals per frame, 5445 in the call: the size prefix sum spans six workgroups."""
    frames = np.random.default_rng(7).integers(0, 256, (5, 528, 528, 3), dtype=np.uint8)
    frames[3, :, :264] = 128  # frames of unequal length
    assert_files(gpu(frames, 90, 1), frames, 90, 1, "528x528")


def raw_call(frames, q, R, cap, fill=None, stream=None, rgb=None):
    """One stac_jpeg_encode with `cap` bytes of output in front of 64 guard bytes -> (out bytes, guard, frame offsets)."""
    from stac_mjx_amd import jpeg

    N, H, W, _ = frames.shape
    rgb = torch.as_tensor(np.ascontiguousarray(frames)).to(DEV) if rgb is None else rgb
    ws = torch.empty(jpeg.workspace_bytes(N, W, H, R) // 8 + 1, dtype=torch.int64, device=DEV)
    out = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    off = torch.full((N + 1,), -7, dtype=torch.int64, device=DEV)
    if fill is not None:
        ws.view(torch.uint8).fill_(fill)
        out[:cap].fill_(fill)
    if stream is None:
        jpeg.encode_raw(rgb, out, off, ws, q, R, out_capacity=cap)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            jpeg.encode_raw(rgb, out, off, ws, q, R, out_capacity=cap)
        stream.synchronize()
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return o[:cap].tobytes(), o[cap:], off.cpu().tolist()


@pytest.fixture(scope="module")
def three_frames():
    rng = np.random.default_rng(3)
    frames = np.stack([rng.integers(0, 256, (61, 97, 3), dtype=np.uint8), IMAGES["noise97x61"], np.full((61, 97, 3), 200, np.uint8)])
    want = [jpeg_ref.pillow(f, 100, 3) for f in frames]
    return frames, want, b"".join(want), list(np.cumsum([0] + [len(w) for w in want]))


def test_capacity_contract(three_frames):
    frames, want, whole, offsets = three_frames
    need = len(whole)
    for cap in (0, 1, 700, need // 2, offsets[1], offsets[2] + 1, need - 1, need):
        data, guard, off = raw_call(frames, 100, 3, cap)
        assert (guard == 0xA5).all(), f"capacity {cap}: bytes written beyond it"
        assert off == offsets, f"capacity {cap}: frame_offset must hold the true sizes"
        assert data == whole[:cap], f"capacity {cap}: {first_difference(data, whole[:cap])}"
    data, guard, off = raw_call(frames, 100, 3, need + 1000)
    assert data[:need] == whole and off == offsets and (guard == 0xA5).all()
    assert set(data[need:]) == {0xA5}


def test_small_first_buffer_is_repeated(three_frames):
    from stac_mjx_amd.jpeg import JpegEncoder

    frames, want, _, _ = three_frames
    enc = JpegEncoder(3, 97, 61, 100, 3, DEV, out_bytes=1000)
    rgb = torch.as_tensor(frames).to(DEV)
    assert enc.encode(rgb) == want and enc.out.numel() >= sum(len(w) for w in want)
    assert enc.encode(rgb[:2]) == want[:2]  # and the buffers serve the next call


def test_stale_state_stream_and_alignment(three_frames):
    frames, want, whole, offsets = three_frames
    cap = len(whole) + 16
    for fill in (0xFF, 0x00, 0x5A):
        data, _, off = raw_call(frames, 100, 3, cap, fill=fill)
        assert data[:len(whole)] == whole and off == offsets, f"workspace and output pre-filled with {fill:#x}"
    data, _, off = raw_call(frames, 100, 3, cap, fill=0xFF, stream=torch.cuda.Stream(device=DEV))
    assert data[:len(whole)] == whole and off == offsets, "non-default stream"
    flat = torch.zeros(frames.size + 8, dtype=torch.uint8, device=DEV)
    for start in (1, 3):
        flat[start:start + frames.size].copy_(torch.as_tensor(frames).reshape(-1))
        view = flat[start:start + frames.size].view(frames.shape)
        assert view.data_ptr() % 2 == 1
        data, _, off = raw_call(frames, 100, 3, cap, rgb=view)
        assert data[:len(whole)] == whole and off == offsets, f"rgb at byte offset {start}"


def _stac_cfg(rodent_cfg):
    from stac_mjx_amd.config import validate_config

    stac = dict(fit_offsets_path="fit.h5", ik_only_path="ik.h5", data_path="d.mat", continuous=False, n_fit_frames=10,
                skip_fit_offsets=False, skip_ik_only=False, infer_qvels=False, n_frames_per_clip=2,
                mujoco=dict(solver="newton", iterations=1, ls_iterations=4))
    return validate_config({"model": dict(rodent_cfg, MJCF_PATH="models/rodent.xml"), "stac": stac})


def test_stac_render_gpu_encoder_end_to_end(tmp_path, reference_dir, rodent_cfg, rodent_mocap):
    from stac_mjx_amd import jpeg, video
    from stac_mjx_amd.stac import Stac

    W, H, R = 97, 61, 7
    stac = Stac(reference_dir / "models" / "rodent.xml", _stac_cfg(rodent_cfg), list(rodent_cfg["KEYPOINT_MODEL_PAIRS"]), verbose=False)
    d = stac.ik_only(rodent_mocap[:4], stac.setup.tables.site_pos)
    args = (d.qpos, d.kp_data, d.offsets, 4)
    kw = dict(camera="close_profile", height=H, width=W, show_marker_error=True)
    base = stac.render(*args, tmp_path / "pil.avi", **kw)
    got = stac.render(*args, tmp_path / "gpu.avi", encoder="gpu", **kw)
    assert len(base) == 4 and jpeg.default_restart_mcus(W) == R
    np.testing.assert_array_equal(np.stack(got), np.stack(base))
    avi = video.read_avi(tmp_path / "gpu.avi")
    assert (avi["width"], avi["height"], avi["n_frames"]) == (W, H, 4)
    assert_files(avi["frames"], base, video.JPEG_QUALITY, R, "gpu.avi")
    assert stac.render(*args, tmp_path / "gpu2.avi", encoder="gpu", return_frames=False, **kw) == []
    assert (tmp_path / "gpu2.avi").read_bytes() == (tmp_path / "gpu.avi").read_bytes()
    assert stac.render(*args, tmp_path / "pil2.avi", return_frames=False, **kw) == []
    assert (tmp_path / "pil2.avi").read_bytes() == (tmp_path / "pil.avi").read_bytes()
    assert video.read_avi(tmp_path / "pil.avi")["frames"] == [video._jpeg(f) for f in base]  # the default file is what it was
    # several chunks, no raw frames to the host
    r, t = stac._get_renderer(), stac.setup.tables
    per_frame = W * H * 3 + jpeg.workspace_bytes(1, W, H, R) + jpeg.JpegEncoder.first_guess(1, W, H)
    budget, r.memory_budget = r.memory_budget, 3 * per_frame + 5  # chunks of 3 + 1 frames
    try:
        out = r.render(d.qpos[:4], d.kp_data[:4], d.offsets, qpos0=t.qpos0, parent=t.body_parentid, want_jpeg=True, want_rgb=False,
                       **kw)
    finally:
        r.memory_budget = budget
    assert "rgb" not in out and out["jpeg"] == avi["frames"]
