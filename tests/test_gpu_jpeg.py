"""The GPU JPEG encoder (csrc/stac_jpeg.hip) against Pillow's bytes, at tolerance 0: small images of every edge shape at three
qualities and five restart intervals, batches of frames of unequal length, a scan whose size prefix sum spans several workgroups,
the capacity contract of stac_jpeg_encode, stale workspace / other stream / odd byte offset, and Stac.render(encoder="gpu") end
to end.  Then what those leave out (jpeg_ref.edge_images, what they emit is asserted in tests/test_jpeg_host.py): words of up
to 55 bits at every bit position, three ZRL codes, nearly every AC symbol, 0xFF bytes where stuffing can go wrong; every shape
of 1..33 pixels, every quality, a DRI above 255, the product's 1920 x 1200, the size limits, more than 2^18 and 2^20 intervals
in one call, stale registers, and a seeded fuzz.  tests/test_jpeg_host.py shows (without a GPU) that tests/jpeg_ref.py states
the same rule as Pillow."""

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


restart_cases = jpeg_ref.restart_cases  # 1, 3, 8, one MCU row, more than all MCUs (DRI present, no marker)


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


@pytest.fixture(scope="module")
def large_scan_frames():
    frames = np.random.default_rng(7).integers(0, 256, (5, 528, 528, 3), dtype=np.uint8)
    frames[3, :, :264] = 128  # frames of unequal length
    return frames, [jpeg_ref.pillow(f, 90, 1) for f in frames]


def test_large_scan(large_scan_frames):
    """1089 intervals per frame, 5445 in the call: the size prefix sum spans six workgroups."""
    frames, want = large_scan_frames
    assert_files(gpu(frames, 90, 1), frames, 90, 1, "528x528")
    assert gpu(frames, 90, 1) == want


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


# ---- what the cases above leave out ---------------------------------------------------------------------------------------------
EDGE = jpeg_ref.edge_images()


@pytest.mark.parametrize("name", list(EDGE))
def test_edge_images(name):
    """Alone, and as frame 1 of a batch between noise and its own mirror image."""
    img, q = EDGE[name]
    H, W = img.shape[:2]
    batch = np.stack([np.random.default_rng(5).integers(0, 256, img.shape, dtype=np.uint8), img, img[::-1, ::-1]])
    for R in restart_cases(W, H):
        assert_files(gpu(img[None], q, R), [img], q, R, name)
        assert_files(gpu(batch, q, R), batch, q, R, name + " in a batch")


SIDES = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33)


@pytest.mark.parametrize("W", SIDES)
def test_every_small_shape(W):
    rng = np.random.default_rng(100 + W)
    for H in SIDES:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        for R in (1, (W + 15) // 16):
            assert_files(gpu(img[None], 75, R), [img], 75, R, f"{W}x{H}")


@pytest.mark.parametrize("name", ["sat33x17", "noise48x32"])
def test_every_quality(name):
    """Both branches of the quality scaling, the clamps of a table entry at 1 and at 255."""
    img = IMAGES[name] if name in IMAGES else np.random.default_rng(48).integers(0, 256, (32, 48, 3), dtype=np.uint8)
    for q in range(1, 101):
        assert_files(gpu(img[None], q, 2), [img], q, 2, name)


@pytest.mark.parametrize("R", [300, 65535])
def test_restart_interval_above_255(R):
    """420 MCUs: the high byte of the DRI segment is not zero; at R = 300 one marker."""
    img = np.random.default_rng(336).integers(0, 256, (320, 336, 3), dtype=np.uint8)
    assert_files(gpu(img[None], 90, R), [img], 90, R, "336x320")


def render_like(H, W, seed=0):
    """Black background, flat-shaded discs and bars."""
    rng = np.random.default_rng(seed)
    out = np.zeros((H, W, 3), np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for _ in range(12):
        cy, cx, rad = int(rng.integers(H)), int(rng.integers(W)), int(rng.integers(20, 200))
        out[(yy - cy) ** 2 + (xx - cx) ** 2 < rad * rad] = rng.integers(30, 256, 3)
    for _ in range(8):
        y, x = int(rng.integers(H)), int(rng.integers(W))
        out[y:y + int(rng.integers(4, 40)), x:x + int(rng.integers(50, 900))] = rng.integers(30, 256, 3)
    return out


def test_product_size_batch():
    from stac_mjx_amd.video import JPEG_QUALITY

    frames = np.stack([np.random.default_rng(1920).integers(0, 256, (1200, 1920, 3), dtype=np.uint8), render_like(1200, 1920)])
    for q in (JPEG_QUALITY, 100):
        assert_files(gpu(frames, q, 120), frames, q, 120, "1920x1200")


def test_product_size_rendered_frame(reference_dir, rodent_cfg, rodent_mocap):
    from stac_mjx_amd import jpeg, video
    from stac_mjx_amd.stac import Stac

    stac = Stac(reference_dir / "models" / "rodent.xml", _stac_cfg(rodent_cfg), list(rodent_cfg["KEYPOINT_MODEL_PAIRS"]), verbose=False)
    r, t = stac._get_renderer(), stac.setup.tables
    out = r.render(np.asarray(t.qpos0)[None], rodent_mocap[:1], t.site_pos, qpos0=t.qpos0, parent=t.body_parentid,
                   camera="close_profile", width=1920, height=1200, show_marker_error=True, want_jpeg=True)
    rgb = out["rgb"].numpy()
    assert rgb.shape == (1, 1200, 1920, 3) and len(np.unique(rgb.reshape(-1, 3), axis=0)) > 10  # a picture, not a blank frame
    assert_files(out["jpeg"], rgb, video.JPEG_QUALITY, jpeg.default_restart_mcus(1920), "rendered 1920x1200")


@pytest.mark.parametrize("W,H", [(65500, 8), (8, 65500)])
def test_largest_size_of_libjpeg(W, H):
    img = np.random.default_rng(W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    for R in (1, (W + 15) // 16):
        assert_files(gpu(img[None], 90, R), [img], 90, R, f"{W}x{H}")


@pytest.mark.parametrize("W,H", [(65535, 1), (1, 65535)])
def test_largest_size_of_the_format(W, H):
    """libjpeg refuses more than 65500: the yardstick is the restatement."""
    img = np.random.default_rng(H).integers(0, 256, (H, W, 3), dtype=np.uint8)
    R = 7 if W > H else 4096
    got, want = gpu(img[None], 75, R), jpeg_ref.encode(img, 75, R)
    assert got[0] == want, f"{W}x{H}: {first_difference(got[0], want)}"


@pytest.mark.parametrize("N", [262147, (1 << 20) + 5])
def test_many_intervals(N):
    """Frames of 1 x 1 pixel, one interval each.  More than 256 tiles of 1024 intervals: the scan of the tile sums goes round
    twice and carries; more than 2^20 intervals: the entropy and pack kernels' workgroups take a second interval."""
    greys = (0, 37, 90, 128, 171, 222, 255)
    files = [jpeg_ref.pillow(np.full((1, 1, 3), g, np.uint8), 90, 1) for g in greys]
    assert len({len(f) for f in files}) > 1  # so the offsets are not multiples of one length
    pick = np.random.default_rng(N).integers(0, len(greys), N)
    frames = np.repeat(np.asarray(greys, np.uint8)[pick][:, None, None, None], 3, -1)
    lengths = np.asarray([len(f) for f in files], np.int64)[pick]
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    want = np.frombuffer(b"".join(files[k] for k in pick), np.uint8)
    data, guard, off = raw_call(frames, 90, 1, int(offsets[-1]))
    assert (guard == 0xA5).all()
    off = np.asarray(off, np.int64)
    bad = np.flatnonzero(off != offsets)
    assert len(bad) == 0, f"frame_offset differs first at frame {bad[0]}: {off[bad[0]]} / {offsets[bad[0]]}"
    got = np.frombuffer(data, np.uint8)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"{len(bad)} bytes differ, the first at {bad[0]} (frame {np.searchsorted(offsets, bad[0], 'right') - 1})"


def test_stale_registers(large_scan_frames):
    """The long words and the large scan once more, each behind a launch that fills scratch memory and the vector registers of
    every wavefront slot with a pattern (tests/tools/poison_scratch.hip): nothing may be read before it is written."""
    import ctypes

    from build_tools import build_poison_tool

    lib = ctypes.CDLL(str(build_poison_tool()))
    lib.poison_scratch.argtypes = [ctypes.c_void_p, ctypes.c_uint32]

    def poison(value):
        assert lib.poison_scratch(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), value) == 0

    for value in (0xFFFFFFFF, 0x7FC00000):
        for name in ("luma_tail", "chroma_tail"):
            img, q = EDGE[name]
            for R in (1, 13):
                poison(value)
                assert_files(gpu(img[None], q, R), [img], q, R, f"{name} after poison {value:#x}")
        frames, want = large_scan_frames
        poison(value)
        got = gpu(frames, 90, 1)
        assert got == want, f"528x528 after poison {value:#x}"


def run_fuzz_case(c):
    """One jpeg_ref.fuzz_case through stac_jpeg_encode with the frames at an odd byte offset and an output of exactly the
    files' size -> None, or what differs."""
    frames, q, R = c["frames"], c["quality"], c["R"]
    want = [jpeg_ref.pillow(f, q, R) for f in frames]
    whole, offsets = b"".join(want), [int(x) for x in np.cumsum([0] + [len(w) for w in want])]
    flat = torch.zeros(frames.size + 8, dtype=torch.uint8, device=DEV)
    flat[c["offset"]:c["offset"] + frames.size].copy_(torch.as_tensor(np.ascontiguousarray(frames)).reshape(-1))
    view = flat[c["offset"]:c["offset"] + frames.size].view(frames.shape)
    assert view.data_ptr() % 2 == 1
    data, guard, off = raw_call(frames, q, R, len(whole), rgb=view)
    what = f"{c['kind']} {frames.shape} q={q} R={R} offset={c['offset']}"
    if not (guard == 0xA5).all():
        return what + ": bytes written beyond the capacity"
    if off != offsets:
        return what + f": frame_offset {off} / {offsets}"
    if data != whole:
        return what + ": " + first_difference(data, whole)
    return None


@pytest.mark.parametrize("part", range(3))
def test_seeded_fuzz(part):
    """150 cases: content family, W and H up to 96, quality 1..100, R from 1 to more than all MCUs, 1..4 frames."""
    bad = [f"seed {seed}: {msg}" for seed in range(50 * part, 50 * part + 50) if (msg := run_fuzz_case(jpeg_ref.fuzz_case(seed)))]
    assert not bad, "\n".join(bad)
