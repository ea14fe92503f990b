"""The JPEG path on the host (no GPU): the numpy restatement tests/jpeg_ref.py equals Pillow byte for byte (so Pillow's bytes can
be the yardstick of tests/test_gpu_jpeg.py) on the parity images, the edge images and a seeded sweep; the edge images make the
streams that they are there for (jpeg_ref.stats: long words at every bit position, three ZRL codes, every DC category, all but
a listed few AC symbols, 0xFF bytes where stuffing can go wrong); the library's header equals Pillow's, the entry points are exported and refuse bad
arguments, Stac.render refuses bad encoder arguments before any device work, and write_avi takes pre-encoded frames alone."""

import ctypes as C

import numpy as np
import pytest

import jpeg_ref

IMAGES = jpeg_ref.images()
QUALITIES = (35, 90, 100)


def test_the_image_list_is_the_one_the_parity_tests_name():
    shapes = {k: v.shape[:2] for k, v in IMAGES.items()}
    assert shapes == {"noise97x61": (61, 97), "noise100x36": (36, 100), "grad50x40": (40, 50), "smooth130x90": (90, 130),
                      "const16x16": (16, 16), "tiny5x3": (3, 5), "one1x1": (1, 1), "sat33x17": (17, 33), "shapes160x64": (64, 160)}


@pytest.mark.parametrize("name", list(IMAGES))
def test_restatement_equals_pillow(name):
    img = IMAGES[name]
    for q in QUALITIES:
        for R in (0, 1, 3, 8):  # 0: plain save, no DRI
            got, want = jpeg_ref.encode(img, q, R), jpeg_ref.pillow(img, q, R)
            assert got == want, (name, q, R, len(got), len(want))


EDGE = jpeg_ref.edge_images()
# AC symbols (run << 4 | size, size 1..10) that no parity or edge image emits.  A long run in front of a coefficient of 9 or 10
# bits needs a high-frequency amplitude that 8-bit pixels (chrominance: the RGB cube) do not hold.  The issue's caps: 8 and 34.
MISSING_AC = {"luma": [0x5A, 0x7A, 0xC9, 0xE7, 0xE9, 0xEA], "chroma": [0xC8, 0xC9, 0xCA, 0xE4, 0xEA]}


@pytest.mark.parametrize("name", list(EDGE))
def test_restatement_equals_pillow_on_edge_images(name):
    img, q = EDGE[name]
    for R in (0,) + jpeg_ref.restart_cases(img.shape[1], img.shape[0]):
        got, want = jpeg_ref.encode(img, q, R), jpeg_ref.pillow(img, q, R)
        assert got == want, (name, q, R, len(got), len(want))
        assert jpeg_ref.restuffed(jpeg_ref.stats(img, q, R)) == jpeg_ref.scan(img, q, R), (name, R)  # stats() sees that stream


def _union(stats):
    out = {k: dict(dc=set(), ac=set(), zrl=set(), eob=False, no_eob=False, longest=0, long_at=set()) for k in ("luma", "chroma")}
    for st in stats:
        for k, u in out.items():
            for f in ("dc", "ac", "zrl", "long_at"):
                u[f] |= st[k][f]
            u["eob"], u["no_eob"], u["longest"] = u["eob"] or st[k]["eob"], u["no_eob"] or st[k]["no_eob"], max(u["longest"], st[k]["longest"])
    return out


@pytest.fixture(scope="module")
def exercised():
    """stats() of every case that tests/test_gpu_jpeg.py gives the encoder from images() and edge_images(): name -> [stats]."""
    out = {}
    for name, img in IMAGES.items():
        out[name] = [jpeg_ref.stats(img, q, R) for q in QUALITIES for R in jpeg_ref.restart_cases(img.shape[1], img.shape[0])]
    for name, (img, q) in EDGE.items():
        out[name] = [jpeg_ref.stats(img, q, R) for R in jpeg_ref.restart_cases(img.shape[1], img.shape[0])]
    return out


def test_tail_images_make_the_long_words(exercised):
    luma, chroma = exercised["luma_tail"][0]["luma"], exercised["chroma_tail"][0]["chroma"]
    assert luma["ac"] == {0xE6} and luma["zrl"] == {3} and luma["longest"] == 55 and luma["no_eob"] and not luma["eob"]
    assert 0xE5 in chroma["ac"] and 3 in chroma["zrl"] and chroma["longest"] == 51 and chroma["no_eob"]
    # behind noise, one interval (R more than all MCUs): a word that needs a third 32-bit word at every bit position, 0 included
    for table in ("luma", "chroma"):
        at = set()
        for seed in range(3):
            st = exercised[f"{table}_tail_behind_noise{seed}"][-1]
            assert len(st["intervals"]) == 1
            at |= st[table]["long_at"]
        assert at == set(range(32)), (table, sorted(set(range(32)) - at))


def test_what_the_images_exercise(exercised):
    u = _union(st for sts in exercised.values() for st in sts)
    for table in ("luma", "chroma"):
        assert u[table]["dc"] == set(range(12)), table
        assert {1, 2, 3} <= u[table]["zrl"], table
        assert u[table]["eob"] and u[table]["no_eob"], table
    assert u["luma"]["longest"] >= 54 and u["chroma"]["longest"] >= 50
    assert max(st["mcu_bits"] for sts in exercised.values() for st in sts) > 4096  # an MCU over many staged words
    stuffing = set().union(*(jpeg_ref.stuffing(st) for sts in exercised.values() for st in sts))
    assert stuffing == {"pair", "last", "pos0", "pos1", "pos2", "pos3", "round"}
    # the seeded stuffing images hold them on their own
    assert {"pair", "last"} <= jpeg_ref.stuffing(exercised["stuffing_pair_last"][0])  # R = 1
    assert "round" in jpeg_ref.stuffing(exercised["stuffing_round"][-1])  # one interval


def test_ac_symbols_missing_are_the_listed_ones(exercised):
    u = _union(st for sts in exercised.values() for st in sts)
    assert len(MISSING_AC["luma"]) <= 8 and len(MISSING_AC["chroma"]) <= 34
    for table in ("luma", "chroma"):
        missing = sorted(set((r << 4) | s for r in range(16) for s in range(1, 11)) - u[table]["ac"])
        assert missing == MISSING_AC[table], (table, [hex(m) for m in missing])


def test_restatement_equals_pillow_on_a_seeded_sweep():
    """The yardstick of the GPU fuzz is itself checked: quality 1..100, sides below 64, R 0..19, every content family."""
    n = 0
    for seed in range(300):
        rng = np.random.default_rng(seed)
        kind = jpeg_ref.FAMILIES[seed % len(jpeg_ref.FAMILIES)]
        img = jpeg_ref.content(rng, kind, int(rng.integers(1, 64)), int(rng.integers(1, 64)))
        q, R = int(rng.integers(1, 101)), int(rng.integers(0, 20))
        assert jpeg_ref.encode(img, q, R) == jpeg_ref.pillow(img, q, R), (seed, kind, img.shape, q, R)
        n += 1
    for seed in range(40):  # and the cases of the GPU fuzz as they are
        c = jpeg_ref.fuzz_case(seed)
        for f in c["frames"]:
            assert jpeg_ref.encode(f, c["quality"], c["R"]) == jpeg_ref.pillow(f, c["quality"], c["R"]), (seed, c["kind"])
    assert n == 300


def _sos_end(data):
    at = data.index(b"\xff\xda")
    return at + 2 + int.from_bytes(data[at + 2:at + 4], "big")


@pytest.mark.parametrize("W,H", [(97, 61), (1, 1), (1920, 1200), (65500, 2), (65535, 3)])
def test_header_equals_pillow(W, H):
    from stac_mjx_amd.build import build_extension
    from stac_mjx_amd.jpeg import jpeg_header

    build_extension()
    for q in (1, 35, 49, 50, 90, 100):
        for R in (0, 1, 3, 8, 65535):
            mine = jpeg_header(W, H, q, R)
            assert mine == jpeg_ref.header(W, H, q, R), (W, H, q, R)
            if max(W, H) <= 65500:  # libjpeg's own limit; the format (and the library) go to 65535
                want = jpeg_ref.pillow(np.zeros((H, W, 3), np.uint8), q, R)
                assert mine == want[:_sos_end(want)], (W, H, q, R)


def test_symbols_and_argument_errors():
    from stac_mjx_amd.build import build_extension
    from stac_mjx_amd.engine import ABI_SYMBOLS, StacHipError, load_library
    from stac_mjx_amd import jpeg

    build_extension()
    lib = load_library()
    for s in ("stac_jpeg_header", "stac_jpeg_workspace_bytes", "stac_jpeg_encode"):
        assert s in ABI_SYMBOLS and hasattr(lib, s), s
    assert lib.stac_abi_version() == 3
    assert lib.stac_jpeg_header(16, 16, 90, 4, None, 0) == len(jpeg.jpeg_header(16, 16, 90, 4)) == 629
    small = (C.c_uint8 * 10)()
    assert lib.stac_jpeg_header(16, 16, 90, 4, small, 10) < 0 and b"smaller" in lib.stac_last_error()
    for bad in ((0, 16, 90, 1), (16, 65536, 90, 1), (16, 16, 0, 1), (16, 16, 101, 1), (16, 16, 90, -1), (16, 16, 90, 65536)):
        with pytest.raises(StacHipError):
            jpeg.jpeg_header(*bad)
    assert jpeg.workspace_bytes(0, 16, 16, 1) >= 0 and jpeg.workspace_bytes(3, 97, 61, 7) > 3 * 28 * 6 * 64
    for bad in ((-1, 16, 16, 1), (1, 0, 16, 1), (1, 16, 65536, 1), (1, 16, 16, 0), (1, 16, 16, 65536)):
        with pytest.raises(StacHipError):
            jpeg.workspace_bytes(*bad)
    # stac_jpeg_encode checks its arguments before it touches the device; N = 0 is a no-op
    enc = lambda N, W, H, q, R, ptr=None, ws=0: lib.stac_jpeg_encode(N, W, H, q, R, ptr, ptr, 0, ptr, ptr, ws, None)
    assert enc(0, 16, 16, 90, 1) == 0
    for bad in ((-1, 16, 16, 90, 1), (1, 0, 16, 90, 1), (1, 16, 70000, 90, 1), (1, 16, 16, 0, 1), (1, 16, 16, 101, 1),
                (1, 16, 16, 90, 0), (1, 16, 16, 90, 65536), (1, 16, 16, 90, 1)):  # the last: null pointers
        assert enc(*bad) == -1 and lib.stac_last_error_code() == -1, bad
    with pytest.raises(ValueError, match="CUDA"):
        jpeg.encode_jpegs_gpu(np.zeros((1, 4, 4, 3), np.uint8))


def test_stac_render_encoder_errors_before_any_device_work(tmp_path):
    from stac_mjx_amd.stac import Stac

    s = object.__new__(Stac)  # no engine: every check below must fire before one would be used
    s._xml_path, s._renderer = None, None
    q, kp = np.zeros((10, 7)), np.zeros((10, 3))
    with pytest.raises(ValueError, match="unknown encoder"):
        s.render(q, kp, None, 2, tmp_path / "v.avi", encoder="nvjpeg")
    with pytest.raises(ValueError, match="avi"):
        s.render(q, kp, None, 2, tmp_path / "v.mp4", encoder="gpu")
    with pytest.raises(ValueError, match="MJCF"):  # accepted names reach the next check
        s.render(q, kp, None, 2, tmp_path / "v.avi", encoder="gpu", return_frames=False)
    with pytest.raises(ValueError, match="MJCF"):
        s.render(q, kp, None, 2, tmp_path / "v.avi", encoder="pil")
    assert not list(tmp_path.iterdir())


def test_viz_stac_passes_the_encoder_keywords_only_when_given(monkeypatch, tmp_path):
    import types

    import stac_mjx_amd
    from stac_mjx_amd import viz

    calls = []
    cfg = types.SimpleNamespace(model=types.SimpleNamespace(MJCF_PATH="m.xml"))
    d = types.SimpleNamespace(qpos=np.zeros((5, 7)), kp_data=np.ones((5, 3)), kp_names=["a"], offsets=np.zeros((1, 3)))

    class FakeStac:
        def __init__(self, *a):
            pass

        def render(self, *a, **kw):
            calls.append(kw)
            return []

    monkeypatch.setattr(viz.io, "load_stac_data", lambda p: (cfg, d))
    monkeypatch.setattr("stac_mjx_amd.stac.Stac", FakeStac)
    stac_mjx_amd.viz_stac(tmp_path / "r.h5", 3, tmp_path / "o.avi", base_path=tmp_path)
    stac_mjx_amd.viz_stac(tmp_path / "r.h5", 3, tmp_path / "o.avi", base_path=tmp_path, encoder="gpu", return_frames=False)
    assert calls == [{}, {"encoder": "gpu", "return_frames": False}]


def test_write_avi_from_jpegs_alone(tmp_path):
    from stac_mjx_amd.video import read_avi, write_avi

    imgs = [IMAGES["noise97x61"], IMAGES["noise97x61"][::-1], IMAGES["noise97x61"][:, ::-1]]
    jpegs = [jpeg_ref.pillow(im, 90, 7) for im in imgs]
    write_avi(tmp_path / "a.avi", None, 25.0, jpegs=jpegs, size=(97, 61))
    avi = read_avi(tmp_path / "a.avi")
    assert avi["frames"] == jpegs and (avi["width"], avi["height"], avi["n_frames"]) == (97, 61, 3) and avi["fps"] == 25.0
    assert [s for _, s in avi["index"]] == [len(j) for j in jpegs]
    # the same file as from raw frames with these JPEGs, and the default path is what it was
    write_avi(tmp_path / "b.avi", imgs, 25.0, jpegs=jpegs)
    assert (tmp_path / "a.avi").read_bytes() == (tmp_path / "b.avi").read_bytes()
    with pytest.raises(ValueError, match="no frames"):
        write_avi(tmp_path / "c.avi", None, 25.0, jpegs=[], size=(97, 61))
    with pytest.raises(ValueError, match="no frames"):
        write_avi(tmp_path / "c.avi", [], 25.0)
