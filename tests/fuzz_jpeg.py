"""Not collected by pytest: `python tests/fuzz_jpeg.py N [max_side]` on a GPU box.  The GPU JPEG encoder on N seeded random cases
of the families of tests/test_gpu_jpeg.py::test_seeded_fuzz (jpeg_ref.fuzz_case: noise, saturated noise, smooth, flat shapes,
sparse DCT blocks in luminance or chrominance; 1..4 frames, quality 1..100, R from 1 to 65535, frames at an odd byte offset) at
sides up to max_side (default 400): every file must equal Pillow's byte for byte, frame_offset the true sizes, nothing written
beyond the capacity.  Prints every case that differs with its first differing byte, then a count."""
import sys
sys.path.insert(0, "tests"); sys.path.insert(0, "tests/tools"); sys.path.insert(0, ".")
import jpeg_ref
import test_gpu_jpeg as T
n, side = int(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 400
c = jpeg_ref.fuzz_case(0)
assert jpeg_ref.encode(c["frames"][0], c["quality"], c["R"]) == jpeg_ref.pillow(c["frames"][0], c["quality"], c["R"]), "tests/jpeg_ref.py != Pillow"
bad = frames = 0
for seed in range(n):
    c = jpeg_ref.fuzz_case(10000 + seed, side)
    frames += len(c["frames"])
    msg = T.run_fuzz_case(c)
    if msg:
        bad += 1; print("seed", seed, "DIFFERS:", msg)
print("ran", n, "cases,", frames, "frames, sides up to", side, "- differ from Pillow:", bad)
