"""Builds the HIP extension in-tree: ``stac_mjx_amd/csrc/libstac_hip.so`` and its companions
``stac_mjx_amd/csrc/select/libstac_select.so``, ``stac_mjx_amd/csrc/mmask/libstac_mmask.so``,
``stac_mjx_amd/csrc/seam/libstac_seam.so`` and ``stac_mjx_amd/csrc/ground/libstac_ground.so`` (gfx950 only).

``hipcc`` cross-compiles without a GPU.  ``-ffp-contract=off -fno-fast-math`` is part of the
arithmetic contract of the kernels (bit-identical to the CPU oracle), not a tuning choice.
"""

from __future__ import annotations

import os
import shutil
import subprocess
from pathlib import Path

CSRC = Path(__file__).resolve().parent / "csrc"
LIB = CSRC / "libstac_hip.so"
# every unit and every header of csrc and of include/: a new file cannot be missing from the build or from source_digest()
SOURCES = sorted(CSRC.glob("*.hip"))
HEADERS = sorted(CSRC.glob("*.hpp")) + sorted((CSRC.parents[1] / "include").glob("*.h"))
# -amdgpu-opt-vgpr-liverange=false: SIOptimizeVGPRLiveRange is the pass behind round 3's stale-state defect (a latency-kernel
# shape whose results depended on what the previous launch left in registers / scratch): with it off that shape is correct under
# every poison pattern, with it on it is wrong on 36 of 36 models (profiles/r04/stale_spill_repro.txt, reproducer:
# tests/tools/repro_stale_spill/).  Costs nothing on the throughput bench, 2 % on 250-frame clips.
# -amdgpu-sched-strategy=max-ilp: with the split kinematics (round 5) the kernels wait on dependent instructions more than on LDS reads
# (dependent VALU instructions of a wavefront do not overlap: profiles/r04/valu_issue_micro.txt): +3 % on the 10 000-frame bench, +4.6 % on
# 250-frame clips over max-memory-clause, which rounds 3-4 used (profiles/r05/NOTES.md).
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-strict-aliasing", "-fno-slp-vectorize",
         "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-mllvm", "-amdgpu-opt-vgpr-liverange=false"]
FLAGS += os.environ.get("STAC_HIP_EXTRA_FLAGS", "").split()


def hipcc_path() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (ROCm toolchain required to build libstac_hip.so)")


STAMP = CSRC / "libstac_hip.so.stamp"
# The companion library of stac.fit_frames (csrc/select/: its own C header, digest and stamp).  ABI v3 of libstac_hip.so stays as it
# is; the directory is matched by neither glob above.  The rule header includes csrc/stac_pairwise.hpp, so HEADERS are in its digest.
SELECT_DIR = CSRC / "select"
SELECT_LIB = SELECT_DIR / "libstac_select.so"
SELECT_STAMP = SELECT_DIR / "libstac_select.so.stamp"
SELECT_SOURCES = sorted(SELECT_DIR.glob("*.hip"))
SELECT_HEADERS = sorted(SELECT_DIR.glob("*.hpp")) + sorted(SELECT_DIR.glob("*.h"))
# The companion library of stac.offset_mask (csrc/mmask/: the offset phase on observed keypoints only), built the same way.  Its C
# header includes include/stac_hip.h for the status codes, so HEADERS are in its digest.
MMASK_DIR = CSRC / "mmask"
MMASK_LIB = MMASK_DIR / "libstac_mmask.so"
MMASK_STAMP = MMASK_DIR / "libstac_mmask.so.stamp"
MMASK_SOURCES = sorted(MMASK_DIR.glob("*.hip"))
MMASK_HEADERS = sorted(MMASK_DIR.glob("*.hpp")) + sorted(MMASK_DIR.glob("*.h"))
# The companion library of stac.seam_report (csrc/seam/: the pose steps of a fitted series), built the same way.
SEAM_DIR = CSRC / "seam"
SEAM_LIB = SEAM_DIR / "libstac_seam.so"
SEAM_STAMP = SEAM_DIR / "libstac_seam.so.stamp"
SEAM_SOURCES = sorted(SEAM_DIR.glob("*.hip"))
SEAM_HEADERS = sorted(SEAM_DIR.glob("*.hpp")) + sorted(SEAM_DIR.glob("*.h"))
# The companion library of stac.ground (csrc/ground/: the ground clearance of fitted poses), built the same way.
GROUND_DIR = CSRC / "ground"
GROUND_LIB = GROUND_DIR / "libstac_ground.so"
GROUND_STAMP = GROUND_DIR / "libstac_ground.so.stamp"
GROUND_SOURCES = sorted(GROUND_DIR.glob("*.hip"))
GROUND_HEADERS = sorted(GROUND_DIR.glob("*.hpp")) + sorted(GROUND_DIR.glob("*.h"))


def source_digest() -> str:
    """sha256 over the sources, headers and flags: what the library was built from (modification times do not survive a copy
    of the tree to another machine)."""
    import hashlib

    h = hashlib.sha256(" ".join(FLAGS).encode())
    for p in SOURCES + HEADERS:
        h.update(p.name.encode())
        h.update(p.read_bytes())
    return h.hexdigest()


def select_digest() -> str:
    """``source_digest`` of ``libstac_select.so``."""
    import hashlib

    h = hashlib.sha256(" ".join(FLAGS).encode())
    for p in SELECT_SOURCES + SELECT_HEADERS + HEADERS:
        h.update(p.name.encode())
        h.update(p.read_bytes())
    return h.hexdigest()


def mmask_digest() -> str:
    """``source_digest`` of ``libstac_mmask.so``."""
    import hashlib

    h = hashlib.sha256(" ".join(FLAGS).encode())
    for p in MMASK_SOURCES + MMASK_HEADERS + HEADERS:
        h.update(p.name.encode())
        h.update(p.read_bytes())
    return h.hexdigest()


def seam_digest() -> str:
    """``source_digest`` of ``libstac_seam.so``."""
    import hashlib

    h = hashlib.sha256(" ".join(FLAGS).encode())
    for p in SEAM_SOURCES + SEAM_HEADERS + HEADERS:
        h.update(p.name.encode())
        h.update(p.read_bytes())
    return h.hexdigest()


def ground_digest() -> str:
    """``source_digest`` of ``libstac_ground.so``."""
    import hashlib

    h = hashlib.sha256(" ".join(FLAGS).encode())
    for p in GROUND_SOURCES + GROUND_HEADERS + HEADERS:
        h.update(p.name.encode())
        h.update(p.read_bytes())
    return h.hexdigest()


def is_stale() -> bool:
    if not LIB.exists() or not STAMP.exists():
        return True
    return STAMP.read_text().strip() != source_digest()


def select_is_stale() -> bool:
    return not SELECT_LIB.exists() or not SELECT_STAMP.exists() or SELECT_STAMP.read_text().strip() != select_digest()


def mmask_is_stale() -> bool:
    return not MMASK_LIB.exists() or not MMASK_STAMP.exists() or MMASK_STAMP.read_text().strip() != mmask_digest()


def seam_is_stale() -> bool:
    return not SEAM_LIB.exists() or not SEAM_STAMP.exists() or SEAM_STAMP.read_text().strip() != seam_digest()


def ground_is_stale() -> bool:
    return not GROUND_LIB.exists() or not GROUND_STAMP.exists() or GROUND_STAMP.read_text().strip() != ground_digest()


def _compile(sources, lib, stamp, digest, verbose):
    import time

    cmd = [hipcc_path(), *FLAGS, *map(str, sources), "-o", str(lib)]
    t0 = time.perf_counter()
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + res.stdout + res.stderr)
    stamp.write_text(digest() + "\n")
    if verbose:
        print(res.stdout + res.stderr)
        print(f"[stac build] {' '.join(cmd)}\n[stac build] compiled in {time.perf_counter() - t0:.0f} s, sources sha256 {digest()[:16]}")


def build_extension(force: bool = False, verbose: bool = False) -> Path:
    """Builds what is stale (``force``: all five libraries) -> the path of ``libstac_hip.so``; ``libstac_select.so`` stands beside
    it in ``csrc/select``, ``libstac_mmask.so`` in ``csrc/mmask``, ``libstac_seam.so`` in ``csrc/seam`` and ``libstac_ground.so`` in
    ``csrc/ground``."""
    if force or ground_is_stale():
        _compile(GROUND_SOURCES, GROUND_LIB, GROUND_STAMP, ground_digest, verbose)
    if force or seam_is_stale():
        _compile(SEAM_SOURCES, SEAM_LIB, SEAM_STAMP, seam_digest, verbose)
    if force or mmask_is_stale():
        _compile(MMASK_SOURCES, MMASK_LIB, MMASK_STAMP, mmask_digest, verbose)
    if force or select_is_stale():
        _compile(SELECT_SOURCES, SELECT_LIB, SELECT_STAMP, select_digest, verbose)
    if force or is_stale():
        _compile(SOURCES, LIB, STAMP, source_digest, verbose)
    return LIB


if __name__ == "__main__":
    print(build_extension(force=True, verbose=True))
