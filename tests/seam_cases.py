"""Cases and checkers of the pose steps (stac.seam_report) and of the warm-started clips (stac.seam_passes), shared by
tests/test_seam_host.py and tests/test_gpu_seam.py: ``cpu_rule``, a CPU build of the rule of csrc/seam/stac_seam.hpp (seam_reference,
through host_scaffold.build_cpu_library); ``judge``, a numpy float32 judge that shares none of its code (whole-array operations, one
rounding each, argmax and boolean masks instead of the serial pass); the shapes; and ``oracle_seam_passes``, the restatement of
Stac.ik_only(passes=P) driven by the CPU oracle."""

import ctypes as C

import numpy as np

import host_scaffold as hs

DRIVER = r"""
#include "seam/stac_seam.hpp"
extern "C" void seam_rule(const float *qpos, long long N, int nq, long long clip_len, const int *quat_cols, int n_quat, int n_lin,
                          float *step_joint, int *step_col, float *step_rot, float *step_lin2, float *col_max_in, float *col_max_seam) {
    stac::seam_reference(qpos, N, nq, clip_len, (const int32_t *)quat_cols, n_quat, n_lin, step_joint, (int32_t *)step_col, step_rot,
                         step_lin2, col_max_in, col_max_seam);
}
extern "C" int seam_layout(int nq, const int *quat_cols, int n_quat, int n_lin) {
    return stac::seam_check_layout(nq, (const int32_t *)quat_cols, n_quat, n_lin);
}
"""

OUTPUTS = ("step_joint", "step_col", "step_rot", "step_lin2", "col_max_in", "col_max_seam")
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def cpu_rule(tmp_path_factory):
    """-> (steps(qpos, clip_len, quat_cols, n_lin) -> dict of the six outputs (numpy), the library)"""
    lib = hs.build_cpu_library(tmp_path_factory, "seam", DRIVER)
    lib.seam_rule.restype = None
    lib.seam_rule.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_longlong, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6
    lib.seam_layout.restype = C.c_int
    lib.seam_layout.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int]

    def steps(qpos, clip_len, quat_cols=(), n_lin=0):
        q = _f32(qpos)
        N, nq = q.shape
        cols = np.ascontiguousarray(quat_cols, dtype=np.int32).reshape(-1)
        out = {"step_joint": np.full(N, -7.0, np.float32), "step_col": np.full(N, -7, np.int32), "step_rot": np.full(N, -7.0, np.float32),
               "step_lin2": np.full(N, -7.0, np.float32), "col_max_in": np.full(nq, -7.0, np.float32), "col_max_seam": np.full(nq, -7.0, np.float32)}
        lib.seam_rule(q.ctypes.data, N, nq, int(clip_len), cols.ctypes.data if cols.size else None, int(cols.size), int(n_lin),
                      *[out[k].ctypes.data for k in OUTPUTS])
        return out

    return steps, lib


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, label=""):
    """Tolerance 0 on every word of the six outputs"""
    for k in OUTPUTS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (label, k, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(bits(g), bits(w)):
            i = int(np.flatnonzero(bits(g) != bits(w))[0])
            raise AssertionError((label, k, i, g[i], w[i], int((bits(g) != bits(w)).sum())))


# ---- the numpy float32 judge -------------------------------------------------------------------------------------------------------
def judge(qpos, clip_len, quat_cols=(), n_lin=0):
    """The rule as whole-array float32 operations -> the six outputs"""
    q = _f32(qpos)
    N, nq = q.shape
    cols = [int(c) for c in quat_cols]
    in_block = np.zeros(nq, bool)
    for c in cols:
        in_block[c: c + 4] = True
    scalar = np.flatnonzero(~in_block & (np.arange(nq) >= n_lin))
    out = {"step_joint": np.zeros(N, np.float32), "step_col": np.full(N, -1, np.int32), "step_rot": np.zeros(N, np.float32),
           "step_lin2": np.zeros(N, np.float32), "col_max_in": np.zeros(nq, np.float32), "col_max_seam": np.zeros(nq, np.float32)}
    if N < 2:
        return out
    a, b = q[:-1], q[1:]
    with np.errstate(all="ignore"):
        d = np.abs(b - a)
        if scalar.size:
            ds = d[:, scalar]
            bad = ~np.isfinite(ds).all(axis=1)
            safe = np.where(np.isfinite(ds), ds, np.float32(-1))
            out["step_joint"][1:] = np.where(bad, QNAN, safe.max(axis=1))
            out["step_col"][1:] = np.where(bad, -1, scalar[safe.argmax(axis=1)])  # (argmax: the first of equals)
        measure = d.copy()
        if cols:
            R = np.empty((N - 1, len(cols)), np.float32)
            for i, c in enumerate(cols):
                dot = ((a[:, c] * b[:, c] + a[:, c + 1] * b[:, c + 1]) + a[:, c + 2] * b[:, c + 2]) + a[:, c + 3] * b[:, c + 3]
                R[:, i] = np.float32(1) - np.abs(dot)
                measure[:, c] = R[:, i]
                measure[:, c + 1: c + 4] = 0
            rbad = ~np.isfinite(R).all(axis=1)
            out["step_rot"][1:] = np.where(rbad, QNAN, np.where(np.isfinite(R), R, -np.inf).max(axis=1).astype(np.float32))
        if n_lin == 3:
            s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            out["step_lin2"][1:] = np.where(np.isfinite(s), s, QNAN)
        m = np.where(np.isfinite(measure) & (measure > 0), measure, np.float32(0))
    seam = np.arange(1, N) % int(clip_len) == 0
    if seam.any():
        out["col_max_seam"] = m[seam].max(axis=0)
    if (~seam).any():
        out["col_max_in"] = m[~seam].max(axis=0)
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------
NS = (1, 2, 63, 64, 65, 130)
NQS = (1, 7, 74, 230)
CLIPS = (1, 5, 13, None)  # None: one clip of N rows
SECOND_BLOCK = {74: 62, 230: 126}  # (a block that straddles the 64th / 128th column; elsewhere the row's last four columns)


def layouts(nq):
    """(quat_cols, n_lin) of every layout of n_quat in {0, 1, 2} x n_lin in {0, 3} that a row of nq columns has room for; the
    second block comes first in the table (any order is allowed)"""
    out = []
    for n_lin in (0, 3):
        if n_lin > nq:
            continue
        out.append(((), n_lin))
        if n_lin + 4 <= nq:
            out.append(((n_lin,), n_lin))
            second = SECOND_BLOCK.get(nq, nq - 4)
            if second >= n_lin + 4:
                out.append(((second, n_lin), n_lin))
    return out


def series(N, nq, quat_cols, seed, quantised):
    """Random poses; the blocks are unit quaternions, except the first of the table where it has two, or where it has one and the
    series is not quantised: those are scaled by 1.5 (|dot| > 1: a negative r).  ``quantised``: multiples of 1 / 8, so that several
    columns tie for the largest step"""
    rng = np.random.default_rng(seed)
    q = rng.normal(0.0, 0.3, (N, nq))
    if quantised:
        q = np.round(q * 8) / 8
    for i, c in enumerate(quat_cols):
        v = rng.normal(0.0, 1.0, (N, 4))
        q[:, c: c + 4] = v / np.linalg.norm(v, axis=1, keepdims=True) * (1.5 if i == 0 and (len(quat_cols) == 2 or not quantised) else 1.0)
    return q.astype(np.float32)


def cases(nq, ns=NS):
    """(label, qpos, clip_len, quat_cols, n_lin) over the shapes of one nq"""
    out = []
    for N in ns:
        for k, (cols, n_lin) in enumerate(layouts(nq)):
            q = series(N, nq, cols, 7919 * N + 31 * nq + k, quantised=(N + k) % 2 == 0)
            for L in sorted({N if L is None else L for L in CLIPS}):
                if N % L == 0:
                    out.append((f"N{N}_nq{nq}_L{L}_quat{len(cols)}_lin{n_lin}", q, L, cols, n_lin))
    return out


POISONS = [(v, where) for v in (np.nan, np.inf, -np.inf) for where in ("scalar", "block", "lin")]


def poisoned(N, nq, value, where, rows=(1, 52)):
    """A case of two blocks and a translation (nq >= 74, clips of 13 rows) with ``value`` in one column of the rows ``rows``, the
    second of which opens a clip"""
    cols, n_lin = ((SECOND_BLOCK.get(nq, nq - 4), 3), 3)
    q = series(N, nq, cols, 4242 + nq, quantised=False)
    j = {"scalar": 9, "block": cols[0] + 2, "lin": 1}[where]
    for t in rows:
        q[t, j] = value
    return f"N{N}_nq{nq}_{value}_{where}", q, 13, cols, n_lin


# ---- the restatement of Stac.ik_only(passes=P), driven by the oracle ------------------------------------------------------------------
def oracle_seam_passes(orc, fs, kp_clips, passes, F=None, solver="pg", nthreads=0, **solver_kw):
    """Pass 1: every clip cold (``ik_clips`` as ik_only calls it).  Pass p >= 2: the clips 1 .. solved again without root optimisation
    from row F - 1 (F None: the last row) of the ``qpos`` that the clip in front of them had after pass p - 1; clip 0 keeps its pass-1
    result.  ``solver`` "lm": ``ik_clips_lm`` with ``solver_kw`` (maxiter, lambda0).  -> the list of the per-pass outputs (every pass a
    full copy: qpos, xpos, xquat, marker_sites, frame_error)"""
    run = orc.ik_clips if solver == "pg" else orc.ik_clips_lm
    kp_clips = _f32(kp_clips)
    F = kp_clips.shape[1] if F is None else F
    args = (fs.lb, fs.ub, fs.part_masks, fs.trunk_kps, max(fs.root_kp_idx, 0), fs.root_dims)
    keys = ("qpos", "xpos", "xquat", "marker_sites", "frame_error")
    first = run(kp_clips, *args, do_root_opt=fs.do_root_opt, nthreads=nthreads, **solver_kw)
    outs = [{k: first[k].copy() for k in keys}]
    for _ in range(1, passes):
        prev = outs[-1]
        cur = {k: prev[k].copy() for k in keys}
        if kp_clips.shape[0] > 1:
            warm = run(kp_clips[1:], *args, do_root_opt=False, q_init=np.ascontiguousarray(prev["qpos"][:-1, F - 1]), nthreads=nthreads,
                       **solver_kw)
            for k in keys:
                cur[k][1:] = warm[k]
        outs.append(cur)
    return outs


def seam_jumps(qpos_clips, scalar, F=None):
    """[C - 1]: per clip border the largest absolute difference over the columns ``scalar`` between row F - 1 of the clip in front and
    the first row of the clip behind"""
    q = np.asarray(qpos_clips)
    F = q.shape[1] if F is None else F
    return np.abs(q[1:, 0][:, scalar] - q[:-1, F - 1][:, scalar]).max(axis=1)
