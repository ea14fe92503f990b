"""Cases and checkers of the offset phase on observed keypoints only (stac.offset_mask), shared by tests/test_mmask_host.py and
tests/test_gpu_mmask.py: ``cpu_rule``, a CPU build of the rule of csrc/mmask/stac_mmask.hpp (mmask_reference / mmask_finish, through
host_scaffold.build_cpu_library), and ``judge_partial`` / ``judge_finish``, a numpy float64 judge that shares none of the rule's
arithmetic (rotation matrices built from the quaternions in double, einsum, boolean masks), with the bounds it allows float32."""

import ctypes as C

import numpy as np

import host_scaffold as hs

DRIVER = r"""
#include "mmask/stac_mmask.hpp"
extern "C" void mmask_partial_rule(const float *kp, const float *xpos, const float *xquat, int nbody, const int *site_bodyid,
                                   const unsigned char *valid, long long T, int K, float *row, float *partial) {
    stac::mmask_reference(kp, xpos, xquat, nbody, (const int32_t *)site_bodyid, valid, T, K, row, partial);
}
extern "C" void mmask_finish_rule(const float *partial, int K, const float *m0, const float *dreg, float lam, float *offsets, float *err,
                                  int *n_out) {
    stac::mmask_finish(partial, K, m0, dreg, lam, offsets, err, (int32_t *)n_out);
}
extern "C" long long mmask_bytes(long long T, long long K) { return stac::mmask_workspace_bytes(T, K); }
"""

U = 2.0 ** -24  # the unit roundoff of float32


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def cpu_rule(tmp_path_factory):
    """-> (partial(kp, xpos, xquat, bodyid, valid) -> [4K + 2] float32,
    finish(partial, m0, dreg, lam) -> (offsets [K, 3] float32, err float32, n [K] int32), the library)"""
    lib = hs.build_cpu_library(tmp_path_factory, "mmask", DRIVER)
    lib.mmask_partial_rule.restype = None
    lib.mmask_partial_rule.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]
    lib.mmask_finish_rule.restype = None
    lib.mmask_finish_rule.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mmask_bytes.restype = C.c_longlong
    lib.mmask_bytes.argtypes = [C.c_longlong, C.c_longlong]

    def partial(kp, xpos, xquat, bodyid, valid):
        xpos, xquat = _f32(xpos), _f32(xquat)
        T, nbody = xpos.shape[0], xpos.shape[1]
        bodyid = np.ascontiguousarray(bodyid, dtype=np.int32)
        K = bodyid.size
        kp = _f32(kp).reshape(T, 3 * K)
        valid = np.ascontiguousarray(np.asarray(valid).reshape(T, K) != 0, dtype=np.uint8)
        assert xpos.shape == (T, nbody, 3) and xquat.shape == (T, nbody, 4)
        row, out = np.zeros(3 * K + 1, np.float32), np.full(4 * K + 2, -7.0, np.float32)
        lib.mmask_partial_rule(kp.ctypes.data, xpos.ctypes.data, xquat.ctypes.data, nbody, bodyid.ctypes.data, valid.ctypes.data, T, K,
                               row.ctypes.data, out.ctypes.data)
        return out

    def finish(part, m0, dreg, lam):
        part = _f32(part)
        K = (part.size - 2) // 4
        m0, dreg = _f32(m0).reshape(K, 3), _f32(dreg).reshape(K, 3)
        off, err, n = np.full((K, 3), -7.0, np.float32), np.full(1, -7.0, np.float32), np.full(K, -7, np.int32)
        lib.mmask_finish_rule(part.ctypes.data, K, m0.ctypes.data, dreg.ctypes.data, float(lam), off.ctypes.data, err.ctypes.data, n.ctypes.data)
        return off, err[0], n

    return partial, finish, lib


# ---- the float64 judge -----------------------------------------------------------------------------------------------------------
def rotations64(q):
    """[..., 4] quaternions (w, x, y, z; not normalised: the rule does not normalise either) -> [..., 3, 3] in double"""
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = 2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z
    return R


def sums64(kp, xpos, xquat, bodyid, valid):
    """-> dict of the float64 sums (s [K, 3], n [K], z2, T) and of the magnitudes that the float32 bounds are made of"""
    xpos, xquat = np.asarray(xpos, np.float64), np.asarray(xquat, np.float64)
    T, nbody = xpos.shape[0], xpos.shape[1]
    bodyid = np.asarray(bodyid)
    K = bodyid.size
    inside = (bodyid >= 0) & (bodyid < nbody)
    ok = (np.asarray(valid).reshape(T, K) != 0) & inside[None, :]
    b = np.where(inside, bodyid, 0)
    y = np.where(ok[..., None], np.asarray(kp, np.float64).reshape(T, K, 3), 0.0)  # (a masked value is never looked at)
    z = np.where(ok[..., None], y - xpos[:, b], 0.0)
    R = rotations64(xquat[:, b])
    r = np.einsum("tkji,tkj->tki", R, z)  # R^T z
    e = np.einsum("tkj,tkj->tk", z, z)
    qq = np.einsum("tkj,tkj->tk", xquat[:, b], xquat[:, b])
    return {"s": r.sum(axis=0), "n": ok.sum(axis=0), "z2": float(e.sum()), "T": T, "K": K,
            "mag_r": (qq * np.abs(z).sum(axis=-1) * ok).sum(axis=0), "mag_e": float(e.sum())}


def partial_bounds(J):
    """What float32 may be off by, from the format (U = 2^-24 per rounding) and the serial sums:
    r_i of one (t, k) is three products of a matrix entry and a z: z = y - p is one rounding (<= U |z|), a matrix entry is four
    products and three sums of quaternion words (<= 8 U |q|^2, the factor 2 is exact), the three products and two sums add 5 U of
    |q|^2 |z|_1: within 14 U |q|^2 |z|_1 =: 14 U a(t, k).  Their sum over T frames, in any order, adds at most (T - 1) U times the sum
    of |r| <= sum a.  So s[k][i] is within (14 + T) U sum_t a(t, k).
    e = z0^2 + z1^2 + z2^2: each z_i^2 is within 3 U of itself (two of z, one of the product), two sums: within 5 U e; summed over K
    keypoints and T frames: z2 within (5 + K + T) U sum e."""
    T, K = J["T"], J["K"]
    return (14 + T) * U * J["mag_r"][:, None] * np.ones((1, 3)), (5 + K + T) * U * J["mag_e"]


def judge_partial(partial, kp, xpos, xquat, bodyid, valid, label=""):
    """``partial`` [4K + 2] against the float64 sums within ``partial_bounds``; n and T exactly -> the judge's sums"""
    J = sums64(kp, xpos, xquat, bodyid, valid)
    K = J["K"]
    partial = np.asarray(partial)
    assert partial.shape == (4 * K + 2,) and partial.dtype == np.float32, label
    bs, bz = partial_bounds(J)
    s = partial[: 3 * K].astype(np.float64).reshape(K, 3)
    assert (np.abs(s - J["s"]) <= bs).all(), (label, "s", float(np.abs(s - J["s"]).max()), float(bs.max()))
    assert np.array_equal(partial[3 * K: 4 * K], J["n"].astype(np.float32)), (label, "n")
    assert abs(float(partial[4 * K]) - J["z2"]) <= bz, (label, "z2", float(partial[4 * K]), J["z2"], bz)
    assert partial[4 * K + 1] == np.float32(J["T"]), (label, "T")
    return J


def finish64(s, n, z2, m0, dreg, lam):
    """The closed form in double -> (v [K, 3], err)"""
    lam = float(np.float32(lam))
    m0, d = np.asarray(m0, np.float64).reshape(-1, 3), np.asarray(dreg, np.float64).reshape(-1, 3)
    denom = np.asarray(n, np.float64)[:, None] + lam * d
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(denom == 0, m0, (s + lam * d * m0) / denom)
    err = z2 - 2.0 * (v * s).sum() + (np.asarray(n, np.float64)[:, None] * v * v).sum() + lam * ((d * (v - m0)) ** 2).sum()
    return v, float(err)


def judge_finish(offsets, err, n_out, J, m0, dreg, lam, label=""):
    """``offsets`` / ``err`` / ``n_out`` of a finish of the sums that ``J`` judges, against ``finish64`` of the float64 sums.
    Bounds, again from the format: with bs the bound of s, numer = s + lam d m0 is within bs + 3 U (|s| + |lam d m0|) (two products,
    one sum), denom within 2 U |denom| (n is exact), the quotient adds U: v within bv = (bs + 3 U (|s| + |lam d m0|)) / |denom| +
    3 U |v|.  err = ((z2 - 2 A) + B) + lam C with A = sum v s, B = sum n v^2, C = sum (d (v - m0))^2, each a serial sum of 3 K terms:
    a term v s is within |s| bv + |v| bs + U |v s|, a term n v^2 within n (2 |v| bv + 2 U v^2), a term of C, with g = d (v - m0), within
    2 |g| d (bv + 2 U |v - m0|) + U g^2; each sum adds 3 K U of the sum of its terms' magnitudes; the three last operations add 3 U of
    |z2| + 2 |A| + |B| + lam C; and z2 comes with its own bound."""
    K = J["K"]
    lam64 = float(np.float32(lam))
    m0, d = np.asarray(m0, np.float64).reshape(K, 3), np.asarray(dreg, np.float64).reshape(K, 3)
    n = J["n"].astype(np.float64)[:, None]
    v, e = finish64(J["s"], J["n"], J["z2"], m0, d, lam)
    bs, bz = partial_bounds(J)
    s = J["s"]
    denom = n + lam64 * d
    with np.errstate(divide="ignore", invalid="ignore"):
        bv = np.where(denom == 0, 0.0, (bs + 3 * U * (np.abs(s) + np.abs(lam64 * d * m0))) / np.abs(denom) + 3 * U * np.abs(v))
    offsets = np.asarray(offsets, np.float64).reshape(K, 3)
    assert (np.abs(offsets - v) <= bv).all(), (label, "offsets", float(np.abs(offsets - v).max()), float(bv.max()))
    assert np.array_equal(np.asarray(n_out), J["n"].astype(np.int32)), (label, "n_out")
    tA = np.abs(s) * bv + np.abs(v) * bs + U * np.abs(v * s)
    tB = n * (2 * np.abs(v) * bv + 2 * U * v * v)
    g = d * (v - m0)
    tC = 2 * np.abs(g) * d * (bv + 2 * U * np.abs(v - m0)) + U * g * g
    A, B, Cc = np.abs(v * s).sum(), (n * v * v).sum(), (g * g).sum()
    be = bz + 2 * (tA.sum() + 3 * K * U * A) + (tB.sum() + 3 * K * U * B) + lam64 * (tC.sum() + 3 * K * U * Cc) \
        + 3 * U * (abs(J["z2"]) + 2 * A + B + lam64 * Cc)
    assert abs(float(err) - e) <= be, (label, "err", float(err), e, be)
    return v, e, be


# ---- cases -----------------------------------------------------------------------------------------------------------------------
NBODY = 5
TS = (1, 63, 64, 65, 130, 1000)
KS = (1, 23, 64)
MASKS = ("all_valid", "all_invalid", "one_kp_never", "one_frame_only", "random30")


def poses(T, K, seed, nbody=NBODY):
    """Random unit quaternions, positions and keypoints -> kp [T, 3K], xpos [T, nbody, 3], xquat [T, nbody, 4], bodyid [K]"""
    rng = np.random.default_rng(seed)
    xquat = rng.normal(0.0, 1.0, (T, nbody, 4))
    xquat = (xquat / np.linalg.norm(xquat, axis=-1, keepdims=True)).astype(np.float32)
    xpos = rng.normal(0.0, 0.1, (T, nbody, 3)).astype(np.float32)
    bodyid = rng.integers(0, nbody, K).astype(np.int32)
    kp = (xpos[:, bodyid] + rng.normal(0.0, 0.03, (T, K, 3))).astype(np.float32).reshape(T, 3 * K)
    return kp, xpos, xquat, bodyid


def mask(kind, T, K, seed):
    rng = np.random.default_rng(seed + 77)
    if kind == "all_valid":
        return np.ones((T, K), bool)
    if kind == "all_invalid":
        return np.zeros((T, K), bool)
    if kind == "one_kp_never":
        v = np.ones((T, K), bool)
        v[:, K // 2] = False
        return v
    if kind == "one_frame_only":
        v = np.zeros((T, K), bool)
        v[T // 2] = True
        return v
    assert kind == "random30"
    return rng.random((T, K)) >= 0.3


FILLERS = (np.nan, np.inf, -np.inf, 1e30)


def with_fillers(kp, valid, seed):
    """``kp`` with every masked keypoint overwritten by NaN / inf / -inf / 1e30, drawn per coordinate"""
    rng = np.random.default_rng(seed + 99)
    T, K = valid.shape
    fill = np.asarray(FILLERS, np.float32)[rng.integers(0, len(FILLERS), (T, K, 3))]
    return np.where(valid[..., None], kp.reshape(T, K, 3), fill).astype(np.float32).reshape(T, 3 * K)


def case(T, K, kind):
    """(label, kp, xpos, xquat, bodyid, valid, m0, dreg, lam) of one shape and mask; random30 carries the fillers"""
    seed = 1000 * K + T
    kp, xpos, xquat, bodyid = poses(T, K, seed)
    valid = mask(kind, T, K, seed)
    if kind == "random30":
        kp = with_fillers(kp, valid, seed)
    rng = np.random.default_rng(seed + 5)
    m0 = rng.normal(0.0, 0.02, (K, 3)).astype(np.float32)
    dreg = np.zeros((K, 3), np.float32)
    dreg[::3] = 1.0  # every third keypoint is regularised (the first one always)
    return f"T{T}_K{K}_{kind}", kp, xpos, xquat, bodyid, valid, m0, dreg, 0.5


def all_cases():
    return [case(T, K, kind) for T in TS for K in KS for kind in MASKS]


# ---- the reference's six known-answer m_opt cases (its tests/unit/test_m_opt.py, as tests/test_oracle.py states them) -----------------
GT_A = np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6], [0.15, 0.25, 0.35]], np.float32)
GT_B = np.array([[0.2, -0.1, 0.4], [0.3, 0.4, -0.2], [-0.1, 0.3, 0.1]], np.float32)


def known_answer_cases():
    """(label, q [T, 3], ground-truth offsets, m0, dreg, lam): every m_opt call of the six cases"""
    z, one = np.zeros((3, 3), np.float32), np.ones((3, 3), np.float32)
    sweep = np.zeros((8, 3), np.float32)
    sweep[:, 0] = np.linspace(0.0, np.pi / 4, 8)
    rows = np.zeros((3, 3), np.float32)
    rows[0] = 1.0
    half = np.full((3, 3), 0.5, np.float32)
    r42 = np.random.RandomState(42).randn(10, 3)
    return [
        ("identity", np.zeros((5, 3), np.float32), GT_A, z, z, 0.0),
        ("varied", (r42 * 0.5).astype(np.float32), GT_A, z, z, 0.0),
        ("sweep", sweep, GT_B, GT_B, z, 0.0),
        ("large", (np.random.RandomState(99).randn(15, 3) * 1.5).astype(np.float32), GT_B, z, z, 0.0),
        ("reg_zero", (r42 * 0.3).astype(np.float32), GT_A, np.full((3, 3), 99.0, np.float32), one, 0.0),
        ("reg_strong", (r42 * 0.3).astype(np.float32), GT_A, z, one, 1e6),
        ("partial_reg_strong", np.zeros((10, 3), np.float32), half, z, rows, 1e4),
        ("partial_reg_none", np.zeros((10, 3), np.float32), half, z, rows, 0.0),
    ]


def oracle_bodies(orc, q):
    """xpos [T, nbody, 3], xquat [T, nbody, 4] of the poses ``q`` by the oracle's kinematics"""
    out = [orc.fk(row) for row in np.asarray(q, np.float32)]
    return np.stack([o["xpos"] for o in out]), np.stack([o["xquat"] for o in out])


# ---- holes (the value test and the end-to-end test) ----------------------------------------------------------------------------------
def cut_holes(kp, n_kp, run, seed):
    """``n_kp`` keypoints drawn with ``seed`` lose one run of ``run`` frames each, strictly inside the series, and the runs are filled
    linearly between their neighbours -> (filled [T, 3K] float32, valid [T, K] bool, the keypoints)"""
    T, K = kp.shape[0], kp.shape[1] // 3
    rng = np.random.default_rng(seed)
    which = np.sort(rng.choice(K, n_kp, replace=False))
    out, valid = kp.reshape(T, K, 3).astype(np.float32).copy(), np.ones((T, K), bool)
    for k in which:
        a = int(rng.integers(1, T - run))  # rows a .. a + run - 1 are missing; a - 1 and a + run are there
        w = (np.arange(1, run + 1, dtype=np.float64) / (run + 1))[:, None]
        out[a: a + run, k] = ((1.0 - w) * out[a - 1, k] + w * out[a + run, k]).astype(np.float32)
        valid[a: a + run, k] = False
    return out.reshape(T, 3 * K), valid, which
