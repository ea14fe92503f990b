"""Shared by tests/test_wrench_sweep_host.py and tests/test_gpu_wrench_sweeps.py: the wrench-sum program of a model as the host plans it
(stac_debug_wsum_program: plan construction only, no device), a float32 emulation of that program in numpy, and small hand-made lean
models -- a free root, hinges below it -- whose site ranges sit where a part of the program can go wrong."""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

NONE = 0xFF      # a capture byte that is nobody's range (kWsumNone, stac_plan.hpp)
MAX_DEPTH = 4    # kWsumMaxDepth


@dataclass
class WsumProgram:
    planned: bool
    ntask: int
    nwhole: int
    nrows: int
    depth: int
    row_start: tuple
    nrange: int
    K: int
    table_words: int
    staged_words: int
    stride16: int
    lds_bytes: int
    mb_words: int
    kxf: int
    c_sw: int
    c_rw: int
    rsplit: int
    staged_words_without: int
    dump: int             # c3_rw0: where the sweeps store a sum that is nobody's
    ranges: np.ndarray    # [nrange, 2] lo, hi
    recs: np.ndarray      # [ntask + nwhole, 4] lo, mid, hi, rid_mid | rid_hi << 16
    rows: np.ndarray      # [nrows, 16, 4] word of the lane's wrench entry (from c_sw), store words of steps 0 | 1, of 2 | 3, capture bytes

    def swept(self):
        """{range index: (row, lane, step)} of the ranges that come out of the sweeps"""
        out = {}
        for row in range(self.nrows):
            for lane in range(16):
                for s in range(MAX_DEPTH):
                    rid = (int(self.rows[row, lane, 3]) >> (8 * s)) & 0xFF
                    if rid != NONE:
                        assert rid not in out, f"range {rid} is captured twice"
                        out[rid] = (row, lane, s)
        return out


def _model_tables(tables, lb, ub):
    from stac_mjx_amd.engine import StacModelTables, _f32p, _i32p

    t = StacModelTables()
    t.nbody, t.njnt, t.nq, t.nsite = tables.nbody, tables.njnt, tables.nq, tables.nsite
    keep = []
    for name, ctype, dt, src in [
        ("body_parentid", _i32p, np.int32, tables.body_parentid), ("body_pos", _f32p, np.float32, tables.body_pos),
        ("body_quat", _f32p, np.float32, tables.body_quat), ("body_jntadr", _i32p, np.int32, tables.body_jntadr),
        ("body_jntnum", _i32p, np.int32, tables.body_jntnum), ("jnt_type", _i32p, np.int32, tables.jnt_type),
        ("jnt_qposadr", _i32p, np.int32, tables.jnt_qposadr), ("jnt_bodyid", _i32p, np.int32, tables.jnt_bodyid),
        ("jnt_pos", _f32p, np.float32, tables.jnt_pos), ("jnt_axis", _f32p, np.float32, tables.jnt_axis),
        ("qpos0", _f32p, np.float32, tables.qpos0), ("site_bodyid", _i32p, np.int32, tables.site_bodyid),
        ("site_pos", _f32p, np.float32, tables.site_pos), ("lb", _f32p, np.float32, lb), ("ub", _f32p, np.float32, ub),
    ]:  # fmt: skip
        arr = np.ascontiguousarray(src, dtype=dt)
        keep.append(arr)
        setattr(t, name, arr.ctypes.data_as(ctype))
    return t, keep


def wsum_program(tables, lb, ub) -> WsumProgram:
    """The wrench-sum program the host plans for the model (under the environment's developer switches, read by the call)."""
    from stac_mjx_amd.engine import StacModelTables, load_library

    lib = load_library()
    t, keep = _model_tables(tables, lb, ub)
    fn = lib.stac_debug_wsum_program
    fn.restype = C.c_int32
    fn.argtypes = [C.POINTER(StacModelTables), C.c_void_p, C.c_int32]
    out = np.zeros(1 << 16, np.int32)
    rc = fn(C.byref(t), out.ctypes.data, out.size)
    assert rc == 0, lib.stac_last_error().decode()
    del keep
    h = [int(x) for x in out[:24]]
    nrange = h[8]
    ranges = out[24:24 + 2 * nrange].reshape(nrange, 2).copy()
    tab = out[24 + 2 * nrange:24 + 2 * nrange + h[10]].copy()
    nrec = h[1] + h[2]
    recs = tab[:4 * nrec].reshape(nrec, 4)
    rows = tab[4 * nrec:].reshape(h[3], 16, 4) if h[0] else np.zeros((0, 16, 4), np.int32)
    if h[0]:
        assert tab.size == 4 * nrec + 64 * h[3]
    return WsumProgram(bool(h[0]), h[1], h[2], h[3], h[4], (h[5], h[6], h[7]), nrange, h[9], h[10], h[11], h[12], h[13], h[14], h[15],
                       h[16], h[17], h[18], h[19], h[20], ranges, recs, rows)


def left_to_right(w, lo, hi):
    """The oracle's sum of a range: from +0, one float32 addition per site in sorted order.  w: [K, 6] float32 -> [6] float32"""
    acc = np.zeros(6, np.float32)
    with np.errstate(all="ignore"):
        for i in range(lo, hi):
            acc = (acc + w[i]).astype(np.float32)
    return acc


def emulate(pr: WsumProgram, w):
    """Runs the program as the kernel does on the wrench entries w [K, 6] float32.  -> ({range index: [6] float32}, number of times
    each range was produced).  The sweeps run on whole rows of 16 lanes: a lane behind its row's end holds the row's last site, lane 0
    takes +0 from outside the row."""
    out, times = {}, np.zeros(pr.nrange, np.int64)

    def put(rid, v):
        out[rid] = np.array(v, np.float32)
        times[rid] += 1

    with np.errstate(all="ignore"):
        for row in range(pr.nrows):
            words = pr.rows[row, :, 0]
            assert (words % pr.kxf == 0).all()
            wl = w[words // pr.kxf]                                   # [16, 6]: the lane's wrench
            acc = (np.zeros_like(wl) + wl).astype(np.float32)         # A_0 = 0 + w
            for s in range(pr.depth):
                if s > 0:
                    shifted = np.vstack([np.zeros((1, 6), np.float32), acc[:-1]])
                    acc = (shifted + wl).astype(np.float32)
                for lane in range(16):
                    rid = (int(pr.rows[row, lane, 3]) >> (8 * s)) & 0xFF
                    pair = int(pr.rows[row, lane, 1 + s // 2]) & 0xFFFFFFFF
                    word = (pair >> 16) if s & 1 else (pair & 0xFFFF)
                    # the store word is the range's entry, or the dump entry
                    assert word == (pr.dump if rid == NONE else pr.c_rw + pr.kxf * rid), (row, lane, s, word)
                    if rid != NONE:
                        put(rid, acc[lane])
            for lane in range(16):  # no capture beyond the depth
                for s in range(pr.depth, MAX_DEPTH):
                    assert (int(pr.rows[row, lane, 3]) >> (8 * s)) & 0xFF == NONE
        for q in range(pr.ntask):
            lo, mid, hi, rids = (int(x) for x in pr.recs[q])
            assert lo <= mid <= hi
            acc = np.zeros(6, np.float32)
            for i in range(lo, mid):
                acc = (acc + w[i]).astype(np.float32)
            if (rids & 0xFFFF) != (rids >> 16):
                put(rids & 0xFFFF, acc)
            else:
                assert mid == hi
            for i in range(mid, hi):
                acc = (acc + w[i]).astype(np.float32)
            put(rids >> 16, acc)
        for q in range(pr.ntask, pr.ntask + pr.nwhole):
            lo, mid, hi, rids = (int(x) for x in pr.recs[q])
            assert mid == hi and (rids & 0xFFFF) == (rids >> 16)
            put(rids >> 16, left_to_right(w, lo, hi))
    return out, times


def special_wrenches(rng, K):
    """Random float32 wrench entries with +0.0, -0.0, denormals, infinities and NaN at random sites."""
    w = rng.standard_normal((K, 6)).astype(np.float32) * np.float32(10.0) ** rng.integers(-3, 4, (K, 6)).astype(np.float32)
    specials = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x7F800000, 0xFF800000, 0x7FC00000], np.uint32)
    hit = rng.random((K, 6)) < 0.25
    w.view(np.uint32)[hit] = rng.choice(specials, int(hit.sum()))
    return w


def check_program(pr: WsumProgram, rng, what, rounds=2):
    """Every range some joint reads is produced exactly once, and bit-equal to the left-to-right sum from zero."""
    assert pr.planned, what
    for _ in range(rounds):
        w = special_wrenches(rng, pr.K)
        out, times = emulate(pr, w)
        assert (times == 1).all(), (what, times.tolist())
        for r, (lo, hi) in enumerate(pr.ranges.tolist()):
            ref = left_to_right(w, lo, hi)
            assert (out[r].view(np.uint32) == ref.view(np.uint32)).all(), (what, r, lo, hi)


# ---- hand-made lean models -----------------------------------------------------------------------------------------------------------
def spec_model(spec, order="sorted", seed=0):
    """A lean model from a nested description.  spec = (own sites, hinges, [child specs]) of the ROOT body, which carries the free joint
    (its `hinges` is ignored); bodies are numbered depth first, so a body's subtree is a run of sorted sites: its own, then its
    children's.  order: "sorted" -- the sites are declared in (body, site) order; "interleaved" -- declared round-robin over the
    bodies, as the rodent's are, so that site index and sorted position differ.  -> ModelTables"""
    from stac_mjx_amd.mjcf import JNT_FREE, JNT_HINGE, ModelTables

    rng = np.random.default_rng(4242 + seed)
    parent, own, nh = [0, 0], [0], [0]  # world, then the bodies

    def walk(node, par):
        sites, hinges, children = node
        b = len(own)
        own.append(sites)
        nh.append(hinges)
        if b > 1:
            parent.append(par)
        for ch in children:
            walk(ch, b)

    walk(spec, 0)
    nbody = len(own)
    depth = [0] * nbody
    for b in range(1, nbody):
        depth[b] = depth[parent[b]] + 1
    body_pos = rng.normal(0, 0.05, (nbody, 3))
    body_quat = np.tile([1.0, 0, 0, 0], (nbody, 1))
    jt, jadr, jbody, jpos, jaxis, jrange, qpos0 = [JNT_FREE], [0], [1], [np.zeros(3)], [np.eye(3)[2]], [[0, 0]], [0, 0, 0.1, 1, 0, 0, 0]
    body_jntadr, body_jntnum = [-1] * nbody, [0] * nbody
    body_jntadr[1], body_jntnum[1] = 0, 1
    nq = 7
    for b in range(2, nbody):
        body_jntadr[b], body_jntnum[b] = len(jt), nh[b]
        for _ in range(nh[b]):
            v = rng.normal(0, 1, 3)
            jt.append(JNT_HINGE)
            jadr.append(nq)
            jbody.append(b)
            jpos.append(np.zeros(3) if rng.random() < 0.4 else rng.normal(0, 0.02, 3))
            jaxis.append(v / np.linalg.norm(v))
            jrange.append([-1.0, 1.2])
            qpos0.append(0.0)
            nq += 1
    by_body = [b for b in range(1, nbody) for _ in range(own[b])]
    if order == "interleaved":
        left = {b: own[b] for b in range(1, nbody)}
        by_body = []
        while any(left.values()):
            for b in range(1, nbody):
                if left[b]:
                    by_body.append(b)
                    left[b] -= 1
    K = len(by_body)
    return ModelTables(
        nbody=nbody, njnt=len(jt), nq=nq, nsite=K, body_parentid=np.array(parent, np.int32), body_pos=body_pos.astype(np.float32),
        body_quat=body_quat.astype(np.float32), body_jntadr=np.array(body_jntadr, np.int32), body_jntnum=np.array(body_jntnum, np.int32),
        body_depth=np.array(depth, np.int32), jnt_type=np.array(jt, np.int32), jnt_qposadr=np.array(jadr, np.int32),
        jnt_bodyid=np.array(jbody, np.int32), jnt_pos=np.array(jpos, np.float32).reshape(-1, 3),
        jnt_axis=np.array(jaxis, np.float32).reshape(-1, 3), jnt_range=np.array(jrange, np.float32).reshape(-1, 2),
        qpos0=np.array(qpos0, np.float32), site_bodyid=np.array(by_body, np.int32), site_pos=rng.normal(0, 0.01, (K, 3)).astype(np.float32),
        body_names=[f"b{i}" for i in range(nbody)], jnt_names=[f"j{i}" for i in range(len(jt))], site_names=[f"s{i}" for i in range(K)])


def leaf(n, hinges=1):
    return (n, hinges, [])


def chain(sites_per_body):
    """bodies one below the other, the first on top"""
    node = None
    for n in reversed(sites_per_body):
        node = (n, 1, [node] if node else [])
    return node


def leaves(*sizes):
    return (0, 1, [leaf(n) for n in sizes])


# The models of tests/test_gpu_wrench_sweeps.py by name: the root body's spec.  What the host must plan for each is asserted by
# tests/test_wrench_sweep_host.py (no device) and again, from the same entry, by the GPU test.
MODELS = {
    # ranges of 1 .. 6 sites that all end on lane 6 (a chain of six one-site bodies): four sums of one lane are ranges, 5 and 6 sites are
    # past the deepest sweep; two leaves of 2 and 3 sites behind them
    "lengths": (0, 1, [chain([1, 1, 1, 1, 1, 1]), leaf(2), leaf(3)]),
    # 16 sites: one full row, the last range ends on lane 15
    "row16": leaves(3, 4, 2, 3, 4),
    # 17 sites: two rows, every cut from 1 to 16 is admissible
    "row17": leaves(2, 2, 2, 2, 2, 2, 2, 2, 1),
    # 20 sites, (14, 18) lies across sorted position 16: the cut moves to where no range crosses it, and the range is swept
    "cross16": leaves(2, 4, 4, 4, 4, 2),
    # 32 sites: the only cut is 16.  (12, 16) ends on the last lane of row 0, (16, 20) starts on lane 0 of row 1 ...
    "row32": leaves(3, 3, 3, 3, 4, 4, 3, 3, 3, 3),
    # ... and here (14, 18) crosses it: four sites, but not a sweep's
    "row32_cross": leaves(4, 4, 3, 3, 4, 4, 4, 3, 3),
    # prefix groups.  Three ranges from site 0 -- the root's (0, 21), A's (0, 13), A1's (0, 8); A and A1 carry no site above their first
    # child, A1 has two hinges on the one range -- and (13, 21) of B and its child: the root's checkpoint, 13 sites, falls on the first
    # site of a remainder
    "prefix3": (0, 1, [(0, 1, [(0, 2, [leaf(8)]), leaf(5)]), (0, 1, [leaf(8)])]),
    # two ranges from site 0 twice over: (0, 20) with (0, 16) -- the checkpoint is the last site of a loop trip -- and (0, 9), (9, 16)
    "prefix2": (0, 1, [(0, 2, [leaf(9), leaf(7)]), leaf(4)]),
    "one_site": (1, 1, []),
    "body20": (0, 1, [leaf(20, 2)]),
    "body32": (0, 1, [leaf(32)]),
}
