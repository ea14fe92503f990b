"""Scripts of entry-point calls for ONE long-lived model, and what each call must return whatever ran before it.

A `stac_model` carries host-side state from call to call ("What a model carries between calls": the mask table and its cache,
the pruned root programs, the per-call box, the LM tables, the chain-order work space, the control word, the site offsets).  Every
other GPU test builds a fresh engine per kind of call, so only the cache-hit path is covered there.  Here a script is a list of
units, a unit is a tuple of steps (one step, or a refusal with the step that must follow it), and a step is one entry-point call
with all its arguments, the per-call parameters it sets on the engine and the site offsets it runs with.  The expectation of a step
comes from the stateless `oracle.Oracle` with the same arguments, so a step is defined on its own: a warm start is the ORACLE's carry
of the step it continues, never a GPU output, and a script may run in any order (tests/test_gpu_call_sequence.py runs each in order,
reversed and on a side stream).  tests/test_call_sequence_host.py shows on the oracle alone that every state-changing transition
would be noticed: the new step with one piece left at the previous step's value differs in bits.

Building all expectations (scripts A-D, `build_all`) takes 1.8 s of wall time on a machine with 8 CPUs and 4.4 s on another one (the oracle runs the clips of
a call in parallel): script A 0.9 s (0.1 s once the oracle's library is loaded), B and D 0.03 s each, script C's 4096 + 3 x 2048
chains of 10 iterations and 4096 poses 0.4 s -- it does not dominate, so its `maxiter` stays at 10.  Measured by
test_call_sequence_host.py::test_expectations_are_affordable, which prints the figure and bounds it at 60 s.
"""

from __future__ import annotations

import time
from dataclasses import dataclass, replace
from types import SimpleNamespace

import numpy as np

from helpers import _edge_tables
from test_gpu_loop_head import MAXITER, STARTS, TOL
from test_gpu_parity import _box, _random_tables

LM_LAMBDA0 = 1e-2  # Engine's default (lm_lambda0)


@dataclass(frozen=True)
class Params:
    """What a step sets on the engine before its call (`apply_params`)."""
    tol: float = TOL
    maxiter: int = MAXITER
    maxls: int = 15
    lanes_per_chain: int = 16
    solver: str = "pg"
    lm_maxiter: int = 20


@dataclass
class Step:
    name: str
    call: str  # "q_phase" | "q_solve" | "fk" | "m_opt"
    args: dict
    params: Params
    offsets: np.ndarray | None = None  # the site offsets in force ([K, 3]; None: the model's own)
    refuse: str | None = None  # the call must return this error (a regular expression) before any launch
    kernel: object = None  # predicate on stac_debug_last_q_kernel's four words after the call (PG launches only)
    verbose: object = None  # predicate on the fields of the call's last "[stac] q_phase..." lines (engines with STAC_HIP_VERBOSE)
    same_as: str | None = None  # the step whose expectation this one repeats bit for bit
    order: bool = False  # q_phase: chain ordering runs (the work space is grown to the largest such C so far)
    reads_order: bool = False  # ... and the launch keeps the order: its chain queue hands the chains out through `perm`
    expect: object = None
    engine: str = "main"  # script D: which of the two engines


def apply_params(eng, p: Params):
    """Sets a step's per-call parameters on an engine: `params` (stac_q_solve) and `phase_params` (stac_q_phase) are plain ctypes
    structs, `solver` is what Engine.q_phase looks at before it copies tol / maxiter over."""
    from stac_mjx_amd.engine import SOLVERS

    for s in (eng.params, eng.phase_params):
        s.tol, s.maxls, s.lanes_per_chain = float(p.tol), int(p.maxls), int(p.lanes_per_chain)
    eng.params.maxiter = int(p.maxiter)
    eng.solver = p.solver
    eng.phase_params.solver = SOLVERS[p.solver]
    eng.phase_params.maxiter = int(p.lm_maxiter if p.solver == "lm" else p.maxiter)
    eng.phase_params.lm_lambda0 = LM_LAMBDA0


def _freeze(x):
    if isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, np.ndarray):
        x.setflags(write=False)
    return x


def expected(model, st: Step):
    """The stateless answer of a step: the oracle with the step's own parameters, offsets and arguments."""
    from oracle import Oracle

    p, a = st.params, st.args
    orc = Oracle(model.tables, tol=p.tol, maxiter=p.maxiter, maxls=p.maxls)
    if st.offsets is not None:
        orc.set_site_pos(st.offsets)
    if st.call == "q_phase":
        kw = dict(do_root_opt=a["do_root_opt"], q_init=a["q_init"], want_bodies=a["want_bodies"])
        if p.solver == "lm":
            kw.update(maxiter=p.lm_maxiter, lambda0=LM_LAMBDA0)
        fn = orc.ik_clips_lm if p.solver == "lm" else orc.ik_clips
        ref = fn(a["kp"], model.lb, model.ub, a["part_masks"], a["trunk_kps"], a["root_kp_idx"], a["root_dims"], **kw)
        ref["carry_qpos"] = ref["qpos"][:, -1].copy()
        return _freeze(ref)
    if st.call == "q_solve":
        lb, ub = (model.lb, model.ub) if a["lb"] is None else (a["lb"], a["ub"])
        xs, sts, cnt = [], [], []
        for n in range(len(a["kp"])):
            x, s = orc.q_opt(a["kp"][n], a["qs_to_opt"], a["kps_to_opt"], a["q0"][n], lb, ub)
            xs.append(x)
            sts.append(np.array([s["error"], s["stepsize"], s["t"], s["loss"]], np.float32))
            cnt.append([s["iter_num"], s["ls_evals"], s["grad_evals"], 1])
        return _freeze(dict(qpos=np.stack(xs), state=np.stack(sts), counters=np.array(cnt, np.int32)))
    if st.call == "fk":
        rs = [orc.fk(q) for q in a["qpos"]]
        return _freeze({k: np.stack([r[k] for r in rs]) for k in a["want"]})
    if st.call == "m_opt":
        off, err = orc.m_opt(a["kp"], a["q"], a["initial_offsets"], a["is_regularized"], a["reg_coef"])
        return _freeze(dict(offsets=off, err=np.float32(err)))
    raise ValueError(st.call)


# ---- the pieces of a step that the model caches between calls, for the stale-state checks of test_call_sequence_host.py ----------
def state_pieces(model, st: Step):
    """{piece: value} of what the step makes the model hold: the rows of the state table a stale copy of which the oracle can restate."""
    a = st.args
    off = model.tables.site_pos if st.offsets is None else st.offsets
    if st.call == "q_phase":
        return dict(part_masks=np.asarray(a["part_masks"], np.uint8).reshape(-1, model.tables.nq), trunk_kps=np.asarray(a["trunk_kps"], np.uint8),
                    do_root_opt=bool(a["do_root_opt"]), solver=st.params.solver, offsets=off)
    if st.call == "q_solve":
        lb, ub = (model.lb, model.ub) if a["lb"] is None else (a["lb"], a["ub"])
        return dict(qs_to_opt=np.asarray(a["qs_to_opt"], np.uint8), kps_to_opt=np.asarray(a["kps_to_opt"], np.uint8),
                    box=np.stack([lb, ub]), offsets=off)
    return dict(offsets=off)


def with_piece(model, st: Step, piece, value):
    """The step with one piece replaced (what the kernels would compute from a stale copy of it)."""
    if piece == "offsets":
        return replace(st, offsets=value)
    if piece == "solver":
        return replace(st, params=replace(st.params, solver=value))
    if piece == "box":
        return replace(st, args={**st.args, "lb": value[0], "ub": value[1]})
    return replace(st, args={**st.args, piece: value})


def stale_variants(model, prev: Step, cur: Step):
    """[(label, step)]: `cur` with one cached piece left as `prev` had it, for every piece the transition changes.  Between calls of
    one entry point the pieces correspond one to one.  Between stac_q_phase and stac_q_solve the mask table changes its layout (tag
    0x5A / 0xA5), so a table that was not rewritten is read in the new layout: row 0 (the root pass's coordinates / qs_to_opt) and
    the keypoint weights (trunk_kps / kps_to_opt) are restated in the other call's terms."""
    if cur.refuse or prev.refuse:
        return []
    a, b = state_pieces(model, prev), state_pieces(model, cur)
    out = []
    if prev.call == cur.call:
        for k in b:
            if not np.array_equal(a[k], b[k]):
                out.append((k, with_piece(model, cur, k, a[k])))
        return out
    if not np.array_equal(a["offsets"], b["offsets"]):
        out.append(("offsets", with_piece(model, cur, "offsets", a["offsets"])))
    nq, K = model.tables.nq, model.tables.nsite
    if prev.call == "q_phase" and cur.call == "q_solve":
        row0 = (np.arange(nq) < prev.args["root_dims"]).astype(np.uint8) * (1 if a["do_root_opt"] else 0)
        out.append(("mask table (phase layout read as qs_to_opt)", with_piece(model, cur, "qs_to_opt", row0)))
        out.append(("mask table (trunk_kps read as kps_to_opt)", with_piece(model, cur, "kps_to_opt", np.repeat(a["trunk_kps"], 3))))
    elif prev.call == "q_solve" and cur.call == "q_phase":
        P = len(b["part_masks"])
        out.append(("mask table (qs_to_opt read as the part rows)", with_piece(model, cur, "part_masks", np.tile(a["qs_to_opt"], (P, 1)))))
        out.append(("mask table (kps_to_opt read as trunk_kps)", with_piece(model, cur, "trunk_kps", a["kps_to_opt"].reshape(K, 3).any(1).astype(np.uint8))))
        if b["solver"] != "pg":  # (stac_q_solve is always the projected gradient)
            out.append(("solver", with_piece(model, cur, "solver", "pg")))
    return out


# ---- builders -------------------------------------------------------------------------------------------------------------------
def _phase_args(m, kp, **over):
    d = dict(kp=kp, part_masks=m.part_masks, trunk_kps=m.trunk_kps, root_kp_idx=m.root_kp_idx, root_dims=m.root_dims, do_root_opt=True,
             q_init=None, want_bodies=True, want_markers=True)
    d.update(over)
    return d


def _lean16(got):
    return got[:2] == (16, 5) and got[3] == 1  # the lean 16-lane throughput kernel of the rodent (test_gpu_loop_head.py)


def _lean16_then_latency(got):
    return got[:2] == (16, 5) and got[3] == 5  # ... with the hand-off: the lean latency kernel (four roles) ran last


class _Script:
    def __init__(self, model):
        self.model, self.units, self.by_name = model, [], {}

    def add(self, *steps):
        for st in steps:
            if st.refuse is None and st.expect is None:
                st.expect = self.by_name[st.same_as].expect if st.same_as else expected(self.models(st), st)
            self.by_name[st.name] = st
        self.units.append(tuple(steps))
        return steps[-1]

    def models(self, st):
        return self.model[st.engine] if isinstance(self.model, dict) else self.model

    def steps(self):
        return [s for u in self.units for s in u]


def rodent_clips(mocap):
    """The nine three-frame clips of tests/test_gpu_loop_head.py."""
    return np.ascontiguousarray(np.stack([mocap[s:s + 3] for s in STARTS]).reshape(9, 3, 69))


def other_trunk(fs):
    """A trunk mask for which the root passes keep other bodies: without the shoulders and the front of the spine."""
    tk = np.array(fs.trunk_kps, bool)
    for n in ("ShoulderL", "ShoulderR", "SpineF"):
        tk[fs.kp_names.index(n)] = False
    return tk


def _tight_box(fs, w):
    lb, ub = np.maximum(fs.lb, -w).astype(np.float32), np.minimum(fs.ub, w).astype(np.float32)
    lb[:7], ub[:7] = fs.lb[:7], fs.ub[:7]
    return lb, ub


def _solve_args(fs, kp9, **over):
    kp = np.ascontiguousarray(kp9[:, 0])
    q0 = np.tile(fs.tables.qpos0, (len(kp), 1)).astype(np.float32)
    q0[:, :3] = kp[:, 3 * fs.root_kp_idx: 3 * fs.root_kp_idx + 3]
    boxA = _tight_box(fs, 0.2)
    d = dict(kp=kp, q0=q0, qs_to_opt=np.asarray(fs.part_masks[1], np.uint8), kps_to_opt=np.ones(69, np.uint8), lb=boxA[0], ub=boxA[1])
    d.update(over)
    return d


def script_a(fs, mocap):
    """Masks and boxes on the rodent: every step changes one thing against the step before it."""
    kp9 = rodent_clips(mocap)
    P0 = Params()
    lm = replace(P0, solver="lm")
    nq, K = fs.tables.nq, fs.tables.nsite
    s = _Script(fs)
    pruned = lambda v: v["n_mlev"] > 0 and v["fk3r"] > 0 and v["launch_root_fast"] == 7  # noqa: E731  (what the launch kept, after plan_q)
    a1 = s.add(Step("A1", "q_phase", _phase_args(fs, kp9), P0, kernel=_lean16, verbose=pruned))
    tk2 = other_trunk(fs)
    s.add(Step("A2", "q_phase", _phase_args(fs, kp9, trunk_kps=tk2), P0, kernel=_lean16, verbose=pruned))
    carry = a1.expect["carry_qpos"].copy()  # (the ORACLE's carry of step 1; a copy: expectations are read-only)
    warm = dict(trunk_kps=tk2, do_root_opt=False, q_init=carry)
    s.add(Step("A3", "q_phase", _phase_args(fs, kp9, **warm), P0, kernel=_lean16, verbose=lambda v: v["n_mlev"] == 0 and v["fk3r"] == 0))
    s.add(Step("A4", "q_phase", _phase_args(fs, kp9, part_masks=np.zeros((0, nq), bool), **warm), P0, kernel=_lean16))
    s.add(Step("A5", "q_phase", _phase_args(fs, kp9, part_masks=fs.part_masks[2:3], **warm), P0, kernel=_lean16))
    boxB = _tight_box(fs, 0.05)
    s.add(Step("A6", "q_solve", _solve_args(fs, kp9), P0))
    s.add(Step("A7", "q_solve", _solve_args(fs, kp9, lb=None, ub=None), P0))
    s.add(Step("A8", "q_solve", _solve_args(fs, kp9, lb=boxB[0], ub=boxB[1]), P0))
    s.add(Step("A9", "q_solve", _solve_args(fs, kp9), P0, same_as="A6"))
    s.add(Step("A10", "q_solve", _solve_args(fs, kp9, qs_to_opt=(np.arange(nq) < 7).astype(np.uint8), kps_to_opt=np.repeat(fs.trunk_kps, 3).astype(np.uint8)), P0))
    again = lambda name, **kw: Step(name, "q_phase", _phase_args(fs, kp9), kw.pop("params", P0), same_as="A1", kernel=kw.pop("kernel", _lean16), **kw)  # noqa: E731
    s.add(again("A11", verbose=pruned))
    s.add(Step("A12", "q_phase", _phase_args(fs, kp9), lm))
    s.add(Step("A13", "q_phase", _phase_args(fs, kp9, part_masks=np.zeros((0, nq), bool)), lm))
    s.add(Step("A14", "q_phase", _phase_args(fs, kp9), lm, same_as="A12"))
    s.add(again("A15"))
    off2 = (fs.tables.site_pos + np.random.default_rng(16).normal(0, 3e-3, (K, 3))).astype(np.float32)
    a16 = s.add(Step("A16a", "q_phase", _phase_args(fs, kp9), P0, offsets=off2, kernel=_lean16))
    poses = np.array(a16.expect["qpos"][:5, 0])
    s.add(Step("A16b", "fk", dict(qpos=poses, want=("site_xpos",)), P0, offsets=off2))
    s.add(Step("A16c", "m_opt", dict(kp=np.ascontiguousarray(kp9[:5, 0]), q=poses, initial_offsets=off2, is_regularized=fs.is_regularized, reg_coef=1.0),
               P0, offsets=off2))
    s.add(again("A16d"))
    s.add(again("A17a"))
    s.add(again("A17b", params=replace(P0, lanes_per_chain=32), kernel=lambda g: g[0] == 32))
    s.add(again("A17c", params=replace(P0, lanes_per_chain=0), kernel=lambda g: g[3] >= 2))  # (nine chains: the latency mode)
    big = np.zeros((38, nq), bool)  # P + 3 = 41 > kMaxKinds = 40
    big[:, 7] = True
    solveA = _solve_args(fs, kp9)
    refusals = [
        # (refused in run_q, AFTER stac_q_phase has uploaded and cached the mask table and rebuilt the root program: with another trunk than
        #  its neighbours, so that this refusal is a cache miss and its follower has to put step 1's table and program back)
        Step("A18a", "q_phase", _phase_args(fs, kp9, trunk_kps=tk2), replace(P0, maxiter=0), refuse="maxiter must be >= 1"),
        Step("A18b", "q_phase", _phase_args(fs, kp9, part_masks=big), P0, refuse="too many part groups"),
        Step("A18c", "q_phase", _phase_args(fs, kp9, root_kp_idx=K), P0, refuse="bad root optimisation arguments"),
        Step("A18d", "q_solve", _solve_args(fs, kp9, lb=solveA["ub"] + np.float32(1.0)), P0, refuse="lb > ub"),
    ]
    for r in refusals:
        s.add(r, again(r.name + "_then_A1"))
    return s


B_ENV = {"STAC_HIP_SPEC": "0", "STAC_HIP_QUEUE": "4", "STAC_HIP_WPB": "1", "STAC_HIP_HANDOFF": "4"}


def script_b(fs, mocap):
    """Behind the control word (engine created under B_ENV): the queue and the hand-off, armed and initialised per call on one d_ctl /
    d_hand.  With STAC_HIP_HANDOFF=4 in force the three-chain launch has no chain queue (fewer chains than slots) but keeps the
    hand-off, with a capacity of all its chains (min(4, 3): threshold 0) -- the control word is initialised for it all the same.  The
    call that plans NO control word between two that do is therefore B2s: a stac_q_solve (single mode: no queue, no hand-off, no
    launch_ctl_init), which finds d_ctl as B2 left it and leaves it to B3."""
    kp9 = rodent_clips(mocap)
    P0 = Params()
    s = _Script(fs)
    q_and_h = lambda v: v["queue"] == 4 and v["handoff"] == 4 and v["threshold"] == 5  # noqa: E731
    s.add(Step("B1", "q_phase", _phase_args(fs, kp9[:, :2]), P0, kernel=_lean16_then_latency, verbose=q_and_h))
    s.add(Step("B2", "q_phase", _phase_args(fs, kp9[:3]), P0, kernel=_lean16_then_latency,
               verbose=lambda v: v["queue"] == 0 and v["handoff"] == 3 and v["threshold"] == 0))
    s.add(Step("B2s", "q_solve", _solve_args(fs, kp9), P0))
    s.add(Step("B3", "q_phase", _phase_args(fs, kp9[:, :1]), P0, kernel=_lean16_then_latency, verbose=q_and_h))
    # (LM: one chain per wavefront, so that four slots of whole workgroups stay below the nine chains and its queue runs)
    s.add(Step("B4", "q_phase", _phase_args(fs, kp9[:, :2]), replace(P0, solver="lm", lanes_per_chain=64), verbose=lambda v: v["lm"] and 0 < v["queue"] < 9))
    s.add(Step("B5", "q_phase", _phase_args(fs, kp9[:, :2]), P0, same_as="B1", kernel=_lean16_then_latency, verbose=q_and_h))
    return s


C_MAXITER = 10
# 1024 chain slots for 2048 / 4096 chains: the launch has a chain queue, which hands the chains out through `perm` (plan_q keeps the
# order for a queue with root fast trips) -- at the issue's sizes no launch would read the order otherwise (placement by SIMD load
# needs more wavefronts than SIMDs).  No hand-off, so that every chain ends in the kernel that drew it from the queue.
C_ENV = {"STAC_HIP_QUEUE": "1024", "STAC_HIP_HANDOFF": "0"}


def small_model():
    """Free root and four hinges of their own bodies (11 coordinates), one site on each: a trunk of two sites leaves two bodies out of
    the root passes, so the root program is pruned and root fast trips are on."""
    t = _edge_tables(11, 4)
    lb, ub = _box(t)
    pm = np.zeros((1, t.nq), bool)
    pm[0, 7:9] = True
    return SimpleNamespace(tables=t, lb=lb, ub=ub, part_masks=pm, trunk_kps=np.array([1, 1, 0, 0], bool), root_kp_idx=0, root_dims=7)


def _targets(m, rng, n, noise=2e-3, spread=0.15):
    """n poses inside the box near the rest pose, and their marker sites with noise: (q [n, nq], kp [n, 3K])."""
    from oracle import Oracle

    t, orc = m.tables, Oracle(m.tables)
    q = np.tile(t.qpos0, (n, 1)) + rng.normal(0, spread, (n, t.nq)).astype(np.float32)
    q = np.clip(q, np.where(np.isfinite(m.lb), m.lb, -3), np.where(np.isfinite(m.ub), m.ub, 3)).astype(np.float32)
    kp = np.stack([orc.fk(x.copy())["site_xpos"].reshape(-1) for x in q]).astype(np.float32)
    return q, (kp + rng.normal(0, noise, kp.shape)).astype(np.float32)


def script_c():
    """Growth and reuse: the chain-order work space (C >= 2048 chains, no q_init), stand-alone kinematics and the q_phase's own at
    changing sizes.  Engine created under C_ENV, 16 lanes per chain (the throughput kernel at every size)."""
    m = small_model()
    rng = np.random.default_rng(33)
    P0 = Params(tol=1e-4, maxiter=C_MAXITER, lanes_per_chain=16)
    K = m.tables.nsite
    q, kp = _targets(m, rng, 4096)
    kp = kp.reshape(4096, 1, 3 * K)
    _, kpf = _targets(m, rng, 64 * 8)
    kpf = kpf.reshape(64, 8, 3 * K)
    s = _Script(m)
    lite = dict(want_bodies=False)
    fast = lambda v: v["n_mlev"] > 0 and v["launch_root_fast"] == 7  # noqa: E731  (a pruned root program; the LAUNCH runs root fast trips)
    queued = lambda v: fast(v) and 1024 <= v["queue"] < 2048  # noqa: E731
    c1 = s.add(Step("C1", "q_phase", _phase_args(m, kp[:2048], **lite), P0, order=True, reads_order=True, verbose=queued))
    s.add(Step("C2", "q_phase", _phase_args(m, kp, **lite), P0, order=True, reads_order=True, verbose=queued))
    s.add(Step("C3", "q_phase", _phase_args(m, kp[:2048], **lite), P0, order=True, reads_order=True, same_as="C1", verbose=queued))
    s.add(Step("C4", "q_phase", _phase_args(m, kp[:5], **lite), P0, verbose=fast))
    s.add(Step("C5", "q_phase", _phase_args(m, kp[:2048], q_init=c1.expect["carry_qpos"].copy(), **lite), P0,
               verbose=lambda v: 1024 <= v["queue"] < 2048))  # (the queue without an order: chains in their own order)
    for i, n in enumerate((1, 4096, 3)):
        s.add(Step(f"C6{'abc'[i]}", "fk", dict(qpos=np.ascontiguousarray(q[:n]), want=("site_xpos",)), P0))
    for i, (c, f) in enumerate(((5, 2), (64, 8), (5, 2))):
        s.add(Step(f"C7{'abc'[i]}", "q_phase", _phase_args(m, np.ascontiguousarray(kpf[:c, :f]), **lite), P0, same_as="C7a" if i == 2 else None))
    return s


def ball_model():
    """The random tree with ball, slide and hinge joints of test_oracle.py::_ball_case(0, free_root=True): the generic kernels, and the
    LM solver with ball joints."""
    rng = np.random.default_rng(0)
    t = _random_tables(rng, 24, True, p_slide=0.15, p_ball=0.3)
    lb, ub = _box(t)
    part = (rng.random((2, t.nq)) < 0.4).astype(np.uint8)
    trunk = (rng.random(t.nsite) < 0.6).astype(np.uint8)
    trunk[0] = 1
    return SimpleNamespace(tables=t, lb=lb, ub=ub, part_masks=part, trunk_kps=trunk, root_kp_idx=0, root_dims=7), rng


def script_d(fs, mocap):
    """Two models alive: steps 1, 6 and 12 of script A on the rodent, interleaved with the same three kinds of call on another model."""
    kp9 = rodent_clips(mocap)
    x, rng = ball_model()
    P0 = Params()
    PX = Params(tol=1e-4, maxiter=15, lanes_per_chain=0, lm_maxiter=15)
    nq, K = x.tables.nq, x.tables.nsite
    qx, kpx = _targets(x, rng, 18, noise=1e-3)
    kpx = kpx.reshape(9, 2, 3 * K)
    fin = np.isfinite(x.lb) & np.isfinite(x.ub)
    lb2, ub2 = x.lb.copy(), x.ub.copy()
    lb2[fin], ub2[fin] = x.lb[fin] * 0.5, x.ub[fin] * 0.5
    q0 = np.clip(qx[:9], np.where(np.isfinite(lb2), lb2, -3), np.where(np.isfinite(ub2), ub2, 3)).astype(np.float32)
    xsolve = dict(kp=np.ascontiguousarray(kpx[:, 0]), q0=q0, qs_to_opt=(rng.random(nq) < 0.6).astype(np.uint8),
                  kps_to_opt=(rng.random(3 * K) < 0.8).astype(np.uint8), lb=lb2, ub=ub2)
    s = _Script({"main": fs, "other": x})
    s.add(Step("D1", "q_phase", _phase_args(fs, kp9), P0, kernel=_lean16))
    s.add(Step("D1x", "q_phase", _phase_args(x, kpx), PX, engine="other"))
    s.add(Step("D6", "q_solve", _solve_args(fs, kp9), P0))
    s.add(Step("D6x", "q_solve", xsolve, PX, engine="other"))
    s.add(Step("D12", "q_phase", _phase_args(fs, kp9), replace(P0, solver="lm")))
    s.add(Step("D12x", "q_phase", _phase_args(x, kpx), replace(PX, solver="lm"), engine="other"))
    return s


_BUILT = {}


def build_all(fs, mocap):
    """{"A" .. "D": script}, built once per process and read-only from then on; ["seconds"] is the wall time of building them."""
    if not _BUILT:
        t0 = time.perf_counter()
        _BUILT.update(A=script_a(fs, mocap), B=script_b(fs, mocap), C=script_c(), D=script_d(fs, mocap))
        _BUILT["seconds"] = time.perf_counter() - t0
    return _BUILT
