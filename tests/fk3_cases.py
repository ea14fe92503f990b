"""Shared by tests/test_fk3_rounds_host.py and tests/test_gpu_fk3_rounds.py: the split-kinematics program of a model as the host
builds it (stac_debug_fk3_program: plan construction only, no device), and searches for random lean models -- free root, hinges only,
some with oriented bodies -- whose programs have a wanted number of rotations or whose plans have a wanted number of site ranges."""

from __future__ import annotations

import ctypes as C
import functools

import numpy as np

INFO = ("fk3", "n1", "n2", "n3", "nrot", "cap2", "noop_quat_word", "sink_word", "nrange", "rsplit", "nab", "nneed")


def lean_box(t):
    """The box of the random-model tests: unit-quaternion components in [-1, 1], hinges in their range (widened to hold 0)."""
    from stac_mjx_amd.mjcf import JNT_FREE

    lb, ub = np.full(t.nq, -np.inf, np.float32), np.full(t.nq, np.inf, np.float32)
    for j in range(t.njnt):
        a, ty = int(t.jnt_qposadr[j]), int(t.jnt_type[j])
        if ty == JNT_FREE:
            lb[a + 3:a + 7], ub[a + 3:a + 7] = -1, 1
        else:
            lb[a], ub[a] = min(t.jnt_range[j, 0], 0.0), t.jnt_range[j, 1]
    return lb, ub


def fk3_program(tables, lb, ub, trunk=None):
    """-> (info dict, T2 as uint32 [cap2, 4]) of the full program (trunk None) or of the root passes' pruned program."""
    from stac_mjx_amd.engine import StacModelTables, _f32p, _i32p, load_library

    lib = load_library()
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
    fn = lib.stac_debug_fk3_program
    fn.restype = C.c_int32
    fn.argtypes = [C.POINTER(StacModelTables), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    info = np.zeros(12, np.int32)
    cap = 4096
    t2 = np.zeros((cap, 4), np.uint32)
    tk = None if trunk is None else np.ascontiguousarray(trunk, dtype=np.uint8)
    rc = fn(C.byref(t), None if tk is None else tk.ctypes.data, info.ctypes.data, t2.ctypes.data, cap)
    assert rc == 0, lib.stac_last_error().decode()
    d = dict(zip(INFO, (int(x) for x in info)))
    return d, t2[:d["cap2"]].copy()


def _random_lean(seed, p_oriented):
    from test_gpu_parity import _random_tables

    rng = np.random.default_rng(770000 + seed)
    nbody = int(rng.integers(12, 64))
    t = _random_tables(rng, nbody, True, p_slide=0.0, p_ball=0.0, max_children_bias=float(rng.choice([0.3, 0.6, 0.9])), lean=True,
                       k_max=int(rng.choice([8, 12, 24])), p_oriented=p_oriented)
    return t, rng


@functools.lru_cache(maxsize=None)
def model_with_rotations(residue, oriented, min_rot=33):
    """The first random lean model (of at most 80 coordinates: the narrow lean shapes) whose full program has `residue` rotations mod 32
    (at least min_rot: the paired rounds of P2 run as well as its single one) and a choice of trunk keypoints whose pruned root program
    has a rotation count of another residue class.  -> (tables, lb, ub, trunk, full info, pruned info)"""
    for seed in range(4000):
        t, rng = _random_lean(seed, 0.3 if oriented else None)
        if not 8 <= t.nq <= 80:
            continue
        lb, ub = lean_box(t)
        full, _ = fk3_program(t, lb, ub)
        if not full["fk3"] or full["nrot"] < min_rot or full["nrot"] % 32 != residue:
            continue
        for _ in range(8):
            trunk = (rng.random(t.nsite) < 0.4).astype(np.uint8)
            trunk[int(rng.integers(t.nsite))] = 1
            root, _ = fk3_program(t, lb, ub, trunk)
            if 0 < root["nneed"] < root["nab"] and root["n3"] > 0 and root["nrot"] % 32 != residue:
                return t, lb, ub, trunk, full, root
    raise AssertionError(f"no random lean model with {residue} rotations mod 32")


@functools.lru_cache(maxsize=None)
def model_with_ranges(nrange):
    """The first random lean model of at most 80 coordinates whose plan has `nrange` distinct site ranges."""
    for seed in range(4000):
        t, rng = _random_lean(10000 + seed, None)
        if not 8 <= t.nq <= 80:
            continue
        lb, ub = lean_box(t)
        info, _ = fk3_program(t, lb, ub)
        if info["fk3"] and info["nrange"] == nrange:
            trunk = (rng.random(t.nsite) < 0.6).astype(np.uint8)
            trunk[0] = 1
            return t, lb, ub, trunk, info
    raise AssertionError(f"no random lean model with {nrange} site ranges")
