"""One long-lived model through changing call sequences, every call held to the stateless oracle (tests/call_sequence_cases.py).

`stac_q_solve`, `stac_q_phase`, `stac_fk` and `stac_set_site_pos` keep host-side state on a `stac_model` between calls and decide from
it what to upload, what to rebuild and which launch to plan ("What a model carries between calls").  Each script runs on
ONE engine (script D: two, alive together) in order with every q_phase output pre-filled with a pattern, in reversed order on a fresh
engine, and as a whole under one side stream with no host synchronisation between the calls beyond what the entry points do
themselves.  After every step the comparison is the one the existing test of that entry point makes (tests/test_gpu_parity.py):
tolerance 0.  Which launch a step ended on is read from `stac_debug_last_q_kernel` and from the plan lines of an engine created with
STAC_HIP_VERBOSE.
"""

import contextlib
import re

import numpy as np
import pytest

import call_sequence_cases as cs
from test_gpu_loop_head import _last_q_kernel
from test_gpu_parity import _compare_phase, _np

pytestmark = pytest.mark.gpu

FILL_F32, FILL_I32 = 0x7FA5A5A5, -0x5A5A5A5B  # a NaN and 0xA5A5A5A5: an element a call does not write fails its comparison
ENV = {"A": {}, "B": cs.B_ENV, "C": cs.C_ENV, "D": {}}


@pytest.fixture(scope="module")
def scripts(rodent_setup, rodent_mocap):
    return cs.build_all(rodent_setup, rodent_mocap)


def _engines(monkeypatch, script, name):
    from stac_mjx_amd.engine import Engine

    for k, v in {"STAC_HIP_VERBOSE": "1", **ENV[name]}.items():
        monkeypatch.setenv(k, v)  # (read once, when the engine creates its model)
    engs = {}
    for st in script.steps():
        if st.engine not in engs:
            m, p = script.models(st), st.params
            engs[st.engine] = Engine(m.tables, m.lb, m.ub, tol=p.tol, maxiter=p.maxiter, maxls=p.maxls, lanes_per_chain=p.lanes_per_chain)
    return engs


def _plan_fields(err):
    """The numbers of a call's last plan lines: "[stac] q_phase: root program ..." and the launch plan of plan_q / plan_q_lm."""
    v = {"lm": False}
    lines = [ln for ln in err.splitlines() if ln.startswith("[stac] q_phase")]
    root = [ln for ln in lines if "root program" in ln]
    plan = [ln for ln in lines if " chains=" in ln]
    for ln in root[-1:] + plan[-1:]:
        v.update({k: int(x) for k, x in re.findall(r"(\w+)=(-?\d+)\b", ln)})
    v["lm"] = bool(plan) and plan[-1].startswith("[stac] q_phase LM")
    return v


def _prefilled(eng, a):
    import torch

    C, F = a["kp"].shape[:2]
    f = lambda *s: torch.full(s, FILL_F32, dtype=torch.int32, device=eng.device).view(torch.float32)  # noqa: E731
    out = dict(qpos=f(C, F, eng.nq), frame_error=f(C, F), counters=torch.full((C, F, 4), FILL_I32, dtype=torch.int32, device=eng.device),
               carry_qpos=f(C, eng.nq), marker_sites=f(C, F, eng.K, 3))
    if a["want_bodies"]:
        out.update(xpos=f(C, F, eng.nbody, 3), xquat=f(C, F, eng.nbody, 4))
    return out


def _call(eng, st, fill):
    a = st.args
    if st.call == "q_phase":
        return eng.q_phase(a["kp"], part_masks=a["part_masks"], trunk_kps=a["trunk_kps"], root_kp_idx=a["root_kp_idx"], root_dims=a["root_dims"],
                           do_root_opt=a["do_root_opt"], q_init=a["q_init"], want_bodies=a["want_bodies"], want_markers=a["want_markers"],
                           out=_prefilled(eng, a) if fill else None)
    if st.call == "q_solve":
        return eng.q_solve(a["kp"], a["q0"], a["qs_to_opt"], a["kps_to_opt"], lb=a["lb"], ub=a["ub"])
    if st.call == "fk":
        return eng.fk(a["qpos"], want=a["want"])
    return eng.m_opt(a["kp"], a["q"], a["initial_offsets"], a["is_regularized"], a["reg_coef"])


def _compare(st, res):
    ref = st.expect
    if st.call == "q_phase":
        _compare_phase(res, ref, bodies=st.args["want_bodies"])
        np.testing.assert_array_equal(_np(res["carry_qpos"]), ref["carry_qpos"], err_msg=st.name)
    elif st.call == "q_solve":
        params, state, counters = (_np(x) for x in res)
        assert counters.tolist() == ref["counters"].tolist(), st.name
        np.testing.assert_array_equal(params, ref["qpos"], err_msg=st.name)
        np.testing.assert_array_equal(state, ref["state"], err_msg=st.name)
    elif st.call == "fk":
        for k in ("qpos", "xpos", "xquat", "site_xpos"):
            if k in st.args["want"]:
                np.testing.assert_array_equal(_np(res[k]), ref[k], err_msg=f"{st.name} {k}")
            else:
                assert res[k] is None
    else:
        off, err = res
        np.testing.assert_array_equal(_np(off), ref["offsets"], err_msg=st.name)
        assert float(err) == ref["err"], st.name


def _run(script, engs, capfd, units, *, fill=False, streams=None, compare_at_once=True):
    """Runs the units in the order given; returns [(step, result)] of what is still to compare and {step name: plan fields}."""
    import torch
    from stac_mjx_amd.engine import StacHipError

    offsets = {e: script.models(st).tables.site_pos for st in script.steps() for e in [st.engine]}
    high_water = dict.fromkeys(engs, 0)
    pending, fields = [], {}
    for st in (s for u in units for s in u):
        eng, model = engs[st.engine], script.models(st)
        with torch.cuda.stream(streams[st.engine]) if streams else contextlib.nullcontext():
            want = model.tables.site_pos if st.offsets is None else st.offsets
            if not np.array_equal(want, offsets[st.engine]):
                eng.set_site_pos(want)
                offsets[st.engine] = want
            cs.apply_params(eng, st.params)
            capfd.readouterr()
            if st.refuse:
                with pytest.raises(StacHipError, match=st.refuse):
                    _call(eng, st, fill)
                assert " chains=" not in capfd.readouterr().err, st.name  # refused before a launch was planned
                continue
            res = _call(eng, st, fill)
        if st.call == "q_phase":
            v = fields[st.name] = _plan_fields(capfd.readouterr().err)
            if st.params.solver == "pg":
                got = _last_q_kernel(eng)
                assert st.kernel is None or st.kernel(got), (st.name, got)
                if st.order:
                    high_water[st.engine] = max(high_water[st.engine], len(st.args["kp"]))
                assert (v["chain_order"], v["order_chains"]) == (int(st.order), high_water[st.engine]), (st.name, v)
                # what the launch kept of the request after plan_q (the latency mode's plan line has no such field: it keeps no order)
                assert v.get("keep_perm", 0) == int(st.reads_order) and v.get("keep_place", 0) == 0, (st.name, v)
            assert v["lm"] == (st.params.solver == "lm"), (st.name, v)
            assert st.verbose is None or st.verbose(v), (st.name, v)
        if compare_at_once:
            _compare(st, res)
        else:
            pending.append((st, res))
    return pending, fields


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_script_in_order_with_outputs_prefilled(scripts, monkeypatch, capfd, name):
    script = scripts[name]
    engs = _engines(monkeypatch, script, name)
    _, v = _run(script, engs, capfd, script.units, fill=True)
    if name == "A":  # the pruned programs of steps 1 and 2 are different ones, and step 11 rebuilt step 1's
        assert (v["A1"]["n_mlev"], v["A1"]["fk3r"]) != (v["A2"]["n_mlev"], v["A2"]["fk3r"]), (v["A1"], v["A2"])
        assert (v["A11"]["n_mlev"], v["A11"]["fk3r"]) == (v["A1"]["n_mlev"], v["A1"]["fk3r"])


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_script_reversed(scripts, monkeypatch, capfd, name):
    """Last unit first on a fresh engine; a refusal keeps the step that follows it."""
    script = scripts[name]
    _run(script, _engines(monkeypatch, script, name), capfd, script.units[::-1])


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_script_on_a_side_stream(scripts, monkeypatch, capfd, name):
    """The whole script under one side stream per engine: the mask, box, LM-table and root-program uploads are asynchronous copies
    from host temporaries behind kernels that may still run.  Outputs are kept alive and compared after one synchronisation."""
    import torch

    script = scripts[name]
    engs = _engines(monkeypatch, script, name)
    streams = {e: torch.cuda.Stream() for e in engs}
    torch.cuda.synchronize()  # (the engines were created on the default stream)
    pending, _ = _run(script, engs, capfd, script.units, streams=streams, compare_at_once=False)
    for s in streams.values():
        s.synchronize()
    assert pending
    for st, res in pending:
        _compare(st, res)
