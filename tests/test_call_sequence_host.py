"""The call-sequence scripts of tests/call_sequence_cases.py can fail: on the oracle alone (no GPU), every transition of scripts A, B
and D that changes something the model caches between calls is shown to be stale-sensitive -- the new step computed with that one
piece left at the previous step's value differs in bits from the step's expectation -- and every expectation is a real solve
(finite, LM converged somewhere, PG iterated, step 8 on its box, step 2 with another root result).

What the oracle cannot restate is not shown here: the control word and the hand-off buffer (script B's changes of chain and frame
counts), the chain-order work space and the sizes of script C.  A stale copy of those has no stateless meaning; the GPU test
compares every step of those scripts with its expectation all the same.
"""

import numpy as np
import pytest

import call_sequence_cases as cs

SOLVER_CALLS = ("q_phase", "q_solve")
MAIN_OUTPUT = {"q_phase": "qpos", "q_solve": "qpos", "fk": "site_xpos", "m_opt": "offsets"}


@pytest.fixture(scope="module")
def scripts(rodent_setup, rodent_mocap):
    return cs.build_all(rodent_setup, rodent_mocap)


def _transitions(script):
    """[(prev, cur)] per engine: a solver call against the solver call before it (the mask table, the box, the LM tables and the
    offsets in the plan blob are theirs alone), a stand-alone FK against the FK before it or the model as it was created (the
    `d_site_pos` mirror of the offsets).  The offset phase reads no cached piece (its offsets are arguments)."""
    from dataclasses import replace

    out, last = [], {}
    for st in script.steps():
        if st.refuse or st.call == "m_opt":
            continue
        kind = "solver" if st.call in SOLVER_CALLS else st.call
        prev = last.get((st.engine, kind))
        if prev is None and st.call == "fk":
            prev = replace(st, name="(the model as created)", offsets=None)
        if prev is not None:
            out.append((prev, st))
        last[(st.engine, kind)] = st
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_every_state_changing_transition_is_stale_sensitive(scripts, name):
    script = scripts[name]
    checked, rows = 0, set()
    for prev, cur in _transitions(script):
        model = script.models(cur)
        a, b = cs.state_pieces(model, prev), cs.state_pieces(model, cur)
        changed = prev.call != cur.call and cur.call in SOLVER_CALLS or any(not np.array_equal(a[k], b[k]) for k in b if k in a)
        # (a restated piece may come out equal to the step's own -- A10 -> A11: kps_to_opt read as trunk_kps IS step 11's trunk --, where a
        #  stale copy cannot matter: such a variant is no evidence and is left out; the assertion below holds that every transition
        #  which changes the state keeps at least one variant that does differ, so no transition is skipped)
        variants = [(lab, v) for lab, v in cs.stale_variants(model, prev, cur)
                    if any(not np.array_equal(x, y) for x, y in zip(cs.state_pieces(model, v).values(), b.values()))]
        if not changed:
            assert not variants
            continue
        assert variants, f"{prev.name} -> {cur.name} changes the model's state but no stale variant of it differs from the step itself"
        key = MAIN_OUTPUT[cur.call]
        for label, v in variants:
            stale = cs.expected(model, v)[key]
            assert not np.array_equal(_bits(stale), _bits(cur.expect[key])), f"{prev.name} -> {cur.name}: stale {label} gives the same {key}"
            rows.add(label.split(" (")[0])
            checked += 1
    assert checked >= {"A": 18, "B": 5, "D": 8}[name], checked
    if name == "A":  # every kind of cached piece is crossed at least once
        assert rows >= {"part_masks", "trunk_kps", "do_root_opt", "solver", "offsets", "box", "qs_to_opt", "mask table"}, rows


def test_expectations_are_finite_and_real_solves(scripts):
    for name in "ABCD":
        for st in scripts[name].steps():
            if st.refuse:
                assert st.expect is None
                continue
            for k, v in st.expect.items():
                if v is not None:
                    assert np.isfinite(np.asarray(v, np.float64)).all(), (st.name, k)
                    assert not np.asarray(v).flags.writeable or np.asarray(v).ndim == 0, (st.name, k)
            if st.same_as:
                assert st.expect is scripts[name].by_name[st.same_as].expect
            if st.call == "q_phase" and st.params.solver == "lm":
                assert (st.expect["frame_error"] <= st.params.tol).any(), st.name  # the LM solver converged on some frame
            elif st.call in SOLVER_CALLS:
                assert (st.expect["counters"][..., 0] > 3).any(), st.name  # the projected gradient iterated


def test_step_8_lies_on_its_box_and_off_the_models(scripts, rodent_setup):
    fs, st = rodent_setup, scripts["A"].by_name["A8"]
    m = st.args["qs_to_opt"].astype(bool)
    x, lb, ub = st.expect["qpos"][:, m], st.args["lb"][m], st.args["ub"][m]
    on_b = (x == lb) | (x == ub)
    on_model = (x == fs.lb[m]) | (x == fs.ub[m])
    assert (on_b & ~on_model).any()
    a6 = scripts["A"].by_name["A6"]  # box A binds too (else step 7 could not tell it from the model's)
    xa = a6.expect["qpos"][:, m]
    assert (((xa == a6.args["lb"][m]) | (xa == a6.args["ub"][m])) & ~((xa == fs.lb[m]) | (xa == fs.ub[m]))).any()


def test_step_2_keeps_other_bodies_and_moves_the_root_solve(scripts, rodent_setup):
    from oracle import Oracle

    fs, t = rodent_setup, rodent_setup.tables
    a1, a2 = scripts["A"].by_name["A1"], scripts["A"].by_name["A2"]

    def kept(trunk):  # the bodies a root pass needs: the ancestors-or-self of the bodies that carry a weighted site
        need = set()
        for b in t.site_bodyid[np.asarray(trunk, bool)]:
            while b > 0:
                need.add(int(b))
                b = t.body_parentid[b]
        return need

    k1, k2 = kept(a1.args["trunk_kps"]), kept(a2.args["trunk_kps"])
    assert k2 < k1 and 0 < len(k2), (sorted(k1 - k2), len(k2))
    orc = Oracle(t, tol=a1.params.tol, maxiter=a1.params.maxiter)
    for c in range(9):
        r1, _ = orc.root_optimization(a1.args["kp"][c], t.qpos0, fs.lb, fs.ub, a1.args["trunk_kps"], fs.root_kp_idx, fs.root_dims)
        r2, _ = orc.root_optimization(a2.args["kp"][c], t.qpos0, fs.lb, fs.ub, a2.args["trunk_kps"], fs.root_kp_idx, fs.root_dims)
        assert not np.array_equal(r1[:7], r2[:7]), c
    assert not np.array_equal(a1.expect["qpos"], a2.expect["qpos"])


def test_script_c_prunes_its_root_passes():
    m = cs.small_model()
    t = m.tables
    need = set()
    for b in t.site_bodyid[m.trunk_kps]:
        while b > 0:
            need.add(int(b))
            b = t.body_parentid[b]
    assert 0 < len(need) < t.nbody - 1  # (bodies are left out: a pruned root program, root fast trips)
    assert t.nq == 11 and t.nsite == 4 and t.jnt_type[0] == 0  # a free root at qpos 0 .. 6


def test_expectations_are_affordable(scripts):
    """The oracle work of the whole module: measured 1.8 s and 4.4 s on two machines (see call_sequence_cases.py); the bound leaves room for a machine with a
    tenth of the threads and stays far below what a test session should spend on setting up."""
    print(f"call-sequence expectations built in {scripts['seconds']:.2f} s")
    assert scripts["seconds"] < 60.0
