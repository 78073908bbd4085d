"""CPU (`-m "not gpu"`): chain_plan.plan_chain — which chain of launches a shape gets and every count Learner allocates by — against
tests/golden/chain_plan.json, the table tests/golden/make_chain_plan.py recorded from Learner's constructor before the plan was
taken out of it (the script's docstring has the format)."""
import dataclasses
import json
import os

import pytest
import torch

from conftest import GOLDEN

from robotic_manipulator_rloa_amd.chain_plan import ChainPlan, plan_chain

# a column of the table -> the field of ChainPlan it records, where the two are not named alike (None: checked by hand below)
FIELD = {"warnings": None, "error": None, "partials_numel": None}


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(GOLDEN, "chain_plan.json")) as f:
        return json.load(f)


def plan_of(table, case, **more):
    """plan_chain for a row of the table's cases; the switches the row's variant sets go in as `env`, never into os.environ"""
    S, A, H, B, p_mode, variant = case[:6]
    kw = dict(table["variants"][variant])
    env = kw.pop("env", {})
    for arg in ("_fold_norm", "_force_allreduce"):
        if arg in kw:
            kw[arg[1:]] = kw.pop(arg)
    return plan_chain(S, A, H, B, p_mode=p_mode, env=env, **kw, **more)


def test_plan_chain_reproduces_the_recorded_constructor(table):
    names = {f.name for f in dataclasses.fields(ChainPlan)}
    groups = list(table["columns"])
    # (the full product alone is 5 x 5 x 5 x 13 x 2 = 3250 cases)
    assert table["case_columns"] == ["S", "A", "H", "B", "p_mode", "variant"] + groups and len(table["cases"]) > 3250
    checked = set()
    for case in table["cases"]:
        want = {}
        for g, i in zip(groups, case[6:]):
            want.update(zip(table["columns"][g], table[g][i]))
        S, A, H, B = case[:4]
        if want["error"] is not None:
            with pytest.raises(ValueError) as e:
                plan_of(table, case)
            assert str(e.value) == want["error"], case
            continue
        plan = plan_of(table, case)
        for col, value in want.items():
            field = FIELD.get(col, col)
            if field is None:
                continue
            assert field in names, field
            got = getattr(plan, field)
            assert (",".join(sorted(got)) if field == "fuse" else got) == value, (case, col, got, value)
            checked.add(field)
        assert [w.format(S=S, A=A, H=H, B=B) for w in want["warnings"]] == ([plan.warning] if plan.warning else []), case
        # (the buffer of norm partials: room for the most any form of the exchange leaves, + the step count's word)
        assert want["partials_numel"] == max(plan.n_partials_fold + 1, plan.n_partials_norm, plan.n_partials) + 1, case
        assert isinstance(plan.fuse, frozenset) and plan.Bp >= B and (plan.hk_rows is None) == ("bb" not in plan.fuse)
    # what no attribute of the old constructor showed is pinned on the device (test_learner_gpu.py: buffer shapes by the plan)
    assert names - checked == {"warning", "nb", "kp", "act_fused"}, names - checked


def test_world_size_rule(table):
    """Beyond one rank: no folded norm, the norm launch's partial count, and the optimizer step rides wherever the row-split chain
    runs and NAF_DEFER_ADAM does not say 0 — nothing else of the plan changes."""
    for case in table["cases"]:
        if table["choice"][case[6]][-1] is not None:      # (an error row)
            continue
        one, two = plan_of(table, case), plan_of(table, case, world_size=2)
        env = table["variants"][case[5]].get("env", {})
        assert two == dataclasses.replace(one, fold_norm=False, n_partials=one.n_partials_norm,
                                          defer_ok="bb" in one.fuse and env.get("NAF_DEFER_ADAM", "1") != "0"), case


def test_plan_chain_is_deterministic_and_reads_only_its_env(table, monkeypatch):
    monkeypatch.setenv("NAF_FUSE", "unfused")
    monkeypatch.setenv("NAF_DEFER_ADAM", "0")
    for case in table["cases"][::97]:
        if table["choice"][case[6]][-1] is None:
            assert plan_of(table, case) == plan_of(table, case)      # (env = the row's own mapping: os.environ is not looked at)
    assert plan_chain(21, 6, 256, 256).chain == "unfused" and not plan_chain(23, 7, 256, 2048, fuse="rows").defer_ok
    assert plan_chain(21, 6, 256, 256, fuse="rows").chain == "rows"       # the argument wins over NAF_FUSE


def test_plan_chain_needs_no_gpu(monkeypatch):
    """No tensor, no require_gpu(), no HIP call: the plan comes out where torch sees no GPU and where asking for one would raise."""
    from robotic_manipulator_rloa_amd import _lib
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_lib, "require_gpu", lambda: pytest.fail("plan_chain called require_gpu()"))
    monkeypatch.setattr(torch, "zeros", lambda *a, **k: pytest.fail("plan_chain allocated a tensor"))
    monkeypatch.setattr(torch, "empty", lambda *a, **k: pytest.fail("plan_chain allocated a tensor"))
    plan = plan_chain(23, 7, 256, 2048, env={})
    assert (plan.chain, plan.Bp, plan.ks_w2, plan.ks_wh, plan.keep_xhat1, plan.n_partials) == ("rows", 2048, 4, 8, False, 205)
    assert not torch.cuda.is_available()
