"""CPU: which TransR descriptors the step plan accepts, and the workspace size
and plan signature of those it does, against values recorded from the build
whose gate was still the retired one-per-CU kernel's LDS carve
(tests/golden/transr_plan.json, tests/golden/make_transr_plan_golden.py)."""

import ctypes
import json
import os

from tests.golden import make_transr_plan_golden as gen

KGE_ENOMEM_WORKSPACE, KGE_EUNSUPPORTED = 4, 5


def test_transr_plan_grid_matches_recorded(hiplib):
    with open(gen.OUT) as f:
        gold = json.load(f)
    assert (tuple(gold["dims"]), tuple(gold["negative_ratios"]), tuple(gold["sides"])) == (gen.DIMS, gen.NEGS, gen.SIDES)
    assert (gold["entities"], gold["relations"], gold["batch"]) == (gen.ENTITIES, gen.RELATIONS, gen.BATCH)
    cases = list(gen.cases())
    assert len(cases) == len(gold["rows"]) == 12 * 12 * 14 * 2
    bad = []
    accepted = 0
    for case, want in zip(cases, gold["rows"]):
        got = gen.probe(hiplib, *case)
        status, ws, sig = got
        # accepted <=> a workspace size, a signature, and only the 16-byte workspace refused
        assert (ws > 0) == (sig != 0) == (status == KGE_ENOMEM_WORKSPACE), (case, got)
        accepted += ws > 0
        if got != want:
            bad.append((case, got, want))
    assert not bad, "%d of %d cases differ, first: %r" % (len(bad), len(cases), bad[:5])
    assert 0 < accepted < len(cases)


def test_big_dim_refusal_names_the_negative_ratio_limit(hiplib):
    for side, neg, ok in (("t", 62, True), ("t", 63, False), ("h+t", 63, True), ("h+t", 64, False)):
        d, _keep = gen.desc(256, 256, neg, side)
        status = hiplib.kge_step(ctypes.byref(d), None)
        assert status == (KGE_ENOMEM_WORKSPACE if ok else KGE_EUNSUPPORTED), (side, neg, status)
        if not ok:
            msg = hiplib.kge_last_error().decode()
            assert "negative_ratio <= 62" in msg and "208" in msg, msg
            assert "LDS" not in msg and "bytes" not in msg, msg
    # sizes up to 208 take every negative ratio the slot limit admits
    d, _keep = gen.desc(208, 208, 71, "t")
    assert hiplib.kge_step(ctypes.byref(d), None) == KGE_ENOMEM_WORKSPACE
