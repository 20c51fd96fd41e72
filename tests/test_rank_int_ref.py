"""CPU: the integer ranking reference (tests/rank_int_ref.py) that
test_gpu_rank_exact.py holds kge_rank to, pinned against the float64 oracle's
get_rank restatement (oracle.filtered_ranks) on the same integer weights; and
the oracle's near-tie count, which bounds what the model-level rank tests
forgive."""

import numpy as np
import pytest

from oracle import kge_oracle as orc
from tests import rank_int_ref as ref

E, R, N = 65, 3, 9
KIND_SCORE = {"p1": ("lp", 1.0), "p2": ("lp", 2.0), "pinf": ("lp", float("inf")), "pow2": ("lppow", 2.0),
              "dot": ("dot", 0.0)}


def _ints(rng, *shape):
    return rng.integers(-2, 3, shape).astype(np.float64)


def _weights(name, rng):
    if name == "TransE":
        return {"ent_emb": _ints(rng, E, 17), "rel_emb": _ints(rng, R, 17)}
    if name == "TransH":
        return {"ent_emb": _ints(rng, E, 17), "rel_emb": _ints(rng, R, 17), "rel_hyper": _ints(rng, R, 17)}
    if name in ("TransD-12-20", "TransD-20-12"):
        ke, kr = (12, 20) if name == "TransD-12-20" else (20, 12)
        return {"ent_emb": _ints(rng, E, ke), "rel_emb": _ints(rng, R, kr), "ent_proj": _ints(rng, E, ke),
                "rel_proj": _ints(rng, R, kr)}
    if name == "DistMult":
        return {"ent_emb": _ints(rng, E, 17), "rel_inter": _ints(rng, R, 17)}
    if name == "RESCAL":
        return {"ent_emb": _ints(rng, E, 5), "rel_inter": _ints(rng, R, 5, 5)}
    if name == "RotatE":   # a wider value range: fewer exact ties for cos / sin rounding to break
        return {"ent_emb": rng.integers(-9, 10, (E, 16, 2)).astype(np.float64),
                "rot": rng.integers(0, 4, (R, 16)).astype(np.float64)}
    raise ValueError(name)


def _triples(rng):
    X = np.stack([rng.integers(0, E, N), rng.integers(0, R, N), rng.integers(0, E, N)], 1).astype(np.int64)
    X[1] = X[0]                                   # two queries sharing a filter list
    extra = np.stack([rng.integers(0, E, 120), rng.integers(0, R, 120), rng.integers(0, E, 120)], 1)
    extra[:60, 1:] = X[2, 1:]                     # a run of known heads of one (r, t)
    extra[60:100, :2] = X[3, :2]                  # ... and of known tails of one (h, r)
    return X, np.concatenate([X, extra]).astype(np.int64)


@pytest.mark.parametrize("name", ["TransE", "TransH", "TransD-12-20", "TransD-20-12", "DistMult", "RESCAL", "RotatE"])
def test_int_reference_equals_oracle(name):
    """Every mode of the integer reference, both sides, unfiltered and filtered,
    every score kind it covers: the ranks of oracle.filtered_ranks on the same
    integer weights. float64 is exact on these, ties included, for every model
    but RotatE, whose rotation goes through cos / sin: its ranks are compared
    where the oracle reports no near-tie."""
    rng = np.random.default_rng(12)
    W = _weights(name, rng)
    X, P = _triples(rng)
    model = name.split("-")[0]
    kinds = ["dot"] if model in ("DistMult", "RESCAL") else ["p2", "pow2"] if model == "RotatE" else list(ref.KINDS)
    checked = 0
    for side in ("h", "t"):
        case = ref.model_case(model, W, X, side)
        assert case.E == E and case.n == N
        for positives in (None, P):
            lists = None if positives is None else ref.positive_lists(X, positives, side)
            for kind in kinds:
                got, pos = case.ranks(kind, X[:, 0 if side == "h" else 2], lists)
                oW, limit = W, None
                if model == "RotatE":   # theta = rel / limit * pi = rot * pi / 2
                    oW, limit = {"ent_emb": W["ent_emb"], "rel_emb": W["rot"]}, 2.0
                want, near = orc.filtered_ranks(model, oW, X, side, positives, score=KIND_SCORE[kind], limit=limit,
                                                constraint=False)
                sure = near == 0 if model == "RotatE" else np.ones(N, dtype=bool)
                assert np.array_equal(got[sure], want[sure]), (side, kind, got, want, near)
                assert (np.abs(got - want) <= near)[~sure].all(), (side, kind, got, want, near)
                checked += int(sure.sum())
                assert (got > 1).any()
    assert checked >= (2 * 2 * len(kinds) * N) // 2


def test_pos_score_formula():
    """The float64 score of the integer reduced value, with score_value's clamp."""
    assert ref.pos_score("dot", -7) == -7.0 and ref.pos_score("pinf", 3) == -3.0 and ref.pos_score("p1", 5) == -5.0
    assert ref.pos_score("p2", 9) == -3.0 and ref.pos_score("pow2", 9) == -9.0
    tiny = float(np.float32(1e-9))
    assert ref.pos_score("p1", 0) == -tiny and ref.pos_score("p2", 0) == -np.sqrt(tiny)
    assert ref.pos_score("pow2", 0) == pytest.approx(-tiny, rel=1e-12) and ref.pos_score("pinf", 0) == 0.0


def test_int_reference_refuses_inexact_inputs():
    """Values whose products leave the exact fp32 range are an error of the
    test's inputs, not silently a rounded comparison."""
    big = np.full((4, 3), 1 << 13)
    with pytest.raises(AssertionError):
        ref.Case(ref.MUL, ref.NONE, "t", big, big).ranks("dot", np.zeros(4, dtype=np.int64))
    with pytest.raises(AssertionError):   # sqrt kinds: R past 2^21
        ref.Case(ref.TRANS, ref.NONE, "t", np.full((4, 3), 1000), -np.full((4, 3), 1000)).ranks(
            "p2", np.zeros(4, dtype=np.int64))


@pytest.mark.parametrize("mode,kind", [(ref.TRANS, "p1"), (ref.TRANS, "pinf"), (ref.MUL, "dot"), (ref.ROT, "p2")])
def test_coded_ranks_equal_row_by_row_ranks(mode, kind):
    """The by-row-value count (used for the 16.7M-row table) is the row-by-row one."""
    rng = np.random.default_rng(4)
    E_, n = 1031, 9
    for side in ("h", "t"):
        case = ref.Case(mode, ref.NONE, side, rng.integers(-2, 3, (E_, 2), dtype=np.int8), rng.integers(-2, 3, (n, 2)),
                        q1=rng.integers(-2, 3, (n, 2)) if side == "h" else None)
        ids = rng.integers(0, E_, n)
        for lists in (None, ref.make_filter(rng, E_, n, ids)):
            a, pa = case.ranks(kind, ids, lists)
            b, pb = case.ranks_coded(kind, ids, lists)
            assert np.array_equal(a, b) and np.array_equal(pa, pb) and (a > 1).any()


def test_filter_helpers():
    rng = np.random.default_rng(0)
    for E_, n in ((1, 1), (65, 9), (257, 9), (1031, 77)):
        ids = rng.integers(0, E_, n)
        lists = ref.make_filter(rng, E_, n, ids)
        assert len(lists) == n
        for L in lists:
            assert np.array_equal(L, np.unique(L)) and (len(L) == 0 or (L[0] >= 0 and L[-1] < E_))
        beg, end, ent = ref.filter_csr(lists)
        assert all(np.array_equal(ent[b:e], L) for b, e, L in zip(beg, end, lists))
        words = ref.filter_words(lists, E_)
        assert words.shape == (n, (E_ + 31) // 32)
        for q, L in enumerate(lists):
            bits = np.unpackbits(words[q].view(np.uint8), bitorder="little")[:E_]
            assert np.array_equal(np.nonzero(bits)[0], L)
        if n > 1:
            assert len(lists[0]) == 0 and ids[1] in lists[1] and E_ - 1 in lists[1]
        if E_ > 256:
            assert len(lists[-1]) > 256 and len(lists[-2]) > 64


def _tie_case():
    rng = np.random.default_rng(3)
    W = {"ent_emb": rng.uniform(-0.5, 0.5, (40, 8)), "rel_emb": rng.uniform(-0.5, 0.5, (2, 8))}
    X = np.array([[3, 0, 7], [5, 1, 9]], dtype=np.int64)
    return W, X


def test_near_tie_count_is_zero_without_ties():
    W, X = _tie_case()
    for side in ("h", "t"):
        for P in (None, X):
            _, near = orc.filtered_ranks("TransE", W, X, side, P)
            assert (near == 0).all(), (side, near)   # (the old count included the true entity: >= 1)


def test_near_tie_count_counts_a_near_duplicate_row():
    """A row within the tolerance of the true entity's counts once; an exact
    duplicate ties in float64 as it does bit for bit in the kernel (counted as
    near, not as above); a filtered near-duplicate does not count."""
    W, X = _tie_case()
    ent = W["ent_emb"]
    ent[20] = ent[7] + 1e-8          # near the true tail of query 0
    ent[21] = ent[7]                 # its exact duplicate
    ranks0, _ = orc.filtered_ranks("TransE", W, X[:1], "t", None)
    ent[22] = ent[7] + 1e-8
    ranks, near = orc.filtered_ranks("TransE", W, X, "t", None)
    assert near.tolist() == [3, 0]
    assert abs(int(ranks[0]) - int(ranks0[0])) <= 1          # the new near row moves the rank by at most itself
    P = np.array([[3, 0, 20], [3, 0, 22], [3, 0, 7]], dtype=np.int64)
    _, near = orc.filtered_ranks("TransE", W, X, "t", P)
    assert near.tolist() == [1, 0]
    # the h side: duplicates of the true head
    ent[30] = ent[5] - 1e-8
    _, near = orc.filtered_ranks("TransE", W, X, "h", None)
    assert near.tolist() == [0, 1]
