"""GPU: KGEModel.predict with float weights against the float64 oracle.

The models, weights and triples are those of tests/test_gpu_rank_exact.py part
B (E = 1031, n = 77, a 300-head hub among the known positives). The reference
scores every entity with oracle.kge_oracle._score_hrt in float64 and sets the
filtered ones to -inf, exactly as filtered_ranks does. An fp32 evaluation may
order two scores within tol = 1e-5 * max(1, |s|) (the oracle's tie_tol) either
way, so a query whose float64 k-th and (k+1)-th scores are that close is
boundary-tied: its returned set is only required to hold everything clearly
above the boundary. The oracle alone leaves at most 4 of the 77 queries so."""

import functools

import numpy as np
import pytest
import torch

from tests.test_gpu_rank_exact import BE, BMODELS, BN, _b_model, b_limit, b_triples, b_weights

pytestmark = pytest.mark.gpu

TIE_TOL = 1e-5
TIED_CAP = 4
KS = (1, 10, 100)


@pytest.fixture(autouse=True)
def _gpu(hiplib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=None)
def oracle_scores(key, side):
    """float64 scores [n, E] of every entity on the corrupted side, the known
    positives at -inf. Read-only."""
    from oracle import kge_oracle as orc
    cls, _, sc, kw, _, _ = BMODELS[key]
    W = {k: torch.tensor(np.asarray(v), dtype=orc.F64) for k, v in b_weights(key).items()}
    L = orc._Lookups(W, False)
    cfg = {"constraint": bool(kw.get("constraint", False)), "constraint_weight": 1.0, "limit": b_limit(key)}
    X, P = b_triples()
    keep, corr = (2, 0) if side == "h" else (0, 2)
    every = np.arange(BE)
    out = np.zeros((BN, BE))
    with torch.no_grad():
        for i, x in enumerate(X):
            h = every if side == "h" else np.full(BE, x[0])
            t = every if side == "t" else np.full(BE, x[2])
            s = orc._score_hrt(cls, W, L, h, np.full(BE, x[1]), t, sc if sc is not None else ("dot", 0.0),
                               cfg).numpy().copy()
            s[P[(P[:, 1] == x[1]) & (P[:, keep] == x[keep]), corr]] = -np.inf
            out[i] = s
    out.setflags(write=False)
    return out


def _tol(s):
    return TIE_TOL * max(1.0, abs(s))


def check_against_oracle(key, side, k, ids, scores, tag=""):
    S = oracle_scores(key, side)
    order = np.argsort(-S, axis=1, kind="stable")
    kth = np.take_along_axis(S, order[:, k - 1:k], 1)[:, 0]
    nxt = np.take_along_axis(S, order[:, k:k + 1], 1)[:, 0]
    assert np.isfinite(nxt).all()          # more than k live entities per query
    tied = np.array([abs(a - b) <= _tol(a) for a, b in zip(kth, nxt)])
    print(key, side, k, tag, "boundary-tied queries:", int(tied.sum()), "of", BN)
    assert tied.sum() <= TIED_CAP, (key, side, k, np.nonzero(tied)[0])
    assert ids.shape == (BN, k) and scores.shape == (BN, k)
    for q in range(BN):
        got = ids[q]
        assert (got >= 0).all() and len(set(got.tolist())) == k, (key, side, k, q)
        want = S[q, got]
        assert np.isfinite(want).all(), (key, side, k, q, "a filtered id was returned")
        err = np.abs(scores[q].astype(np.float64) - want)
        assert (err <= TIE_TOL * np.maximum(1.0, np.abs(want))).all(), (key, side, k, q, err.max())
        assert (scores[q, 1:] <= scores[q, :-1]).all(), (key, side, k, q)
        same = scores[q, 1:] == scores[q, :-1]
        assert (got[1:][same] > got[:-1][same]).all(), (key, side, k, q)
        if not tied[q]:
            assert set(got.tolist()) == set(order[q, :k].tolist()), (key, side, k, q)
        else:
            clear = np.nonzero(S[q] > kth[q] + _tol(kth[q]))[0]
            assert set(clear.tolist()) <= set(got.tolist()), (key, side, k, q)


@pytest.mark.parametrize("key", list(BMODELS))
def test_predict_matches_oracle(key):
    """Every fused model through predict's native path, both sides, k = 1, 10
    (the tiled producer where the model has one) and 100 (the lane producer).
    TransR runs one call per relation group, the single query 40 included."""
    from KGE import ranking
    m = _b_model(key)
    assert ranking.supported(m)
    if BMODELS[key][0] == "RotatE":
        m._set_limit()
    X, P = b_triples()
    for side in ("h", "t"):
        for k in KS:
            ids, scores = m.predict(X, side, k=k, positive_X=P)
            assert ids.dtype == np.int64 and scores.dtype == np.float32
            check_against_oracle(key, side, k, ids, scores)
    # the corrupted column is ignored, and no filter means the hub's heads come back
    Xi = X.copy()
    Xi[:, 0] = -1
    a = m.predict(Xi, "h", k=10, positive_X=P)
    b = m.predict(X, "h", k=10, positive_X=P)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    raw = m.predict(X[:1], "h", k=1000)
    flt = m.predict(X[:1], "h", k=1000, positive_X=P)
    live = BE - len(np.unique(P[(P[:, 1] == X[0, 1]) & (P[:, 2] == X[0, 2]), 0]))
    assert live < 1000 and (raw[0] >= 0).all() and (flt[0][0, :live] >= 0).all()
    assert (flt[0][0, live:] == -1).all() and np.isneginf(flt[1][0, live:]).all()


@pytest.mark.parametrize("key", ["TransR", "DistMult"])
def test_predict_query_chunking(key, monkeypatch):
    """ranking._BITS_MAX_BYTES down to ten queries' bitmaps: batched_topk runs
    the set (TransR: each relation group) in chunks, with the same results."""
    from KGE import _hip, ranking
    m = _b_model(key)
    X, P = b_triples()
    calls = []
    real = _hip.kge_topk_desc

    def spy():
        calls.append(real())
        return calls[-1]
    monkeypatch.setattr(ranking._hip, "kge_topk_desc", spy)
    for side in ("h", "t"):
        want = m.predict(X, side, k=10, positive_X=P)
        whole = len(calls)
        limit = ranking._BITS_MAX_BYTES
        monkeypatch.setattr(ranking, "_BITS_MAX_BYTES", 10 * ((BE + 31) // 32) * 4)
        got = m.predict(X, side, k=10, positive_X=P)
        monkeypatch.setattr(ranking, "_BITS_MAX_BYTES", limit)
        assert len(calls) - whole > whole and max(c.q.n for c in calls[whole:]) <= 10
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        del calls[:]


def test_predict_fallback_agrees_with_native():
    """A score function of the user's own (a subclass of LpDistance) takes
    predict's score_hrt fallback: the same answers as the native path within
    the near-tie rule, against the same oracle."""
    from KGE import ranking, score

    class MyLp(score.LpDistance):
        pass

    key = "TransH"
    m = _b_model(key)
    X, P = b_triples()
    native = m.predict(X, "t", k=10, positive_X=P)
    m.score_fn = MyLp(BMODELS[key][2][1])
    assert not ranking.supported(m)
    ids, scores = m.predict(X, "t", k=10, positive_X=P)
    check_against_oracle(key, "t", 10, ids, scores, tag="fallback")
    S = oracle_scores(key, "t")
    for q in range(BN):
        diff = set(ids[q].tolist()) ^ set(native[0][q].tolist())
        kth = np.sort(S[q])[::-1][9]
        assert all(abs(S[q, e] - kth) <= _tol(kth) for e in diff), (q, diff)
