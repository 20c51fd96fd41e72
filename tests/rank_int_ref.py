"""Exact integer reference for kge_rank (csrc/kge_rank.hip) -- test helper.

kge_rank is fed rows whose entries are small integers, so every fp32 operation
of its scoring functions is exact (all intermediates stay below 2^24) and this
int64 numpy restatement of each mode's reduced value decides the ranks with no
tolerance: for the Lp kinds rank = 1 + #{unfiltered e : R_e < R_true} (the
score maps R monotonically: -R, -sqrt R, -(sqrt R)^2), for Dot and the MUL /
DOT modes rank = 1 + #{unfiltered e : S_e > S_true}. The formulas are those of
the header comment of kge_rank.hip / include/kge_hip.h:

  TRANS   P(e) = e (NONE), e - (w.e) w (HYPER), r_p (e_p.e) + e[:kmin]
          zero-extended to dim (RANK1, no clip);
          't': a = q0 - P(e); 'h': a = (P(e) + q0) - q1
          Lp: R = sum |a| / sum a^2 / max |a|; Dot: sum(q0 P) / sum((P + q0) q1)
  ROT     complex pairs; 't': a = q0 - e; 'h': a = e o q0 - q1; R = sum |a|^2
  MUL     't': sum(q0 e); 'h': sum((e q0) q1)
  DOT     sum(q0 e)

Shared by tests/test_gpu_rank_exact.py (the kernel against this) and
tests/test_rank_int_ref.py (this against the float64 oracle, on the CPU)."""

import numpy as np

TRANS, ROT, MUL, DOT = range(4)          # KGE_RANK_*
NONE, HYPER, RANK1 = range(3)            # KGE_RPROJ_*
KINDS = ("p1", "p2", "pinf", "pow2", "dot")

LIM = 1 << 24        # integers below this are exact in fp32, and so are their sums and products
# sqrt kinds (p2, pow2): -sqrtf(R) and -(sqrtf(R))^2 carry up to 1.5 * 2^-23
# relative error, so R and R + 1 are sure to stay distinct floats (and the
# integer order to be the score's) only while 1 / R > 3 * 2^-23: R < 2^21
SQRT_LIM = 1 << 21


def _chk(*xs):
    for x in xs:
        assert np.abs(x).max(initial=0) < LIM, "intermediate leaves the exact fp32 range"
    return xs[0]


def _sum(t):
    """Row sums whose every partial sum is exact in fp32."""
    assert np.abs(t).sum(axis=1).max(initial=0) < LIM, "sum leaves the exact fp32 range"
    return t.sum(axis=1)


class Case:
    """One kge_rank problem on integer rows (int64 numpy arrays)."""

    def __init__(self, mode, proj, side, cand, q0, q1=None, qw=None, aux=None, dim=None):
        self.mode, self.proj, self.side = mode, proj, side
        as64 = lambda a: None if a is None else np.asarray(a, dtype=np.int64)   # noqa: E731
        self.q0, self.q1, self.qw = as64(q0), as64(q1), as64(qw)
        # the tables stay in the integer type they come in (a 16.7M-row table is
        # int8); values() widens them
        self.cand, self.aux = np.asarray(cand), None if aux is None else np.asarray(aux)
        assert self.cand.dtype.kind == "i" and (self.aux is None or self.aux.dtype.kind == "i")
        self.dim = int(self.q0.shape[1] if dim is None else dim)
        self.E, self.n = int(self.cand.shape[0]), int(self.q0.shape[0])

    def values(self, kind, q, cand=None):
        """(V [E] int64, lower_is_better) of query q against every candidate
        (``cand``: against these rows in the table's place)."""
        D, hs = self.dim, self.side == "h"
        x = (self.cand if cand is None else cand).astype(np.int64)
        a0 = self.q0[q]
        a1 = self.q1[q] if self.q1 is not None else None
        w = self.qw[q] if self.qw is not None else None
        if self.mode == ROT:
            assert kind in ("p2", "pow2"), "RotatE p = 1 / inf take a sqrt per element: not exact"
            er, ei = x[:, 0:D:2], x[:, 1:D:2]
            if hs:
                xr = _chk(er * a0[0::2]) - _chk(ei * a0[1::2])
                xi = _chk(er * a0[1::2]) + _chk(ei * a0[0::2])
                ar, ai = _chk(xr) - a1[0::2], _chk(xi) - a1[1::2]
            else:
                ar, ai = a0[0::2] - er, a0[1::2] - ei
            R = _sum(_chk(_chk(ar * ar) + _chk(ai * ai)))
            assert R.max(initial=0) < SQRT_LIM
            return R, True
        if self.mode in (MUL, DOT):
            t = _chk(_chk(x[:, :D] * a0) * a1) if (self.mode == MUL and hs) else _chk(a0 * x[:, :D])
            return _sum(t), False
        if self.proj == HYPER:
            dt = _sum(_chk(w * x[:, :D]))
            P = _chk(x[:, :D] - _chk(dt[:, None] * w))
        elif self.proj == RANK1:
            assert cand is None
            cols = x.shape[1]
            kmin = min(D, cols)
            de = _sum(_chk(self.aux.astype(np.int64) * x))
            xe = np.zeros((self.E, D), dtype=np.int64)
            xe[:, :kmin] = x[:, :kmin]
            P = _chk(_chk(w * de[:, None]) + xe)
        else:
            P = x[:, :D]
        if kind == "dot":
            return _sum(_chk(_chk(P + a0) * a1) if hs else _chk(a0 * P)), False
        m = np.abs(_chk(_chk(P + a0) - a1) if hs else _chk(a0 - P))
        if kind == "p1":
            return _sum(m), True
        if kind == "pinf":
            return m.max(axis=1), True
        assert kind in ("p2", "pow2"), kind
        R = _sum(_chk(m * m))
        assert R.max(initial=0) < SQRT_LIM
        return R, True

    def ranks(self, kind, ids, lists=None):
        """(ranks int64 [n], pos scores float64 [n]): filtered ranks of the true
        entities ``ids`` (``lists``: per query the filtered entity ids, or None)."""
        ranks = np.zeros(self.n, dtype=np.int64)
        pos = np.zeros(self.n, dtype=np.float64)
        for q in range(self.n):
            V, lower = self.values(kind, q)
            vt = int(V[ids[q]])
            above = (V < vt) if lower else (V > vt)
            if lists is not None:
                above[lists[q]] = False
            ranks[q] = 1 + int(np.count_nonzero(above))
            pos[q] = pos_score(kind, vt)
        return ranks, pos

    def ranks_coded(self, kind, ids, lists=None):
        """``ranks`` for a table too long to score row by row but with few
        distinct rows (16.7M rows of two elements in {-2..2}: 25): every
        possible row is scored once per query with ``values`` and the counts
        come from the histogram of the table's rows over them, less the
        filtered ones."""
        assert self.proj != RANK1
        x = self.cand[:, :self.dim]
        lo, span = int(x.min()), int(x.max()) - int(x.min()) + 1
        nrow = span ** self.dim
        assert nrow <= 4096
        code = np.zeros(self.E, dtype=np.int16)
        for c in range(self.dim):
            code = code * span + (x[:, c].astype(np.int16) - lo)
        table = (np.arange(nrow)[:, None] // span ** np.arange(self.dim - 1, -1, -1)[None, :]) % span + lo
        hist = np.bincount(code, minlength=nrow)
        ranks = np.zeros(self.n, dtype=np.int64)
        pos = np.zeros(self.n, dtype=np.float64)
        for q in range(self.n):
            V, lower = self.values(kind, q, cand=table)
            vt = int(V[code[ids[q]]])
            above = (V < vt) if lower else (V > vt)
            cnt = int(hist[above].sum())
            if lists is not None:
                cnt -= int(np.count_nonzero(above[code[lists[q]]]))
            ranks[q] = 1 + cnt
            pos[q] = pos_score(kind, vt)
        return ranks, pos


def pos_score(kind, v):
    """kge_models.h score_value on the integer reduced value, in float64 (the
    Lp kinds with finite p clamp R to 1e-9 first, score.py:49-76)."""
    if kind == "dot":
        return float(v)
    if kind == "pinf":
        return -float(v)
    r = max(float(v), float(np.float32(1e-9)))
    if kind == "p1":
        return -r
    lp = -np.sqrt(r)
    return lp if kind == "p2" else -(lp * lp)


# ---------------------------------------------------------------- filters
def make_filter(rng, E, n, ids):
    """Per query a sorted, unique id list: empty lists (every fourth query),
    lists holding the query's true entity (odd queries), the ids at the bitmap's
    word edges (0, 31, 32, 63, 64, E - 1), a hub of 300 ids on the last query
    when E > 256 (longer than a workgroup's stride over a list) and one of 70
    on the one before when E > 64 (longer than a wave's)."""
    special = [e for e in (0, 31, 32, 63, 64, E - 1) if 0 <= e < E]
    lists = []
    for q in range(n):
        s = set()
        if n == 1 or q % 4:
            s.update(rng.integers(0, E, int(rng.integers(1, 25))).tolist())
            if q % 2:
                s.add(int(ids[q]))
            if n == 1 or q % 4 == 1:
                s.update(special)
        lists.append(s)
    if n >= 2 and E > 256:
        lists[n - 1] = set(rng.permutation(min(E, 1 << 16))[:300].tolist()) | set(special)
    if n >= 3 and E > 64:
        lists[n - 2] = set(rng.permutation(min(E, 1 << 16))[:70].tolist()) | {E - 1}
    return [np.array(sorted(s), dtype=np.int64) for s in lists]


def filter_csr(lists):
    """(beg [n], end [n], ent) of the lists laid end to end."""
    lens = np.array([len(x) for x in lists], dtype=np.int64)
    end = np.cumsum(lens)
    ent = np.concatenate(lists) if len(lists) else np.zeros(0, dtype=np.int64)
    return end - lens, end, ent.astype(np.int64)


def filter_words(lists, E):
    """The bitmap kge_rank builds: bit e of query q's ceil(E / 32) words."""
    W = (E + 31) // 32
    out = np.zeros((len(lists), W), dtype=np.uint32)
    for q, ents in enumerate(lists):
        np.bitwise_or.at(out[q], ents >> 5, np.uint32(1) << (ents & 31).astype(np.uint32))
    return out


def positive_lists(X, P, side):
    """get_rank's filter (BaseModel.py:646-650): per query the corrupted-side
    entities of the known positives sharing its (relation, kept entity)."""
    keep, corr = (2, 0) if side == "h" else (0, 2)
    return [np.unique(P[(P[:, 1] == x[1]) & (P[:, keep] == x[keep]), corr]).astype(np.int64) for x in X]


# ---------------------------------------------------------------- model rows
def model_case(name, W, X, side):
    """The Case kge_rank is given for a model's integer weights W and triples X:
    ranking.py's row builders (the model's own op order) in int64. TransD
    without its clip; RotatE takes the rotation ``rot`` [R, d] in quarter turns
    (w = i^rot) in place of rel_emb."""
    g = lambda k: np.asarray(W[k], dtype=np.int64)   # noqa: E731
    h, r, t = X[:, 0], X[:, 1], X[:, 2]
    ent = g("ent_emb")
    if name == "TransE":
        q0, q1 = (ent[h] + g("rel_emb")[r], None) if side == "t" else (g("rel_emb")[r], ent[t])
        return Case(TRANS, NONE, side, ent, q0, q1)
    if name == "TransH":
        w = g("rel_hyper")[r]
        proj = lambda e: e - np.sum(w * e, axis=-1, keepdims=True) * w   # noqa: E731
        q0, q1 = (proj(ent[h]) + g("rel_emb")[r], None) if side == "t" else (g("rel_emb")[r], proj(ent[t]))
        return Case(TRANS, HYPER, side, ent, q0, q1, qw=w)
    if name == "TransD":
        rp, ep, re_ = g("rel_proj")[r], g("ent_proj"), g("rel_emb")[r]
        kr, ke = re_.shape[1], ent.shape[1]

        def proj(i):
            p = rp * np.sum(ep[i] * ent[i], axis=-1, keepdims=True)
            p[:, :min(kr, ke)] += ent[i][:, :min(kr, ke)]
            return p
        q0, q1 = (proj(h) + re_, None) if side == "t" else (re_, proj(t))
        return Case(TRANS, RANK1, side, ent, q0, q1, qw=rp, aux=ep, dim=kr)
    if name == "DistMult":
        ri = g("rel_inter")[r]
        q0, q1 = (ent[h] * ri, None) if side == "t" else (ri, ent[t])
        return Case(MUL, NONE, side, ent, q0, q1)
    if name == "RESCAL":
        Rm = g("rel_inter")[r]
        q0 = np.einsum("ni,nij->nj", ent[h], Rm) if side == "t" else np.einsum("nij,nj->ni", Rm, ent[t])
        return Case(DOT, NONE, side, ent, q0)
    if name == "RotatE":
        k = g("rot")[r] % 4
        wr, wi = np.array([1, 0, -1, 0])[k], np.array([0, 1, 0, -1])[k]
        n, d = k.shape
        if side == "t":
            hr, hi = ent[h][..., 0], ent[h][..., 1]
            q0, q1 = np.stack([hr * wr - hi * wi, hr * wi + hi * wr], -1).reshape(n, 2 * d), None
        else:
            q0, q1 = np.stack([wr, wi], -1).reshape(n, 2 * d), ent[t].reshape(n, 2 * d)
        return Case(ROT, NONE, side, ent.reshape(ent.shape[0], 2 * d), q0, q1)
    raise ValueError(name)
