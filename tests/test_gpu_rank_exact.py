"""GPU: kge_rank (csrc/kge_rank.hip) held to exact ranks.

Part A drives the C-ABI with rows of small integers: every fp32 operation of
the scoring functions is then exact, the reference is plain int64 numpy
(tests/rank_int_ref.py) and the ranks must be equal with no tolerance, through
every launch path: the register-tiled and the lane-per-candidate count pass,
the bitmap filter (LDS and global-atomics build) and the rescoring filter
passes, int32 ids, padded rows, the sizes around the tile / group / chunk
widths, the lane pass's second launch and the staged-row limit. The many exact
ties small integers produce sit right on the strict > of the count.

Part B ranks float weights through ranking.batched_ranks against the float64
oracle: equal wherever the oracle sees no countable candidate within the tie
tolerance of the true score, within that count elsewhere."""

import ctypes

import numpy as np
import pytest
import torch

from tests import rank_int_ref as ref
from tests.rank_int_ref import DOT, HYPER, MUL, NONE, RANK1, ROT, TRANS

pytestmark = pytest.mark.gpu

SCORE = {"p1": (0, 1.0), "p2": (0, 2.0), "pinf": (0, float("inf")), "pow2": (1, 2.0), "dot": (2, 0.0)}   # KGE_SCORE_*
MODES = {"trans": (TRANS, NONE), "hyper": (TRANS, HYPER), "rank1": (TRANS, RANK1), "rot": (ROT, NONE),
         "mul": (MUL, NONE), "dot": (DOT, NONE)}
LANE = 1   # KGE_RANK_FLAG_LANE_PASS


@pytest.fixture(autouse=True)
def _gpu(hiplib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _kinds(mode):
    return ("dot",) if mode in (MUL, DOT) else ("pow2", "p2") if mode == ROT else ref.KINDS


def _variants(mode, proj):
    """(flags, bitmap): the tiled modes have two count passes and two filter
    passes; for the projected modes and ROT the lane flag is a no-op."""
    if mode == ROT or proj != NONE:
        return [(0, True), (0, False)]
    return [(0, True), (0, False), (LANE, True), (LANE, False)]


def make_case(rng, mode, proj, side, E, n, dim, cols=None, lo=-2, hi=2):
    cols = dim if cols is None else cols
    r = lambda *s: rng.integers(lo, hi + 1, s, dtype=np.int8)   # noqa: E731
    return ref.Case(mode, proj, side, r(E, cols), r(n, dim),
                    q1=r(n, dim) if (side == "h" and mode != DOT) else None,
                    qw=r(n, dim) if proj != NONE else None,
                    aux=r(E, cols) if proj == RANK1 else None, dim=dim)


class DevCase:
    """A ref.Case on the device, run through the kge_rank C-ABI.

    ``pad``: rows are laid out with cand.ld = cols + 3 (the aux table too) and
    ldq = dim + 5, the padding filled with NaN; ``idx32``: int32 true_ids /
    filt_ent. Outputs and the bitmap are prefilled with garbage before each run."""

    def __init__(self, case, ids, lists=None, idx32=False, pad=False):
        self.case, self.dev = case, torch.device("cuda", 0)
        self.ids_np, self.lists = np.asarray(ids, dtype=np.int64), lists
        self.cand = self._rows(case.cand, 3 if pad else 0)
        self.aux = self._rows(case.aux, 3 if pad else 0)
        self.q0, self.q1, self.qw = (self._rows(a, 5 if pad else 0) for a in (case.q0, case.q1, case.qw))
        self.idt = torch.int32 if idx32 else torch.int64
        self.ids = torch.as_tensor(self.ids_np, device=self.dev).to(self.idt)
        if lists is not None:
            beg, end, ent = ref.filter_csr(lists)
            self.fb, self.fe = torch.as_tensor(beg, device=self.dev), torch.as_tensor(end, device=self.dev)
            self.fent = torch.as_tensor(ent, device=self.dev).to(self.idt)
        self.W = (case.E + 31) // 32

    def _rows(self, a, pad):
        """(storage, view of the values): small integers go up as int8."""
        if a is None:
            return None
        assert np.abs(a).max(initial=0) < 128
        t = torch.from_numpy(np.ascontiguousarray(a.astype(np.int8))).to(self.dev).to(torch.float32)
        full = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=self.dev)
        full[:, :t.shape[1]] = t
        return full, full[:, :t.shape[1]]

    def run(self, kind, flags=0, bitmap=False, n=None):
        """-> (return code, ranks, pos scores, status word, bitmap words or None)."""
        from KGE import _hip
        c = self.case
        n = c.n if n is None else n
        rk = torch.full((c.n,), -1, dtype=torch.int64, device=self.dev)
        ps = torch.full((c.n,), float("nan"), dtype=torch.float32, device=self.dev)
        status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        d = _hip.kge_rank_desc()
        d.abi_version = _hip.ABI_VERSION
        d.mode, d.proj = c.mode, c.proj
        d.corrupt_side = _hip.SIDE_H if c.side == "h" else _hip.SIDE_T
        d.cand = _hip.table(self.cand[1])
        assert d.cand.ld == self.cand[0].shape[1] and d.cand.cols == c.cand.shape[1]
        if self.aux is not None:
            d.cand_aux = _hip.table(self.aux[1])
        d.dim, d.clip = c.dim, 0
        d.q0 = self.q0[0].data_ptr()
        d.q1 = self.q1[0].data_ptr() if self.q1 is not None else None
        d.qw = self.qw[0].data_ptr() if self.qw is not None else None
        d.ldq = self.q0[0].shape[1]
        d.true_ids = self.ids.data_ptr()
        d.idx_dtype = _hip.IDX_I32 if self.idt == torch.int32 else _hip.IDX_I64
        d.score_kind, d.score_p = SCORE[kind]
        d.flags, d.n = flags, n
        bits = None
        if self.lists is not None:
            d.filt_beg, d.filt_end, d.filt_ent = self.fb.data_ptr(), self.fe.data_ptr(), self.fent.data_ptr()
            if bitmap:
                bits = torch.full((c.n * self.W,), -1, dtype=torch.int32, device=self.dev)
                d.filt_bits, d.filt_bits_words = bits.data_ptr(), bits.numel()
        d.rank_out, d.pos_score_out, d.status = rk.data_ptr(), ps.data_ptr(), status.data_ptr()
        rc = _hip.lib().kge_rank(ctypes.byref(d), _hip.stream_handle(self.dev))
        torch.cuda.synchronize()
        words = None if bits is None else bits.view(c.n, self.W).cpu().numpy().view(np.uint32)
        return rc, rk.cpu().numpy(), ps.cpu().numpy(), int(status.item()), words


def check(dc, kinds=None, variants=None, coded=False):
    """Every variant of every kind: ranks equal to the integer reference's,
    pos scores the float64 formula's, bitmap words the filter lists'."""
    from KGE import _hip
    c = dc.case
    want_words = None
    for kind in (_kinds(c.mode) if kinds is None else kinds):
        want, wpos = (c.ranks_coded if coded else c.ranks)(kind, dc.ids_np, dc.lists)
        for flags, bitmap in (_variants(c.mode, c.proj) if variants is None else variants):
            rc, got, pos, status, words = dc.run(kind, flags, bitmap)
            tag = (c.mode, c.proj, c.side, c.E, c.n, c.dim, kind, flags, bitmap)
            assert rc == _hip.KGE_OK and status == 0, (tag, rc, status)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (tag, bad[:10], got[bad][:10], want[bad][:10])
            if kind in ("p2", "pow2"):   # sqrtf and one multiply: <= 2^-22 relative
                assert np.allclose(pos, wpos, rtol=1e-6, atol=0), (tag, pos, wpos)
            else:
                assert np.array_equal(pos.astype(np.float64), wpos), (tag, pos, wpos)
            if words is not None:
                if want_words is None:
                    want_words = ref.filter_words(dc.lists, c.E)
                assert np.array_equal(words, want_words), (tag, np.nonzero(words != want_words))
    return want


def _dev_case(rng, key, side, E, n, dim, cols=None, **kw):
    mode, proj = MODES[key]
    case = make_case(rng, mode, proj, side, E, n, dim, cols)
    ids = rng.integers(0, E, n)
    return DevCase(case, ids, ref.make_filter(rng, E, n, ids), **kw)


# ---------------------------------------------------------------- part A
DIMS = [(k, d) for k in ("trans", "hyper", "rank1", "mul", "dot") for d in (3, 16, 17, 20, 33)] + \
       [("rot", d) for d in (2, 18, 34)]


@pytest.mark.parametrize("key,dim", DIMS)
def test_exact_modes_and_dims(key, dim):
    """Every (mode, projection, side) at every row width class: below a float4,
    one staged chunk, a chunk and a remainder, a multiple of 4 but not of 16,
    two chunks and one element. E = 257 is two lane chunks and five tiles with
    one candidate in the last; n = 9 one query past a lane group."""
    rng = np.random.default_rng(1000 + dim)
    for side in ("h", "t"):
        ranks = check(_dev_case(rng, key, side, 257, 9, dim))
        assert (ranks > 1).any()


SIZES = [(1, 1), (63, 7), (64, 8), (65, 65), (257, 9), (1031, 77), (1, 9), (65, 1), (257, 63), (1031, 8)]


@pytest.mark.parametrize("E,n", SIZES)
def test_exact_sizes(E, n):
    """E and n around the tile (64), the lane group (8) and the lane chunk
    (256), one below / at / one above, every mode and side, one score kind
    each in turn."""
    rng = np.random.default_rng(E * 131 + n)
    for i, (key, dim) in enumerate([("trans", 17), ("hyper", 20), ("rank1", 16), ("rot", 18), ("mul", 17),
                                    ("dot", 20)]):
        for j, side in enumerate(("h", "t")):
            kinds = _kinds(MODES[key][0])
            check(_dev_case(rng, key, side, E, n, dim), kinds=(kinds[(i + j + E + n) % len(kinds)],))


@pytest.mark.parametrize("cols,dim", [(12, 20), (20, 12)])
def test_exact_transd_widths(cols, dim):
    """RANK1 with entity rows narrower and wider than the projected rows
    (kmin = cols and kmin = dim), more than one candidate chunk."""
    rng = np.random.default_rng(cols)
    for side in ("h", "t"):
        for E, n in ((300, 9), (1031, 77)):
            check(_dev_case(rng, "rank1", side, E, n, dim, cols), kinds=("p1", "p2", "dot") if E == 300 else ("pinf",))


@pytest.mark.parametrize("key,dim", [("trans", 17), ("hyper", 20), ("rank1", 20), ("rot", 18), ("mul", 33),
                                     ("dot", 3)])
def test_exact_padded_rows(key, dim):
    """cand.ld = cols + 3 and ldq = dim + 5 with NaN in the padding (the aux
    table too): no pass may read past a row's values."""
    rng = np.random.default_rng(77 + dim)
    for side in ("h", "t"):
        dc = _dev_case(rng, key, side, 257, 9, dim, cols=12 if key == "rank1" else None, pad=True)
        assert torch.isnan(dc.cand[0][:, -3:]).all() and torch.isnan(dc.q0[0][:, -5:]).all()
        check(dc, kinds=_kinds(MODES[key][0])[:2])


@pytest.mark.parametrize("key", ["trans", "hyper", "rank1", "rot", "mul", "dot"])
def test_exact_int32_ids(key):
    """idx_dtype = KGE_IDX_I32: int32 true_ids and filt_ent, both sides, read by
    the pos pass, the bitmap build and both rescoring filter passes."""
    rng = np.random.default_rng(32)
    for side in ("h", "t"):
        check(_dev_case(rng, key, side, 1031, 9, 18 if key == "rot" else 17, idx32=True),
              kinds=_kinds(MODES[key][0])[:1])


@pytest.mark.parametrize("E", [262144, 262145, 262221])
def test_exact_bitmap_builds(E):
    """The two bitmap builds at their boundary: ceil(E / 32) = 8192 words is the
    last size gathered in LDS (all of its 32 KB), 8193 and 8195 the first built
    with global atomics after a clear -- the buffer comes in as all ones, so a
    missing clear leaves every candidate filtered. Words, and ranks against the
    reference and the rescoring pass, tiled and lane count."""
    rng = np.random.default_rng(E)
    for side in ("h", "t"):
        dc = _dev_case(rng, "trans", side, E, 10, 8)
        assert E - 1 in dc.lists[1] and len(dc.lists[-1]) > 256
        ranks = check(dc, kinds=("p1",))
        assert (ranks > 1000).any()


def test_exact_second_lane_launch():
    """E = 65,535 * 256 + 300: the lane pass needs a second launch for the last
    two candidate chunks (grid y <= 65,535), the tiled pass 262,145 tiles along
    x; the bitmap (524,290 words per query) is built with global atomics. The
    134 MB table has 25 distinct rows: the reference counts by row value."""
    E, n = 65535 * 256 + 300, 9
    rng = np.random.default_rng(5)
    dc = _dev_case(rng, "trans", "t", E, n, 2)
    assert E - 1 in dc.lists[1]   # a filter bit in the last word, in the second launch's chunks
    ranks = check(dc, kinds=("p1",), variants=[(LANE, True), (0, True)], coded=True)
    assert (ranks > 1 << 20).any()


def test_exact_lds_limit():
    """dim = 680 stages 3 * 8 * 680 floats = 65,280 B of query rows, the widest
    the lane pass accepts; 684 is refused, by kge_rank and by
    ranking.supported() at the same width."""
    from KGE import _hip, ranking
    from tests.test_plugin_surface import build
    rng = np.random.default_rng(680)
    mode, proj = MODES["mul"]
    case = make_case(rng, mode, proj, "t", 300, 9, 680, lo=-1, hi=1)
    ids = rng.integers(0, 300, 9)
    check(DevCase(case, ids, ref.make_filter(rng, 300, 9, ids)))
    wide = make_case(rng, mode, proj, "t", 300, 9, 684, lo=-1, hi=1)
    for flags in (LANE, 0):
        rc, rk, _, _, _ = DevCase(wide, ids, ref.make_filter(rng, 300, 9, ids)).run("dot", flags, True)
        assert rc == _hip.KGE_EUNSUPPORTED and (rk == -1).all()
    dev = torch.device("cuda", 0)
    for d, ok in ((680, True), (681, False), (684, False)):
        m = build("DistMult", embedding_params={"embedding_size": d})
        m.model_weights = {"ent_emb": torch.zeros(4, d, device=dev), "rel_inter": torch.zeros(2, d, device=dev)}
        assert ranking.supported(m) is ok, d
        assert (3 * ranking.RANK_Q * ((d + 3) & ~3) * 4 <= 64 * 1024) is ok


def test_exact_status_paths():
    """A true id equal to E sets KGE_ERANGE in the status word (the call
    returns OK, as for filter ids) and leaves the other queries' ranks right;
    n = 0 returns OK and touches nothing."""
    from KGE import _hip
    rng = np.random.default_rng(9)
    for key in ("trans", "hyper"):
        mode, proj = MODES[key]
        case = make_case(rng, mode, proj, "t", 257, 9, 17)
        ids = rng.integers(0, 257, 9)
        lists = ref.make_filter(rng, 257, 9, ids)
        want, _ = case.ranks("p1", ids, lists)
        bad = ids.copy()
        bad[4] = 257
        for flags, bitmap in _variants(mode, proj):
            rc, got, _, status, _ = DevCase(case, bad, lists).run("p1", flags, bitmap)
            assert rc == _hip.KGE_OK and status == _hip.KGE_ERANGE
            keep = np.arange(9) != 4
            assert np.array_equal(got[keep], want[keep])
            rc, got, pos, status, words = DevCase(case, ids, lists).run("p1", flags, bitmap, n=0)
            assert rc == _hip.KGE_OK and status == 0
            assert (got == -1).all() and np.isnan(pos).all() and (words is None or (words == 0xFFFFFFFF).all())


# ---------------------------------------------------------------- part B
BE, BR, BN = 1031, 5, 77

# name -> (class, embedding_params, score, constructor kwargs, weight scale, seed). The seeds were chosen on the
# CPU so that the float64 oracle alone stays under the cap asserted below; behind each, the number of the 77
# queries for which it reports a near-tie on the (h, t) side (seeds 1..5 gave 0..11 for every model).
_D1220 = {"ent_embedding_size": 12, "rel_embedding_size": 20}
_D2012 = {"ent_embedding_size": 20, "rel_embedding_size": 12}
BMODELS = {
    "TransH": ("TransH", {"embedding_size": 20}, ("lp", 2.0), {}, 1.0, 1),                    # (2, 5)
    "TransD-12-20": ("TransD", _D1220, ("lp", 2.0), {"constraint": False}, 1.0, 1),           # (3, 4)
    "TransD-12-20-clip": ("TransD", _D1220, ("lp", 2.0), {"constraint": True}, 1.0, 1),       # (4, 3)
    "TransD-20-12": ("TransD", _D2012, ("lp", 2.0), {"constraint": False}, 1.0, 1),           # (5, 2)
    "TransD-20-12-clip": ("TransD", _D2012, ("lp", 2.0), {"constraint": True}, 1.0, 1),       # (1, 2)
    "TransR": ("TransR", _D1220, ("lp", 2.0), {"constraint": True}, 1.0, 1),                  # (3, 6)
    "RESCAL": ("RESCAL", {"embedding_size": 20}, None, {}, 1.0, 1),                           # (1, 0)
    "RotatE": ("RotatE", {"embedding_size": 17}, ("lp", 1.0), {}, 1.0, 1),                    # (1, 4)
    "DistMult": ("DistMult", {"embedding_size": 19}, None, {}, 1.0, 1),                       # (2, 4)
    "TransE-p3": ("TransE", {"embedding_size": 20}, ("lp", 3.0), {}, 1.0, 1),                 # (4, 3)
}
NEAR_CAP = 12


def b_weights(key):
    """float32 weights ~ U(-0.5, 0.5) * scale, as numpy."""
    cls, ep, _, _, scale, seed = BMODELS[key]
    rng = np.random.default_rng(seed)
    u = lambda *s: (rng.uniform(-0.5, 0.5, s) * scale).astype(np.float32)   # noqa: E731
    d = ep.get("embedding_size")
    ke, kr = ep.get("ent_embedding_size"), ep.get("rel_embedding_size")
    if cls == "TransE":
        return {"ent_emb": u(BE, d), "rel_emb": u(BR, d)}
    if cls == "TransH":
        return {"ent_emb": u(BE, d), "rel_emb": u(BR, d), "rel_hyper": u(BR, d)}
    if cls == "TransD":
        return {"ent_emb": u(BE, ke), "rel_emb": u(BR, kr), "ent_proj": u(BE, ke), "rel_proj": u(BR, kr)}
    if cls == "TransR":
        return {"ent_emb": u(BE, ke), "rel_emb": u(BR, kr), "rel_proj": u(BR, ke, kr)}
    if cls == "RESCAL":
        return {"ent_emb": u(BE, d), "rel_inter": u(BR, d, d)}
    if cls == "RotatE":
        return {"ent_emb": u(BE, d, 2), "rel_emb": u(BR, d)}
    if cls == "DistMult":
        return {"ent_emb": u(BE, d), "rel_inter": u(BR, d)}
    raise ValueError(cls)


def b_triples():
    """77 evaluation triples over four relations plus one with a single query
    (a TransR group of its own), and the positive set: the triples and 300
    known heads of the first one's (r, t)."""
    rng = np.random.default_rng(2024)
    X = np.stack([rng.integers(0, BE, BN), rng.integers(0, BR - 1, BN), rng.integers(0, BE, BN)], 1).astype(np.int64)
    X[40, 1] = BR - 1
    hub = np.stack([rng.permutation(BE)[:300], np.full(300, X[0, 1]), np.full(300, X[0, 2])], 1).astype(np.int64)
    return X, np.concatenate([X, hub])


def b_limit(key):
    """RotatE's limit (RotatE.py:73-77): (margin + 2) / k with the default loss's margin 3."""
    cls, ep, _, _, _, _ = BMODELS[key]
    return (3.0 + 2.0) / ep["embedding_size"] if cls == "RotatE" else None


def b_oracle(key, side):
    from oracle import kge_oracle as orc
    cls, _, sc, kw, _, _ = BMODELS[key]
    X, P = b_triples()
    return orc.filtered_ranks(cls, b_weights(key), X, side, P, score=sc if sc is not None else ("dot", 0.0),
                              limit=b_limit(key), constraint=bool(kw.get("constraint", False)))


def transd_norms(key):
    """Norms of every query's projected candidates (the clip's branch variable), float64."""
    W = {k: v.astype(np.float64) for k, v in b_weights(key).items()}
    X, _ = b_triples()
    de = np.sum(W["ent_proj"] * W["ent_emb"], axis=1)
    kr, ke = W["rel_emb"].shape[1], W["ent_emb"].shape[1]
    xe = np.zeros((BE, kr))
    xe[:, :min(kr, ke)] = W["ent_emb"][:, :min(kr, ke)]
    return np.stack([np.linalg.norm(W["rel_proj"][r][None, :] * de[:, None] + xe, axis=1) for r in np.unique(X[:, 1])])


def _b_model(key):
    from KGE import score
    from tests.test_plugin_surface import build
    cls, ep, sc, kw, _, _ = BMODELS[key]
    m = build(cls, None if sc is None else score.LpDistance(sc[1]), embedding_params=ep, **kw)
    m.metadata = {"ind2ent": list(range(BE)), "ind2rel": list(range(BR))}
    dev = torch.device("cuda", 0)
    m.model_weights = {k: torch.tensor(v, device=dev) for k, v in b_weights(key).items()}
    return m


@pytest.mark.parametrize("key", list(BMODELS))
def test_float_ranks_match_oracle(key):
    """E = 1031 (five lane chunks), n = 77, filtered by the triples and a
    300-head hub, both sides, the four variants: identical to each other, equal
    to the float64 oracle's ranks where it has no near-tie, within its near-tie
    count elsewhere -- and the oracle alone leaves at most 12 of 77 queries
    near-tied, so at least 65 ranks per side are compared exactly."""
    from KGE import _hip, ranking
    m = _b_model(key)
    assert ranking.supported(m)
    if hasattr(m, "limit") or BMODELS[key][0] == "RotatE":
        m._set_limit()
        assert m.limit == pytest.approx(b_limit(key))
    if key.endswith("-clip"):
        nr = transd_norms(key)
        assert (nr < 0.98).mean() > 0.05 and (nr >= 1.02).mean() > 0.05, ((nr < 1).mean(), (nr >= 1).mean())
    X, P = b_triples()
    for side in ("h", "t"):
        want, near = b_oracle(key, side)
        print(key, side, "queries with a near-tie:", int((near > 0).sum()), "of", BN)
        assert (near > 0).sum() <= NEAR_CAP, (side, near)
        assert (want > 1).any()
        runs = [ranking.batched_ranks(m, X, side, P, flags=f)
                for f in (0, _hip.RANK_FLAG_LANE_PASS, ranking.RESCORE_FILTER,
                          ranking.RESCORE_FILTER | _hip.RANK_FLAG_LANE_PASS)]
        for r in runs[1:]:
            assert np.array_equal(runs[0], r), (side, np.nonzero(runs[0] != r)[0][:10])
        got = runs[0]
        exact = near == 0
        bad = np.nonzero(got[exact] != want[exact])[0]
        assert bad.size == 0, (side, bad[:10], got[exact][bad][:10], want[exact][bad][:10])
        assert (np.abs(got - want) <= near).all(), (side, got, want, near)


def test_bitmap_size_fallback(monkeypatch):
    """Past ranking._BITS_MAX_BYTES the bitmap is not allocated and the
    library's rescoring filter pass runs: the same ranks."""
    from KGE import _hip, ranking
    m = _b_model("DistMult")
    X, P = b_triples()
    descs = []
    real = _hip.kge_rank_desc

    def spy():
        descs.append(real())
        return descs[-1]
    monkeypatch.setattr(ranking._hip, "kge_rank_desc", spy)
    want = ranking.batched_ranks(m, X, "h", P)
    assert descs[-1].filt_bits and descs[-1].filt_bits_words == BN * ((BE + 31) // 32)
    monkeypatch.setattr(ranking, "_BITS_MAX_BYTES", BN * ((BE + 31) // 32) * 4 - 1)
    got = ranking.batched_ranks(m, X, "h", P)
    assert not descs[-1].filt_bits and descs[-1].filt_beg
    assert np.array_equal(got, want) and (want > 1).any()
