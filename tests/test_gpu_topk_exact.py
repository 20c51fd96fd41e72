"""GPU: kge_topk (csrc/kge_topk.hip) held to exact answers.

The C-ABI is driven with rows of small integers (tests/rank_int_ref.py): every
fp32 operation of the scoring functions is then exact, so the reference is a
plain numpy lexsort on (id, value) with the filtered ids removed, and ids,
counts and padding must be equal with no tolerance. Values in {-2..2} make
most scores tie, so the id tie-break decides at every position. Every case
runs through both producers (KGE_TOPK_FLAG_LANE_PASS) with whole-table and
256-candidate slabs (KGE_TOPK_FLAG_DEBUG_SLAB): the four must agree bit for
bit. Outputs, bitmap and workspace are prefilled with garbage before each run."""

import ctypes

import numpy as np
import pytest
import torch

from tests import rank_int_ref as ref
from tests.rank_int_ref import NONE, TRANS
from tests.test_gpu_rank_exact import MODES, SCORE, DevCase, _dev_case, _kinds

pytestmark = pytest.mark.gpu

LANE, SLAB = 1, 2                    # KGE_TOPK_FLAG_*
VARIANTS = (0, LANE, SLAB, LANE | SLAB)
KEYS = ("trans", "hyper", "rank1", "rot", "mul", "dot")


@pytest.fixture(autouse=True)
def _gpu(hiplib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def run_topk(dc, kind, k, flags=0, n=None, filt=True):
    """-> (return code, ids [n, k], scores [n, k], counts [n], status word)."""
    from KGE import _hip
    c = dc.case
    n = c.n if n is None else n
    ids = torch.full((c.n, k), 0x5A5A5A5A, dtype=dc.idt, device=dc.dev)
    sc = torch.full((c.n, k), float("nan"), dtype=torch.float32, device=dc.dev)
    cnt = torch.full((c.n,), -7, dtype=torch.int32, device=dc.dev)
    status = torch.zeros(1, dtype=torch.int32, device=dc.dev)
    d = _hip.kge_topk_desc()
    d.q.abi_version = _hip.ABI_VERSION
    d.q.mode, d.q.proj = c.mode, c.proj
    d.q.corrupt_side = _hip.SIDE_H if c.side == "h" else _hip.SIDE_T
    d.q.cand = _hip.table(dc.cand[1])
    if dc.aux is not None:
        d.q.cand_aux = _hip.table(dc.aux[1])
    d.q.dim, d.q.clip = c.dim, 0
    d.q.q0 = dc.q0[0].data_ptr()
    d.q.q1 = dc.q1[0].data_ptr() if dc.q1 is not None else None
    d.q.qw = dc.qw[0].data_ptr() if dc.qw is not None else None
    d.q.ldq = dc.q0[0].shape[1]
    d.q.idx_dtype = _hip.IDX_I32 if dc.idt == torch.int32 else _hip.IDX_I64
    d.q.score_kind, d.q.score_p = SCORE[kind]
    d.q.n = n
    bits = None
    if dc.lists is not None and filt:
        d.q.filt_beg, d.q.filt_end, d.q.filt_ent = dc.fb.data_ptr(), dc.fe.data_ptr(), dc.fent.data_ptr()
        bits = torch.full((c.n * dc.W,), -1, dtype=torch.int32, device=dc.dev)
        d.q.filt_bits, d.q.filt_bits_words = bits.data_ptr(), bits.numel()
    d.q.status = status.data_ptr()
    d.k, d.flags = k, flags
    d.ids_out, d.scores_out, d.count_out = ids.data_ptr(), sc.data_ptr(), cnt.data_ptr()
    lib = _hip.lib()
    need = int(lib.kge_topk_workspace_bytes(ctypes.byref(d)))
    assert need > 0 or n == 0, lib.kge_last_error()
    ws = torch.full((max(need, 8),), 0xFF, dtype=torch.uint8, device=dc.dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), need
    rc = lib.kge_topk(ctypes.byref(d), _hip.stream_handle(dc.dev))
    torch.cuda.synchronize()
    return rc, ids.cpu().numpy().astype(np.int64), sc.cpu().numpy(), cnt.cpu().numpy(), int(status.item())


def reference(case, kind, lists):
    """Per query (ids, values) of every live candidate, best first, ties by id."""
    out = []
    for q in range(case.n):
        V, lower = case.values(kind, q)
        live = np.ones(case.E, dtype=bool)
        if lists is not None:
            live[lists[q]] = False
        ids = np.nonzero(live)[0]
        v = V[ids]
        o = np.lexsort((ids, v if lower else -v))
        out.append((ids[o], v[o]))
    return out


def compare(tag, kind, k, got, want):
    ids, sc, cnt = got
    for q, (wi, wv) in enumerate(want):
        c = min(k, len(wi))
        assert cnt[q] == c, (tag, q, cnt[q], c)
        assert np.array_equal(ids[q, :c], wi[:c]), (tag, q, ids[q, :c][:12], wi[:12])
        ws = np.array([ref.pos_score(kind, int(v)) for v in wv[:c]], dtype=np.float64)
        if kind in ("p2", "pow2"):   # sqrtf and one multiply: <= 2^-22 relative
            assert np.allclose(sc[q, :c], ws, rtol=1e-6, atol=0), (tag, q)
        else:
            assert np.array_equal(sc[q, :c].astype(np.float64), ws), (tag, q, sc[q, :c][:12], ws[:12])
        assert (ids[q, c:] == -1).all() and np.isneginf(sc[q, c:]).all(), (tag, q)


def check(dc, ks, kinds=None, filt=True):
    """Every kind x k: the four variants equal bit for bit, and equal to the
    integer reference. -> the last variant-0 result."""
    from KGE import _hip
    c = dc.case
    last = None
    for kind in (_kinds(c.mode) if kinds is None else kinds):
        want = reference(c, kind, dc.lists if filt else None)
        for k in ks:
            tag = (c.mode, c.proj, c.side, c.E, c.n, c.dim, kind, k)
            runs = []
            for flags in VARIANTS:
                rc, ids, sc, cnt, status = run_topk(dc, kind, k, flags, filt=filt)
                assert rc == _hip.KGE_OK and status == 0, (tag, flags, rc, status, _hip.lib().kge_last_error())
                runs.append((ids, sc, cnt))
            for flags, r in zip(VARIANTS[1:], runs[1:]):
                assert np.array_equal(r[0], runs[0][0]), (tag, flags)
                assert np.array_equal(r[1].view(np.uint32), runs[0][1].view(np.uint32)), (tag, flags)
                assert np.array_equal(r[2], runs[0][2]), (tag, flags)
            compare(tag, kind, k, runs[0], want)
            last = runs[0]
    return last


DIMS = [(k, d) for k in ("trans", "hyper", "rank1", "mul", "dot") for d in (3, 16, 17, 33)] + [("rot", 2), ("rot", 18)]


@pytest.mark.parametrize("key,dim", DIMS)
def test_topk_modes_and_dims(key, dim):
    """Every (mode, projection, side) x its score kinds at E = 257 (two lane
    chunks, five tiles, two debug slabs with one candidate in the last), n = 9
    (one query past a lane group), row widths below a float4, one staged chunk,
    a chunk and one, two chunks and one (RotatE: 2 and 18)."""
    rng = np.random.default_rng(2000 + dim)
    for side in ("h", "t"):
        check(_dev_case(rng, key, side, 257, 9, dim), ks=(1, 10))


SIZES = [(1, 1), (63, 7), (64, 8), (65, 65), (255, 9), (256, 9), (257, 9), (1031, 77)]


@pytest.mark.parametrize("E,n", SIZES)
def test_topk_sizes(E, n):
    """E and n around the tile (64), the lane group (8) and the lane chunk /
    debug slab (256), every mode and side with one score kind each in turn;
    k = 1, 2, one tile, past the tiled producer's limit, and the largest (two
    queries per lane group) -- k > E and k > E - |filter| included."""
    rng = np.random.default_rng(E * 137 + n)
    for i, (key, dim) in enumerate([("trans", 17), ("hyper", 20), ("rank1", 16), ("rot", 18), ("mul", 17),
                                    ("dot", 20)]):
        for j, side in enumerate(("h", "t")):
            kinds = _kinds(MODES[key][0])
            check(_dev_case(rng, key, side, E, n, dim), ks=(1, 2, 64, 100, 1024),
                  kinds=(kinds[(i + j + E + n) % len(kinds)],))


class WideCase(DevCase):
    """DevCase for integer rows beyond int8 (still exact in fp32)."""

    def _rows(self, a, pad):
        if a is None:
            return None
        assert np.abs(a).max(initial=0) < (1 << 20)
        t = torch.from_numpy(np.ascontiguousarray(a.astype(np.float32))).to(self.dev)
        return t, t


@pytest.mark.parametrize("shape", ["increasing", "decreasing", "identical"])
def test_topk_threshold_machinery(shape):
    """E = 4099 (three slabs by default, seventeen debug slabs), n = 9, dim 2,
    p1: scores strictly increasing with the id (every candidate beats the
    threshold: the buffers fill and compact as often as they can), strictly
    decreasing (none does after the first k), and all rows identical (the
    answer is ids 0 .. k - 1 less the filtered ones)."""
    E, n = 4099, 9
    rng = np.random.default_rng(4099)
    cand = np.zeros((E, 2), dtype=np.int32)
    q0 = np.zeros((n, 2), dtype=np.int64)
    if shape == "identical":
        cand[:] = (1, -2)
        q0[:, 0] = np.arange(n)
    else:
        cand[:, 0] = np.arange(E)
        # t side, p1: score = -(|q0[0] - e| + |q0[1]|)
        q0[:, 0] = (E + 10 + np.arange(n)) if shape == "increasing" else -1 - np.arange(n)
        q0[:, 1] = np.arange(n)
    case = ref.Case(TRANS, NONE, "t", cand, q0, dim=2)
    ids = rng.integers(0, E, n)
    lists = ref.make_filter(rng, E, n, ids)
    dc = WideCase(case, ids, lists)
    for filt in (True, False):
        got = check(dc, ks=(1, 2, 10), kinds=("p1",), filt=filt)
        if not filt:
            want = {"increasing": np.arange(E - 1, E - 11, -1), "decreasing": np.arange(10),
                    "identical": np.arange(10)}[shape]
            assert (got[0] == want[None, :]).all()


@pytest.mark.parametrize("key,dim", [("trans", 17), ("hyper", 20), ("rank1", 20), ("rot", 18), ("mul", 33),
                                     ("dot", 3)])
def test_topk_padded_rows(key, dim):
    """cand.ld = cols + 3 and ldq = dim + 5 with NaN in the padding (the aux
    table too): no producer may read past a row's values."""
    rng = np.random.default_rng(78 + dim)
    for side in ("h", "t"):
        dc = _dev_case(rng, key, side, 257, 9, dim, cols=12 if key == "rank1" else None, pad=True)
        assert torch.isnan(dc.cand[0][:, -3:]).all() and torch.isnan(dc.q0[0][:, -5:]).all()
        check(dc, ks=(10,), kinds=_kinds(MODES[key][0])[:2])


@pytest.mark.parametrize("key", KEYS)
def test_topk_int32_ids(key):
    """idx_dtype = KGE_IDX_I32: int32 ids_out and filt_ent."""
    rng = np.random.default_rng(33)
    for side in ("h", "t"):
        check(_dev_case(rng, key, side, 1031, 9, 18 if key == "rot" else 17, idx32=True), ks=(10,),
              kinds=_kinds(MODES[key][0])[:1])


def test_topk_global_atomics_bitmap():
    """E = 262,145: ceil(E / 32) = 8193 words per query, the first size built
    with global atomics after a clear (the buffer comes in as all ones: a
    missing clear leaves every candidate filtered), feeding both producers."""
    rng = np.random.default_rng(262145)
    for side in ("h", "t"):
        dc = _dev_case(rng, "trans", side, 262145, 10, 8)
        assert 262144 in dc.lists[1] and len(dc.lists[-1]) > 256
        check(dc, ks=(10,), kinds=("p1",))


@pytest.mark.parametrize("key", KEYS)
def test_topk_consistent_with_kge_rank(key):
    """Each returned id fed back to kge_rank as the true entity, same filter:
    pos_score_out has the bits of scores_out, and the rank is 1 + the number
    of entries of the row with a strictly greater score."""
    from KGE import _hip
    rng = np.random.default_rng(55)
    k = 10
    for side in ("h", "t"):
        dc = _dev_case(rng, key, side, 257, 9, 18 if key == "rot" else 17)
        kind = _kinds(MODES[key][0])[-1]
        ids, sc, cnt = check(dc, ks=(k,), kinds=(kind,))
        assert (cnt == k).sum() >= 8     # (the last query's hub filters every entity of so small a table)
        for j in range(k):
            ok = ids[:, j] >= 0
            dc.ids = torch.as_tensor(np.where(ok, ids[:, j], 0), device=dc.dev).to(dc.idt)
            rc, rk, pos, status, _ = dc.run(kind, 0, bitmap=True)
            assert rc == _hip.KGE_OK and status == 0
            assert np.array_equal(pos.view(np.uint32)[ok], sc[:, j].view(np.uint32)[ok]), (key, side, j)
            assert np.array_equal(rk[ok], 1 + (sc > sc[:, j:j + 1]).sum(axis=1)[ok]), (key, side, j)


def test_topk_signed_zero_scores():
    """pinf at dim 2 in {-2..2}: a candidate equal to the query's row scores a
    zero distance, whose sign kge_rank keeps; kge_topk returns the same bits,
    and the zeros tie by id ahead of everything else."""
    from KGE import _hip
    rng = np.random.default_rng(0)
    dc = _dev_case(rng, "trans", "t", 257, 9, 2)
    ids, sc, cnt = check(dc, ks=(10,), kinds=("pinf",))
    assert (sc == 0).any()
    for j in range(10):
        ok = ids[:, j] >= 0
        dc.ids = torch.as_tensor(np.where(ok, ids[:, j], 0), device=dc.dev).to(dc.idt)
        rc, rk, pos, status, _ = dc.run("pinf", 0, bitmap=True)
        assert rc == _hip.KGE_OK and np.array_equal(pos.view(np.uint32)[ok], sc[:, j].view(np.uint32)[ok])


def test_topk_nan_scores_order_last():
    """Two NaN rows among 300, Dot scores (a sum carries the NaN through; the
    Lp kinds clamp it away with fmaxf, in kge_rank as here): they come after
    every other live candidate (below -inf), in id order, as NaN; with k below
    the live count they do not appear at all."""
    from KGE import _hip
    rng = np.random.default_rng(300)
    E, n = 300, 9
    for key, kind in (("trans", "dot"), ("hyper", "dot"), ("mul", "dot")):
        dc = _dev_case(rng, key, "t", E, n, 17)
        lists = [np.setdiff1d(l, [7, 100]) for l in dc.lists]   # the NaN rows stay live for every query
        dc = DevCase(dc.case, dc.ids_np, lists)
        want = reference(dc.case, kind, lists)
        dc.cand[0][7, :] = float("nan")
        dc.cand[0][100, :] = float("nan")
        runs = []
        for flags in VARIANTS:
            rc, ids, sc, cnt, status = run_topk(dc, kind, E, flags)
            assert rc == _hip.KGE_OK and status == 0
            runs.append((ids, sc.view(np.uint32), cnt))
            for q in range(n):
                wi = np.array([e for e in want[q][0] if e not in (7, 100)] + [7, 100])
                assert cnt[q] == len(wi) and np.array_equal(ids[q, :len(wi)], wi), (key, flags, q)
                assert np.isnan(sc[q, len(wi) - 2:len(wi)]).all() and not np.isnan(sc[q, :len(wi) - 2]).any()
                assert (ids[q, len(wi):] == -1).all() and np.isneginf(sc[q, len(wi):]).all()
            rc, ids5, sc5, cnt5, _ = run_topk(dc, kind, 5, flags)
            assert np.array_equal(ids5, ids[:, :5]) and np.array_equal(cnt5, np.minimum(cnt, 5))
            assert np.array_equal(sc5.view(np.uint32), sc[:, :5].view(np.uint32))
            # (the last query's hub filters all but the two NaN rows)
            assert not np.isnan(sc5[cnt >= 7]).any() and (cnt >= 7).sum() >= n - 1
        for r in runs[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(r, runs[0]))


def test_topk_status_paths():
    """A filter id equal to E sets KGE_ERANGE in the status word (the call
    returns OK) and leaves the other queries right; n = 0 returns OK and
    touches nothing."""
    from KGE import _hip
    rng = np.random.default_rng(9)
    for key in ("trans", "hyper"):
        dc = _dev_case(rng, key, "t", 257, 9, 17)
        want = reference(dc.case, "p1", dc.lists)
        bad = [l.copy() for l in dc.lists]
        bad[4] = np.append(bad[4], 257)
        dcb = DevCase(dc.case, dc.ids_np, bad)
        for flags in VARIANTS:
            rc, ids, sc, cnt, status = run_topk(dcb, "p1", 10, flags)
            assert rc == _hip.KGE_OK and status == _hip.KGE_ERANGE
            keep = [q for q in range(9) if q != 4]
            compare((key, flags), "p1", 10, (ids[keep], sc[keep], cnt[keep]), [want[q] for q in keep])
            rc, ids, sc, cnt, status = run_topk(dc, "p1", 10, flags, n=0)
            assert rc == _hip.KGE_OK and status == 0
            assert (ids == 0x5A5A5A5A).all() and np.isnan(sc).all() and (cnt == -7).all()
