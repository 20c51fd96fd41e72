"""CPU: the top-k link prediction surface without a GPU -- kge_topk_desc's
ctypes mirror against gcc on the header, kge_topk's descriptor validation (no
kernel is launched for a refused descriptor) and KGEModel.predict's host
fallback (KGE_BACKEND=eager, CPU tensors) for every model class against a
direct numpy sort of score_hrt's output."""

import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests.test_plugin_surface import MODELS, build, toy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kge_hip.h")


def test_topk_desc_matches_c_layout():
    from KGE import _hip
    cls = _hip.kge_topk_desc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "kge_hip.h"', 'int main(void){',
             'printf("sizeof %zu\\n", sizeof(kge_topk_desc));',
             'printf("max_k %d\\n", (int)KGE_TOPK_MAX_K);',
             'printf("flag_lane %d\\n", (int)KGE_TOPK_FLAG_LANE_PASS);',
             'printf("flag_slab %d\\n", (int)KGE_TOPK_FLAG_DEBUG_SLAB);']
    for f, _ in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(kge_topk_desc, %s));' % (f, f))
    for f, _ in _hip.kge_rank_desc._fields_:
        lines.append('printf("q.%s %%zu\\n", offsetof(kge_topk_desc, q.%s));' % (f, f))
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        with open(c, "w") as f:
            f.write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-I", os.path.dirname(HEADER), c, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    lay = {l.split()[0]: int(l.split()[1]) for l in out.splitlines()}
    assert ctypes.sizeof(cls) == lay["sizeof"]
    for f, _ in cls._fields_:
        assert getattr(cls, f).offset == lay[f], f
    for f, _ in _hip.kge_rank_desc._fields_:
        assert cls.q.offset + getattr(_hip.kge_rank_desc, f).offset == lay["q." + f], f
    assert (_hip.TOPK_MAX_K, _hip.TOPK_FLAG_LANE_PASS, _hip.TOPK_FLAG_DEBUG_SLAB) == \
        (lay["max_k"], lay["flag_lane"], lay["flag_slab"])


def _desc(**kw):
    """A valid descriptor over host memory (never launched: every test below
    breaks it first or only asks for the workspace size)."""
    from KGE import _hip
    buf = (ctypes.c_float * 2048)()
    addr = ctypes.addressof(buf)
    d = _hip.kge_topk_desc()
    d.q.abi_version = _hip.ABI_VERSION
    d.q.mode, d.q.proj, d.q.corrupt_side = _hip.RANK_TRANS, _hip.RPROJ_NONE, _hip.SIDE_T
    d.q.cand = _hip.kge_table(addr, 10, 4, 4)
    d.q.dim, d.q.q0, d.q.ldq = 4, addr, 4
    d.q.idx_dtype, d.q.score_kind, d.q.score_p, d.q.n = _hip.IDX_I64, 0, 2.0, 2
    d.k, d.flags = 3, 0
    d.ids_out, d.scores_out = addr, addr
    d.workspace, d.workspace_bytes = addr, ctypes.sizeof(buf)
    for key, v in kw.items():
        obj = d
        *path, last = key.split("__")
        for p in path:
            obj = getattr(obj, p)
        setattr(obj, last, v)
    return d, buf


def test_topk_workspace_bytes(hiplib):
    d, _keep = _desc()
    need = hiplib.kge_topk_workspace_bytes(ctypes.byref(d))
    assert need >= 2 * 3 * 8          # at least the answer's keys
    assert need <= ctypes.sizeof(_keep)
    d2, _keep2 = _desc(flags=2)       # 256-candidate slabs: one slab at E = 10, the same size
    assert hiplib.kge_topk_workspace_bytes(ctypes.byref(d2)) == need
    d3, _keep3 = _desc(q__cand=_table257(_keep), flags=2)
    assert hiplib.kge_topk_workspace_bytes(ctypes.byref(d3)) == 2 * 2 * 3 * 8   # E = 257: two slabs


def _table257(buf):
    from KGE import _hip
    return _hip.kge_table(ctypes.addressof(buf), 257, 4, 4)


EINVAL, ENOMEM, EUNSUP = 1, 4, 5


@pytest.mark.parametrize("kw,status,msg", [
    ({"k": 0}, EINVAL, "k = 0"),
    ({"k": 1025}, EINVAL, "k = 1025"),
    ({"ids_out": None}, EINVAL, "null ids_out"),
    ({"scores_out": None}, EINVAL, "null ids_out"),
    ({"workspace": None}, EINVAL, "null ids_out"),
    ({"q__filt_beg": 1, "q__filt_end": 1, "q__filt_ent": 1}, EINVAL, "filt_bits"),
    ({"flags": 4}, EINVAL, "unknown flags"),
    ({"q__flags": 1}, EINVAL, "q.flags"),
    ({"workspace_bytes": 8}, ENOMEM, "workspace"),
    ({"q__abi_version": 99}, EINVAL, "abi_version"),
    ({"q__mode": 9}, EINVAL, "rank mode"),
    ({"q__q0": None}, EINVAL, "null query rows"),
])
def test_topk_invalid_descriptors_are_rejected_without_gpu(hiplib, kw, status, msg):
    from KGE import _hip
    assert (EINVAL, ENOMEM, EUNSUP) == (_hip.KGE_EINVAL, 4, _hip.KGE_EUNSUPPORTED)
    if "q__filt_beg" in kw:
        base, _b = _desc()
        kw = {key: base.q.q0 for key in kw}      # any non-null address: the check comes first
    d, _keep = _desc(**kw)
    assert hiplib.kge_topk(ctypes.byref(d), None) == status
    assert msg in hiplib.kge_last_error().decode()
    if status == EINVAL and "ids_out" not in msg:
        assert hiplib.kge_topk_workspace_bytes(ctypes.byref(d)) == 0


def test_topk_ignored_pointers_may_be_null(hiplib):
    """true_ids / rank_out / pos_score_out are not needed: the descriptor is
    valid without them (kge_rank refuses the same one)."""
    d, _keep = _desc()
    assert not d.q.true_ids and not d.q.rank_out and not d.q.pos_score_out
    assert hiplib.kge_topk_workspace_bytes(ctypes.byref(d)) > 0
    assert hiplib.kge_rank(ctypes.byref(d.q), None) == EINVAL


# ---------------------------------------------------------------- predict, host fallback
@pytest.fixture
def _eager(monkeypatch):
    monkeypatch.setenv("KGE_BACKEND", "eager")


def _model(name):
    train, val, md = toy()
    m = build(name)
    m._model_weights_initial = None
    m.metadata = md
    m._init_embeddings(seed=None)
    return m, train, val


def _want(m, x, side, k, P):
    """A direct sort of score_hrt's scores: filtered entities dropped, score
    descending, ties by ascending id."""
    with torch.no_grad():
        s = m.score_hrt(None, x[1], x[2]) if side == "h" else m.score_hrt(x[0], x[1], None)
    s = np.asarray(s.reshape(-1).cpu().numpy(), dtype=np.float32)
    keep, corrupt = (2, 0) if side == "h" else (0, 2)
    drop = set() if P is None else set(P[(P[:, 1] == x[1]) & (P[:, keep] == x[keep]), corrupt].tolist())
    rows = sorted((-float(s[e]), e) for e in range(len(s)) if e not in drop)[:k]
    ids = np.full(k, -1, dtype=np.int64)
    sc = np.full(k, -np.inf, dtype=np.float32)
    ids[:len(rows)] = [e for _, e in rows]
    sc[:len(rows)] = [s[e] for _, e in rows]
    return ids, sc


@pytest.mark.parametrize("name", MODELS)
def test_predict_eager_matches_sorted_scores(_eager, name):
    m, train, val = _model(name)
    E = len(m.metadata["ind2ent"])
    allp = np.concatenate((train, val), axis=0)
    hit = False
    for side in ("h", "t"):
        for P in (None, allp):
            for k in (1, 3, E + 5):
                ids, sc = m.predict(val, side, k=k, positive_X=P)
                assert ids.shape == (len(val), k) and ids.dtype == np.int64
                assert sc.shape == (len(val), k) and sc.dtype == np.float32
                for i, x in enumerate(val):
                    wi, ws = _want(m, x, side, k, P)
                    assert np.array_equal(ids[i], wi), (name, side, k, i)
                    assert np.array_equal(sc[i], ws), (name, side, k, i)
                if k > E:
                    assert (ids[:, E:] == -1).all() and np.isneginf(sc[:, E:]).all()
                    hit |= P is not None and bool((ids[:, E - 1] == -1).any())
    assert hit, "no query of the toy KG has a filtered entity"


def test_predict_ignores_the_corrupted_column(_eager):
    m, train, val = _model("TransE")
    for side, col in (("h", 0), ("t", 2)):
        X = val.copy()
        X[:, col] = -1
        got = m.predict(X, side, k=4, positive_X=train)
        want = m.predict(val, side, k=4, positive_X=train)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        one = m.predict(torch.as_tensor(X[0]), side, positive_X=train)   # a single triple, default k = 10
        assert one[0].shape == (1, 10) and np.array_equal(one[0][0, :4], want[0][0])


def test_predict_nan_and_ties(_eager):
    """The fallback's order on scores with ties, +-0 and NaN (a score function
    of the test's own): finite descending, ties by id, NaNs last by id."""
    m, _, val = _model("TransE")
    E = len(m.metadata["ind2ent"])
    s = np.zeros(E, dtype=np.float32)
    s[1], s[2], s[3], s[4], s[5] = np.nan, -0.0, 2.0, 2.0, np.nan
    s[6:] = -np.inf
    m.score_hrt = lambda h, r, t: torch.tensor(s)
    ids, sc = m.predict(val[:1], "t", k=E)
    want = [3, 4, 0, 2] + list(range(6, E)) + [1, 5]
    assert ids[0].tolist() == want
    assert np.isnan(sc[0, -2:]).all() and not np.isnan(sc[0, :-2]).any()
    with pytest.raises(ValueError):
        m.predict(val, "x")
    with pytest.raises(ValueError):
        m.predict(val, "t", k=0)
