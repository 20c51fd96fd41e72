"""Device time of top-k link prediction on the evaluation shape.

The C2 model shape (TransE, d = 200, LpDistance(2), every entity of the graph) over the 17,526
FB15k-237 validation triples, filtered by train + valid, both sides, k = 10 and
100. Timed with HIP events in one process, 3 warm-ups then the median of 20:

  (a) kge_topk, default producer
  (b) kge_topk, KGE_TOPK_FLAG_LANE_PASS
  (c) kge_rank on the same queries (scoring only: the floor)
  (d) PyTorch: the [chunk, E] score matrix from the model's score function,
      filtered entries at -inf, then torch.topk

and prints one JSON line with the four numbers and the ratios (a)/(c), (d)/(a).

    python tools/topk_time.py [--repeats 20] [--warmup 3] [--chunk 128]
"""

import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "knowledge-graph-embedding_amd"))


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=128, help="queries per score matrix of the PyTorch route")
    args = ap.parse_args()

    import __graft_entry__
    __graft_entry__.build()
    from KGE import _hip, ranking, score
    from KGE.models.translating_based.TransE import TransE
    from KGE.ns_strategy import UniformStrategy

    z = np.load(os.path.join(ROOT, "data", "fb15k237_train.npz"))
    train, E, R = z["triples"].astype(np.int64), int(z["n_entities"]), int(z["n_relations"])
    V = np.load(os.path.join(ROOT, "data", "fb15k237_valid.npz"))["triples"].astype(np.int64)
    P = np.concatenate([train, V])
    d = 200
    model = TransE({"embedding_size": d}, 8, "h+t", score_fn=score.LpDistance(2),
                   ns_strategy=UniformStrategy(np.arange(E), seed=1), constraint=True)
    model.metadata = {"ind2ent": list(range(E)), "ind2rel": list(range(R))}
    model._model_weights_initial = None
    model._init_embeddings(seed=12345)
    model._to_device()
    assert ranking.supported(model)
    dev = model.model_weights["ent_emb"].device
    lib, stream = _hip.lib(), _hip.stream_handle(dev)
    ent, rel = model.model_weights["ent_emb"].detach(), model.model_weights["rel_emb"].detach()
    n, W = len(V), (E + 31) // 32
    X = torch.as_tensor(V, device=dev)
    out = {"shape": {"model": "TransE", "d": d, "E": E, "n": n, "score": "LpDistance(2)"},
           "repeats": args.repeats, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}

    for side in ("h", "t"):
        with torch.no_grad():
            g = ranking._q_transe(model, X[:, 0], X[:, 1], X[:, 2], side)[0]
        q0 = g["q0"].to(torch.float32).contiguous()
        q1 = g["q1"].to(torch.float32).contiguous() if g["q1"] is not None else None
        fkeys, fent = ranking.cached_filter_keys(P, side, E, dev)
        fb, fe = ranking.filter_lookup(X, fkeys, fent, side, E)
        bits = torch.empty(n * W, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        true_ids = X[:, 0 if side == "h" else 2].contiguous()
        ranks = torch.zeros(n, dtype=torch.int64, device=dev)
        pos = torch.zeros(n, dtype=torch.float32, device=dev)

        def rank_desc(q):
            q.abi_version = _hip.ABI_VERSION
            q.mode, q.proj = g["mode"], g["proj"]
            q.corrupt_side = _hip.SIDE_H if side == "h" else _hip.SIDE_T
            q.cand = _hip.table(g["cand"])
            q.dim, q.clip = g["dim"], 0
            q.q0, q.q1, q.ldq = q0.data_ptr(), q1.data_ptr() if q1 is not None else None, q0.shape[1]
            q.idx_dtype = _hip.IDX_I64
            q.score_kind, q.score_p = g["score"]
            q.n = n
            q.filt_beg, q.filt_end, q.filt_ent = fb.data_ptr(), fe.data_ptr(), fent.data_ptr()
            q.filt_bits, q.filt_bits_words = bits.data_ptr(), bits.numel()
            q.status = status.data_ptr()

        rd = _hip.kge_rank_desc()
        rank_desc(rd)
        rd.true_ids, rd.rank_out, rd.pos_score_out = true_ids.data_ptr(), ranks.data_ptr(), pos.data_ptr()
        c_ms = timed(lambda: _hip.check(lib.kge_rank(ctypes.byref(rd), stream), "kge_rank"), args.warmup, args.repeats)

        # (d): what a user writes without kge_topk
        beg, end = fb.cpu().numpy(), fe.cpu().numpy()
        rows = torch.as_tensor(np.repeat(np.arange(n), end - beg), device=dev)
        cols = torch.cat([fent[b:e] for b, e in zip(beg.tolist(), end.tolist())]) if n else fent[:0]
        row_beg = np.concatenate([[0], np.cumsum(end - beg)])

        for k in (10, 100):
            ids = torch.empty((n, k), dtype=torch.int64, device=dev)
            sc = torch.empty((n, k), dtype=torch.float32, device=dev)
            res = {}
            for name, flags in (("a_topk_ms", 0), ("b_topk_lane_ms", _hip.TOPK_FLAG_LANE_PASS)):
                td = _hip.kge_topk_desc()
                rank_desc(td.q)
                td.k, td.flags = k, flags
                td.ids_out, td.scores_out = ids.data_ptr(), sc.data_ptr()
                need = int(lib.kge_topk_workspace_bytes(ctypes.byref(td)))
                ws = torch.empty(need, dtype=torch.uint8, device=dev)
                td.workspace, td.workspace_bytes = ws.data_ptr(), need
                res[name] = timed(lambda: _hip.check(lib.kge_topk(ctypes.byref(td), stream), "kge_topk"),
                                  args.warmup, args.repeats)
                res[name.replace("_ms", "_workspace_mb")] = round(need / 2 ** 20, 2)
            native_ids = ids.clone()

            tids = torch.empty_like(ids)

            def torch_route():
                with torch.no_grad():
                    for c0 in range(0, n, args.chunk):
                        c1 = min(n, c0 + args.chunk)
                        if side == "t":
                            a, b = (ent[X[c0:c1, 0]] + rel[X[c0:c1, 1]]).unsqueeze(1), ent.unsqueeze(0)
                        else:
                            a, b = ent.unsqueeze(0) + rel[X[c0:c1, 1]].unsqueeze(1), ent[X[c0:c1, 2]].unsqueeze(1)
                        s = model.score_fn(a, b)
                        lo, hi = int(row_beg[c0]), int(row_beg[c1])
                        s[rows[lo:hi] - c0, cols[lo:hi]] = float("-inf")
                        tids[c0:c1] = torch.topk(s, k, dim=1).indices
            res["d_torch_ms"] = timed(torch_route, args.warmup, args.repeats)
            res["c_rank_ms"] = c_ms
            res["a_over_c"] = round(res["a_topk_ms"] / c_ms, 3)
            res["d_over_a"] = round(res["d_torch_ms"] / res["a_topk_ms"], 3)
            # sanity, not a test: the two routes name the same entities but for fp32 near-ties
            res["rows_same_set_as_torch"] = round(float(
                (torch.sort(native_ids, 1).values == torch.sort(tids, 1).values).all(1).float().mean()), 4)
            out["%s_k%d" % (side, k)] = {kk: (round(v, 4) if isinstance(v, float) else v) for kk, v in res.items()}
        _hip.check_device_status(status, "topk_time")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
