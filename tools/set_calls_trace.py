"""The set calls of one small set, once each, as the program of a kernel trace: what a change of the host side of these calls
must leave as it was is the ORDER of the kernels each call launches.

The all-pairs calls (the default): cluster_rate's planted set at n = 200, s = 1000, k = 21, under MHX_TRI_QBATCH=48 (several
blocks per reference slice, several slices):

    dist_triangle, dist_triangle_edges and dist_cluster at 0.05, dist_mst recomputed (MHX_MST_STORE=0), then stored (=1),
    dist_linkage complete and average, dist_nj, dist_nj_support with 3 replicates, dist_medoids on the labels of that
    dist_cluster, dist_to on those medoids, resample_rows, and dist_cluster and dist_mst once more with device pointers

The query-by-reference calls (--pairs): 150 queries derived from that set against it, device pointers, under
MHX_SEARCH_QBATCH=48 and MHX_WITHIN_QBATCH=48 (four query batches by seven slices), MHX_WITHIN_CELLS=420 (three super-batches):

    dist_search (top 5, with the distances), dist_within storing and counting at 0.05, dist_contain, dist_contain_winner,
    dist_contain_search (top 5) -- and all of them once more under MHX_DIST_GENERIC=1

One line per call with a digest of what it returned, so that two libraries (MHX_LIB) can be compared by their output too.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/set_calls_trace.py [--pairs]
    python3 tools/set_calls_trace.py --names DIR/.../*_kernel_trace.csv     the kernel names of such a trace in launch order
"""
import csv
import hashlib
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def names(path):
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id") or 0)))
    return [r["Kernel_Name"].split("(")[0] for r in rows]


def digest(parts):
    h = hashlib.sha256()
    for part in parts:
        h.update(getattr(part, "tobytes", lambda: repr(part).encode())())
    return h.hexdigest()[:16]


def all_pairs():
    os.environ["MHX_TRI_QBATCH"] = "48"
    import torch  # noqa: F401  before the engine's library: the two then share one device runtime

    from auriclass_amd import engine
    from cluster_rate import make_set

    engine.init(0)
    rows, lens, _ = make_set(200, 1000, seed=1200)
    calls = [("dist_triangle", None, lambda: engine.dist_triangle(rows, lens, 21, 1000)),
             ("dist_triangle_edges 0.05", None, lambda: engine.dist_triangle_edges(rows, lens, 21, 1000, 0.05)),
             ("dist_cluster 0.05", None, lambda: engine.dist_cluster(rows, lens, 21, 1000, 0.05)),
             ("dist_mst recomputed", "0", lambda: engine.dist_mst(rows, lens, 21, 1000)),
             ("dist_mst stored", "1", lambda: engine.dist_mst(rows, lens, 21, 1000))]
    got = {}   # what a traced call returned, for the calls that go on from it
    for what, store, call in calls:
        if store is not None:
            os.environ["MHX_MST_STORE"] = store
        got[what] = call()
        print(f"{what}: {digest(got[what])}", flush=True)
    del os.environ["MHX_MST_STORE"]
    label = got["dist_cluster 0.05"][0]
    more = [("dist_linkage complete", lambda: engine.dist_linkage(rows, lens, 21, 1000, "complete")),
            ("dist_linkage average", lambda: engine.dist_linkage(rows, lens, 21, 1000, "average")),
            ("dist_nj", lambda: engine.dist_nj(rows, lens, 21, 1000)),
            ("dist_nj_support 3", lambda: engine.dist_nj_support(rows, lens, 21, 1000, 3)),
            ("dist_medoids", lambda: engine.dist_medoids(rows, lens, 21, 1000, label)),
            ("dist_to the medoids", lambda: engine.dist_to(rows, lens, 21, 1000, got["dist_medoids"][0])),
            ("resample_rows", lambda: engine.resample_rows(rows, lens, 1000, 42, 0, 0.5)),
            ("dist_cluster 0.05 device", lambda: device_forms(engine, rows, lens, "cluster")),
            ("dist_mst device", lambda: device_forms(engine, rows, lens, "mst"))]
    for what, call in more:
        got[what] = call()
        print(f"{what}: {digest(got[what])}", flush=True)


def device_forms(engine, rows, lens, which):
    """dist_cluster at 0.05 or dist_mst of the set with everything on the device; the tree's edges sorted, since they arrive in any order"""
    import numpy as np
    import torch

    dev = torch.device("cuda")
    n, stride = rows.shape
    d_rows = torch.from_numpy(np.ascontiguousarray(rows).view(np.int64)).to(dev)
    d_len = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint32).view(np.int32)).to(dev)
    if which == "cluster":
        label, degree = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        counts = engine.dist_cluster_device(d_rows.data_ptr(), d_len.data_ptr(), n, stride, 21, 1000, 0.05, label.data_ptr(), degree.data_ptr())
        return [counts, label.cpu().numpy(), degree.cpu().numpy()]
    out = [torch.zeros(n - 1, dtype=torch.int32, device=dev) for _ in range(4)]
    m = engine.dist_mst_device(d_rows.data_ptr(), d_len.data_ptr(), n, stride, 21, 1000, *[o.data_ptr() for o in out])
    return [m, sorted(zip(*[o.cpu().numpy().tolist() for o in out]))]


def query_sets():
    """(Q, q_len, R, r_len) as numpy: the planted set as references; a query is a reference with a share of its hashes replaced"""
    import numpy as np
    from cluster_rate import make_set

    R, r_len, _ = make_set(200, 1000, seed=1200)
    rng = np.random.default_rng(150)
    Q = np.zeros((150, R.shape[1]), np.uint64)
    for i in range(150):
        row = R[(7 * i) % 200, :1000].copy()
        fresh = rng.random(1000) < 0.02 * (i % 9)
        row[fresh] = rng.integers(0, 2 ** 64 - 2 ** 12, size=int(fresh.sum()), dtype=np.uint64)
        Q[i, :1000] = np.sort(row)
    return Q, np.full(150, 1000, np.uint32), R, np.asarray(r_len, np.uint32)


def pairs():
    os.environ.update(MHX_SEARCH_QBATCH="48", MHX_WITHIN_QBATCH="48", MHX_WITHIN_CELLS="420")
    import numpy as np
    import torch  # before the engine's library: the two then share one device runtime

    from auriclass_amd import engine

    engine.init(0)
    dev = torch.device("cuda")
    K, S, TOP, D, nq, nr = 21, 1000, 5, 0.05, 150, 200
    Q, ql, R, rl = (torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)).to(dev) for a in query_sets())
    stride = Q.shape[1]
    sets = (Q.data_ptr(), ql.data_ptr(), nq, R.data_ptr(), rl.data_ptr(), nr, stride)
    contain_sets = (Q.data_ptr(), ql.data_ptr(), nq, S, R.data_ptr(), rl.data_ptr(), nr, S, stride)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)   # noqa: E731
    host = lambda *ts: [t.cpu().numpy() for t in ts]                         # noqa: E731

    def search():
        ref, common, denom, n_hits = i32(nq, TOP), i32(nq, TOP), i32(nq, TOP), i32(nq)
        dist = torch.zeros((nq, TOP), dtype=torch.float64, device=dev)
        engine.dist_search_device(*sets, K, S, TOP, D, ref.data_ptr(), common.data_ptr(), denom.data_ptr(), dist.data_ptr(), n_hits.data_ptr())
        n = n_hits.cpu().numpy()
        live = np.arange(TOP)[None, :] < n[:, None]   # entries behind n_hits are unspecified
        return [n] + [np.where(live, a, 0) for a in host(ref, common, denom, dist)]

    def within(store):
        row_off = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        if not store:
            return [engine.dist_within_device(*sets, K, S, D, row_off.data_ptr(), 0, 0, 0, 0, 0)] + host(row_off)
        cap = nq * nr
        ref, common, denom = i32(cap), i32(cap), i32(cap)
        dist = torch.zeros(cap, dtype=torch.float64, device=dev)
        n = engine.dist_within_device(*sets, K, S, D, row_off.data_ptr(), ref.data_ptr(), common.data_ptr(), denom.data_ptr(), dist.data_ptr(), cap)
        return [n] + host(row_off, ref[:n], common[:n], denom[:n], dist[:n])

    def contain(winner):
        shared, n_qry, n_ref, won = i32(nq, nr), i32(nq, nr), i32(nq, nr), i32(nq, nr)
        if winner:
            engine.dist_contain_winner_device(*contain_sets, 0, won.data_ptr(), shared.data_ptr(), n_qry.data_ptr(), n_ref.data_ptr())
        else:
            engine.dist_contain_device(*contain_sets, shared.data_ptr(), n_qry.data_ptr(), n_ref.data_ptr())
        return host(won, shared, n_qry, n_ref)

    def contain_search():
        ref, shared, n_ref, n_qry, n_hits = i32(nq, TOP), i32(nq, TOP), i32(nq, TOP), i32(nq, TOP), i32(nq)
        engine.dist_contain_search_device(*contain_sets, K, TOP, 0.0, 1, ref.data_ptr(), shared.data_ptr(), n_ref.data_ptr(), n_qry.data_ptr(), n_hits.data_ptr())
        n = n_hits.cpu().numpy()
        live = np.arange(TOP)[None, :] < n[:, None]
        return [n] + [np.where(live, a, 0) for a in host(ref, shared, n_ref, n_qry)]

    calls = [("dist_search top 5", search), ("dist_within 0.05", lambda: within(True)), ("dist_within 0.05 counting", lambda: within(False)),
             ("dist_contain", lambda: contain(False)), ("dist_contain_winner", lambda: contain(True)), ("dist_contain_search top 5", contain_search)]
    lib = engine.load()
    for generic in (False, True):
        if generic:
            os.environ["MHX_DIST_GENERIC"] = "1"
        for what, call in calls:
            out = digest(call())
            print(f"{what}{' generic' if generic else ''}: {out} ranges {lib.mhx_last_dist_ranges()} fallbacks {lib.mhx_last_dist_fallback_blocks()}", flush=True)


def main():
    if sys.argv[1:2] == ["--names"]:
        print("\n".join(names(sys.argv[2])))
    elif sys.argv[1:2] == ["--pairs"]:
        pairs()
    else:
        all_pairs()


if __name__ == "__main__":
    main()
