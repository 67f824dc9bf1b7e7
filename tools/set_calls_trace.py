"""The all-pairs calls of one small set, once each, as the program of a kernel trace: what a change of the host side of the
triangle must leave as it was is the ORDER of the kernels each call launches.  cluster_rate's planted set at n = 200,
s = 1000, k = 21, under MHX_TRI_QBATCH=48 (several blocks per reference slice, several slices):

    dist_triangle, dist_triangle_edges and dist_cluster at 0.05, dist_mst recomputed (MHX_MST_STORE=0), then stored (=1)

One line per call with a digest of what it returned, so that two libraries (MHX_LIB) can be compared by their output too.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/set_calls_trace.py
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


def main():
    if sys.argv[1:2] == ["--names"]:
        print("\n".join(names(sys.argv[2])))
        return
    os.environ["MHX_TRI_QBATCH"] = "48"
    from auriclass_amd import engine
    from cluster_rate import make_set

    engine.init(0)
    rows, lens, _ = make_set(200, 1000, seed=1200)
    calls = [("dist_triangle", None, lambda: engine.dist_triangle(rows, lens, 21, 1000)),
             ("dist_triangle_edges 0.05", None, lambda: engine.dist_triangle_edges(rows, lens, 21, 1000, 0.05)),
             ("dist_cluster 0.05", None, lambda: engine.dist_cluster(rows, lens, 21, 1000, 0.05)),
             ("dist_mst recomputed", "0", lambda: engine.dist_mst(rows, lens, 21, 1000)),
             ("dist_mst stored", "1", lambda: engine.dist_mst(rows, lens, 21, 1000))]
    for what, store, call in calls:
        if store is not None:
            os.environ["MHX_MST_STORE"] = store
        h = hashlib.sha256()
        for part in call():
            h.update(getattr(part, "tobytes", lambda: repr(part).encode())())
        print(f"{what}: {h.hexdigest()[:16]}", flush=True)


if __name__ == "__main__":
    main()
