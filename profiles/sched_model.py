"""List-scheduling model of a kernel whose workgroups each own one or more work items of known cost (pure Python / NumPy, no GPU).

The dispatcher hands workgroup i to XCD i % 8; inside an XCD a freed slot takes that XCD's next workgroup.  The model runs exactly that:
`slots` resident workgroups in all, slots / 8 per XCD, every workgroup busy for the sum of its items' costs.  It knows nothing of memory
or of two wavefronts sharing a SIMD's issue slots -- a wavefront alone on its SIMD in the tail of a launch runs faster than the model says --
so the idle share it reports is an UPPER bound on what a better order can win.

    python profiles/sched_model.py counts.npy [--slots 2048] [--fixed 0]

prints, for the tracer backward's per-batch entry counts (one int per batch, or the (batches, 2) n_entries array), the makespan over the
ideal (total cost / slots) of the dispatch until round 6 (coherence order, grid-stride over 8192 workgroups) and of the longest-first
order with K = 1, 8, 32 classes and a full sort.
"""
import argparse
import heapq
import os
import sys

if __name__ == "__main__":       # run as a script this directory leads sys.path, and its numbers.py would shadow the stdlib's under NumPy
    sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != os.path.dirname(os.path.abspath(__file__))]

import numpy as np  # noqa: E402


def makespan(workgroup_costs, slots=2048, xcds=8):
    """workgroup_costs: cost of each workgroup in dispatch order.  Returns the time at which the last one finishes."""
    per = max(1, slots // xcds)
    end = 0.0
    for x in range(xcds):
        mine = workgroup_costs[x::xcds]
        free = [0.0] * per
        heapq.heapify(free)
        for c in mine:
            t = heapq.heappop(free) + float(c)
            heapq.heappush(free, t)
            end = max(end, t)
    return end


def ideal(costs, slots=2048):
    costs = np.asarray(costs, dtype=np.float64)
    return max(costs.sum() / slots, costs.max() if costs.size else 0.0)


def strided_workgroups(costs, grid=8192):
    """Round 6's dispatch: workgroup w runs items w, w + grid, ... back to back."""
    costs = np.asarray(costs, dtype=np.float64)
    g = min(grid, len(costs))
    out = np.zeros(g)
    for s in range(0, len(costs), g):
        part = costs[s:s + g]
        out[:len(part)] += part
    return out


def class_order(counts, classes):
    """The order envgs_trace_forward builds (include/envgs_trace.h: bwd_order): stable, descending class = count * K // (max + 1); classes = 0: full sort."""
    counts = np.asarray(counts, dtype=np.int64)
    key = counts if classes <= 0 else (counts * classes) // (int(counts.max()) + 1)
    return np.argsort(-key, kind="stable")


def report(counts, slots=2048, fixed=0.0):
    counts = np.asarray(counts, dtype=np.int64)
    if counts.ndim == 2:
        counts = counts.sum(1)
    cost = counts.astype(np.float64) + fixed
    lo = ideal(cost, slots)
    rows = [("coherence order, 8192 workgroups (round 6)", makespan(strided_workgroups(cost), slots) / lo)]
    for k in (1, 8, 32, 0):
        rows.append(("one workgroup per batch, %s" % ("full sort" if k == 0 else "K = %d" % k), makespan(cost[class_order(counts, k)], slots) / lo))
    return dict(batches=int(counts.size), mean=float(counts.mean()), cv=float(counts.std() / max(counts.mean(), 1e-9)), max=int(counts.max()),
                min=int(counts.min()), rounds=float(counts.size / slots), rows=rows)


def format_report(r):
    s = "batches %d  entries per batch: mean %.1f  cv %.3f  min %d  max %d  (%.2f rounds of the resident slots)\n" % (
        r["batches"], r["mean"], r["cv"], r["min"], r["max"], r["rounds"])
    for name, v in r["rows"]:
        s += "    %-46s makespan / ideal %.3f\n" % (name, v)
    return s


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("counts")
    ap.add_argument("--slots", type=int, default=2048, help="resident workgroups: 256 CUs x 4 SIMDs x 2 wavefronts")
    ap.add_argument("--fixed", type=float, default=0.0, help="cost of a batch beyond its entries, in entries")
    a = ap.parse_args()
    print(format_report(report(np.load(a.counts), a.slots, a.fixed)), end="")
