"""Gang runs: one ke_schedule call with ke_pod_gangs against the caller's only path without them.

Workload: a synthetic cluster saturated until a share of the gangs fail (NodeInfo.Requested a little below Allocatable,
NodeResourcesFit's Filter on) and a queue of plain pods of which a fixed share sit in runs of 8 and 32 (strict,
min_member = the run's length).  Three ways, each on fresh contexts, `--warmup` throwaway repeats and `--repeats` timed:
  single    one ke_schedule with the runs
  per_run   one ke_schedule per run and per plain stretch, ke_unreserve per placed member of a failed run (the yardstick)
  stripped  the same queue without runs, fully pipelined (the cost of serial gang batches; placements differ)
The condition (§4q's form): single's slowest repeat is faster than per_run's fastest, and both place identically.
Writes one JSON file (default profiles/gangs/gang_bench.json) and prints it.
Usage: python tools/gang_bench.py [--nodes 20000 --pods 5000 --share 0.3 --out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from koordinator_amd import Evaluator, abi, synth  # noqa: E402


def workload(nodes, n_pods, share, seed):
    rng = np.random.default_rng(seed)
    cl = synth.make_cluster(nodes, seed + 1)
    # three nodes in four are full; the rest leave about 0.85 of the queue's 4.67-core mean request x n_pods in all, in
    # pieces of 2, 4 and 8 cores, so the queue's tail -- and a long run sooner than a plain pod -- finds no room
    room = 0.85 * 4670 * n_pods / nodes
    slack = rng.choice([0, 2000, 4000, 8000], nodes, p=[0.75, 0.10, 0.10, 0.05]) * max(room / 1000.0, 0.0)
    slack = (np.round(slack / 2000.0) * 2000).astype(np.int64)
    cl.nodes["requested"][:, 0] = np.maximum(cl.nodes["allocatable"][:, 0] - slack, 0)
    cl.nodes["requested"][:, 1] = np.maximum(cl.nodes["allocatable"][:, 1] - 64 * synth.GI, 0)
    tables = synth.make_node_resources(cl, seed + 2)
    pods = synth.make_pods(n_pods, seed + 3)
    for f in ("requests", "limits"):
        pods[f][:] = 0
    pods["requests"][:, abi.RES_CPU] = pods["limits"][:, abi.RES_CPU] = rng.choice([2, 4, 8], n_pods) * 1000
    pods["requests"][:, abi.RES_MEMORY] = pods["limits"][:, abi.RES_MEMORY] = rng.choice([2, 4, 8], n_pods) * synth.GI
    pods["priority_class"], pods["qos_class"], pods["is_daemonset"] = abi.PRIORITY_PROD, abi.QOS_LS, 0
    runs, p, in_runs = [], 0, 0
    while p < n_pods:
        c = int(rng.choice([8, 32]))
        gap = int(rng.geometric(share / (1 - share) / 20.0)) if share < 1 else 0
        p += gap
        if p + c > n_pods:
            break
        runs.append((p, c, c, 0, abi.GANG_STRICT))
        p, in_runs = p + c, in_runs + c
    return cl, tables, pods, runs, in_runs / n_pods


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=20000)
    ap.add_argument("--pods", type=int, default=5000)
    ap.add_argument("--share", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gangs", "gang_bench.json"))
    a = ap.parse_args()
    cl, tables, pods, runs, share = workload(a.nodes, a.pods, a.share, synth.BASE_SEED + 88_000)
    cfg = synth.fit_config(synth.config(a.nodes), filter=True)
    T0 = synth.T0

    def fresh():
        ev = Evaluator(cfg)
        synth.load_into(ev, cl)
        synth.load_node_resources(ev, tables)
        ev.eval(pods[:0], T0)  # every node row resident
        return ev

    def single(ev):
        return ev.schedule(pods, T0, gangs=runs)[0]

    def stripped(ev):
        return ev.schedule(pods, T0)[0]

    def per_run(ev):
        chosen = np.full(len(pods), -1, np.int32)
        edges = sorted({0, len(pods)} | {r[0] for r in runs} | {r[0] + r[1] for r in runs})
        first = {r[0] for r in runs}
        for lo, hi in zip(edges[:-1], edges[1:]):
            c, _ = ev.schedule(pods[lo:hi], T0)
            if lo in first and (c < 0).any():  # strict, min_member = the length: any failure rejects the gang
                for q in np.nonzero(c >= 0)[0]:
                    ev.unreserve(pods[lo + q], int(q))
                c[:] = -1
            chosen[lo:hi] = c
        return chosen

    out = {"nodes": a.nodes, "pods": a.pods, "runs": len(runs), "share_in_runs": share, "warmup": a.warmup, "repeats": a.repeats}
    results = {}
    for name, fn in (("single", single), ("per_run", per_run), ("stripped", stripped)):
        ms = []
        for r in range(a.warmup + a.repeats):
            ev = fresh()
            t0 = time.perf_counter()
            results[name] = fn(ev)
            dt = (time.perf_counter() - t0) * 1e3
            if name == "single" and r == 0:
                d = ev.debug_gangs()
                out["failed_run_rate"] = d["rolled_back"] / max(d["runs"], 1)
                out["debug_gangs"] = d
                out["pipelined_batches"] = ev.kernel_stats()["pipelined_batches"]
            ev.close()
            if r >= a.warmup:
                ms.append(dt)
        out[name + "_ms"] = ms
    # (a skipped member is never tried in the single call; per_run tries and unreserves it: same end state)
    if out["failed_run_rate"] < 0.05:
        print(json.dumps(out))
        sys.exit("gang_bench: fewer than 5 % of the runs failed (%.3f): the workload is not saturated, no condition reported"
                 % out["failed_run_rate"])
    out["identical"] = bool(np.array_equal(results["single"], results["per_run"]))
    out["placed"] = int((results["single"] >= 0).sum())
    out["condition_met"] = bool(out["identical"] and max(out["single_ms"]) < min(out["per_run_ms"]))
    out["serial_gang_batches_cost_ms"] = float(np.median(out["single_ms"]) - np.median(out["stripped_ms"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0 if out["condition_met"] else 1


if __name__ == "__main__":
    sys.exit(main())
