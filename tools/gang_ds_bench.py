"""Gang runs with DeviceShare members ("DeviceShare members"): one ke_schedule call with ke_pod_gangs and
ke_set_gang_devices against the caller's only path without them.

Workload: a config-5-like cluster -- 8 GPUs and 2 RDMA NICs on every node, most GPUs taken, NodeResourcesFit's Filter on
-- and a queue of which a fixed share sits in strict runs of 8 workers asking for one whole GPU each (min_member = 8); a
fifth of the other pods ask for devices too.  A worker of two runs in five fits nowhere (its CPU request), and the free
GPUs run short along the queue, so a sizeable share of the runs fails with members placed and is rolled back.  Three
ways, each on fresh contexts, `--warmup` throwaway repeats and `--repeats` timed:
  single    one ke_schedule with the runs and the switch on
  per_run   one ke_schedule per run and per plain stretch, ke_unreserve per placed member of a failed run (the yardstick)
  stripped  the same queue without runs (the cost of the gang batches; placements differ)
The condition (§4w's form): single's slowest repeat is faster than per_run's fastest, and both place identically, minors
included.  Writes one JSON file (default profiles/gangs/gang_ds_bench.json) and prints it.
Usage: python tools/gang_ds_bench.py [--nodes 2000 --pods 1200 --share 0.33 --out FILE]
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


def workload(nodes, n_pods, share, taken, fail, seed):
    rng = np.random.default_rng(seed)
    cl = synth.make_cluster(nodes, seed + 1)
    cl.nodes["requested"][:, 0] = np.maximum(cl.nodes["allocatable"][:, 0] - 32000, 0)
    cl.nodes["requested"][:, 1] = np.maximum(cl.nodes["allocatable"][:, 1] - 64 * synth.GI, 0)
    tables = synth.make_node_resources(cl, seed + 2)
    devs = synth.make_devices(nodes, seed + 3, no_cache_fraction=0.0, unhealthy_fraction=0.0)
    for d in devs:  # most of the GPUs the generator left free are taken whole
        for m in np.nonzero((d["type"] == abi.DEV_GPU) & (d["has_used"][:, 0] == 0))[0]:
            if rng.random() < taken:
                d[m]["has_used"][:] = 1
                d[m]["used"][:] = d[m]["total"]
    pods = synth.make_pods(n_pods, seed + 4)
    for f in ("requests", "limits"):
        pods[f][:] = 0
    pods["requests"][:, abi.RES_CPU] = pods["limits"][:, abi.RES_CPU] = rng.choice([1, 2, 4], n_pods) * 1000
    pods["requests"][:, abi.RES_MEMORY] = pods["limits"][:, abi.RES_MEMORY] = rng.choice([2, 4, 8], n_pods) * synth.GI
    pods["priority_class"], pods["qos_class"], pods["is_daemonset"] = abi.PRIORITY_PROD, abi.QOS_LS, 0
    pods["gpu_ring_bus_bandwidth"] = abi.ABSENT
    gpu, shared, core, ratio = (abi.PDR[k] for k in ("nvidia.com/gpu", "koordinator.sh/gpu.shared", "koordinator.sh/gpu-core",
                                                     "koordinator.sh/gpu-memory-ratio"))
    runs, p, in_runs = [], 0, 0
    member = np.zeros(n_pods, bool)
    while p < n_pods:
        gap = int(rng.geometric(share / (1 - share) / 8.0)) if share < 1 else 0
        p += gap
        if p + 8 > n_pods:
            break
        runs.append((p, 8, 8, 0, abi.GANG_STRICT))
        member[p:p + 8] = True
        p, in_runs = p + 8, in_runs + 8
    pods["device_requests"][member, gpu] = 1
    for r in runs:  # a worker of two runs in five asks for more CPU than any node has: the run fails at that member
        if rng.random() < fail:
            q = r[0] + int(rng.integers(2, 8))
            pods["requests"][q, abi.RES_CPU] = pods["limits"][q, abi.RES_CPU] = 10_000_000
    for q in np.nonzero(~member & (rng.random(n_pods) < 0.2))[0]:
        pods["device_requests"][q, shared], pods["device_requests"][q, core], pods["device_requests"][q, ratio] = 1, 25, 25
    pods["has_other_requests"][pods["device_requests"].any(axis=1)] = 1
    return cl, tables, devs, pods, runs, in_runs / n_pods


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=2000)
    ap.add_argument("--pods", type=int, default=1200)
    ap.add_argument("--share", type=float, default=0.33)
    ap.add_argument("--taken", type=float, default=0.9, help="share of the free GPUs taken whole before the queue")
    ap.add_argument("--fail", type=float, default=0.4, help="share of the runs with a worker that fits nowhere")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gangs", "gang_ds_bench.json"))
    a = ap.parse_args()
    cl, tables, devs, pods, runs, share = workload(a.nodes, a.pods, a.share, a.taken, a.fail, synth.BASE_SEED + 89_000)
    cfg = synth.fit_config(synth.config(a.nodes), filter=True)
    T0 = synth.T0

    def fresh(on):
        ev = Evaluator(cfg)
        synth.load_into(ev, cl)
        synth.load_node_resources(ev, tables)
        synth.load_devices(ev, devs)
        ev.set_gang_devices(on)
        ev.eval(pods[:0], T0)  # every node row resident
        return ev

    def single(ev):
        c = ev.schedule(pods, T0, gangs=runs)[0]
        return c, np.asarray(ev.last_device_allocations, np.uint64).copy()

    def stripped(ev):
        c = ev.schedule(pods, T0)[0]
        return c, np.asarray(ev.last_device_allocations, np.uint64).copy()

    def per_run(ev):
        chosen, minors = np.full(len(pods), -1, np.int32), np.zeros(len(pods), np.uint64)
        edges = sorted({0, len(pods)} | {r[0] for r in runs} | {r[0] + r[1] for r in runs})
        first = {r[0] for r in runs}
        for lo, hi in zip(edges[:-1], edges[1:]):
            c, _ = ev.schedule(pods[lo:hi], T0)
            m = np.asarray(ev.last_device_allocations, np.uint64).copy()
            if lo in first and (c < 0).any():  # strict, min_member = the length: any failure rejects the gang
                for q in np.nonzero(c >= 0)[0]:
                    ev.unreserve(pods[lo + q], int(q))
                c[:], m[:] = -1, 0
            chosen[lo:hi], minors[lo:hi] = c, m
        return chosen, minors

    out = {"nodes": a.nodes, "pods": a.pods, "runs": len(runs), "share_in_runs": share, "taken": a.taken, "fail": a.fail,
           "warmup": a.warmup, "repeats": a.repeats}
    results = {}
    for name, fn, on in (("single", single, True), ("per_run", per_run, False), ("stripped", stripped, False)):
        ms = []
        for r in range(a.warmup + a.repeats):
            ev = fresh(on)
            t0 = time.perf_counter()
            results[name] = fn(ev)
            dt = (time.perf_counter() - t0) * 1e3
            if name == "single" and r == 0:
                d = ev.debug_gangs()
                out["failed_run_rate"] = d["rolled_back"] / max(d["runs"], 1)
                out["debug_gangs"] = d
                out["debug_gang_devices"] = ev.debug_gang_devices()
                out["ds_cuts"] = ev.ds_cuts()
                out["pipelined_batches"] = ev.kernel_stats()["pipelined_batches"]
            ev.close()
            if r >= a.warmup:
                ms.append(dt)
        out[name + "_ms"] = ms
    if out["failed_run_rate"] < 0.05:
        print(json.dumps(out))
        sys.exit("gang_ds_bench: fewer than 5 % of the runs failed (%.3f): the workload is not saturated, no condition reported"
                 % out["failed_run_rate"])
    out["identical"] = bool(np.array_equal(results["single"][0], results["per_run"][0]) and
                            np.array_equal(results["single"][1], results["per_run"][1]))
    out["placed"] = int((results["single"][0] >= 0).sum())
    out["condition_met"] = bool(out["identical"] and max(out["single_ms"]) < min(out["per_run_ms"]))
    out["gang_batches_cost_ms"] = float(np.median(out["single_ms"]) - np.median(out["stripped_ms"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0 if out["condition_met"] else 1


if __name__ == "__main__":
    sys.exit(main())
