"""Per-pod node score offsets: what a queue with score table ids costs on the config-3 workload.

The same cluster and queue (BASELINE config 3: 50k nodes x 100k pods) scheduled twice through the submit-ahead loop
of bench.py (ke_schedule_submit of step s+1 before ke_schedule_wait of step s), with 8 random tables of values
0..200 loaded both times: once with every pod's id 0 (the kernels of a call without ids run) and once with a random
id 0..8 per pod (the score-offset instantiations).  A bounded prefix of the run with offsets is checked against the
lock-step oracle (its eval's total plus the offset where feasible, the argmax, then the Reserve).  Prints one JSON
line with evals/s and the sampled per-batch kernel times of both runs.
Usage: python tools/nodescore_bench.py [--nodes 50000 --pods 100000 --steps 20 --warmup 5 --tables 8 --repeats 2]
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


def run(cfg, cl, tables, pods, ids, steps, warmup):
    def fresh():
        ev = Evaluator(cfg)
        synth.load_into(ev, cl)
        ev.node_scores_load(tables)
        return ev

    sl = len(pods) // steps
    if warmup > 0:  # a throwaway context, other pods
        ew = fresh()
        wp = synth.make_pods(warmup * sl, synth.BASE_SEED + 203)
        for w in range(warmup):
            ew.schedule(wp[w * sl:(w + 1) * sl], synth.T0, node_scores=ids[w * sl:(w + 1) * sl])
        ew.close()
    ev = fresh()
    ev.eval(pods[:0], synth.T0)  # every node row resident in HBM
    ev.set_profiling(8)  # (as bench.py: HIP-event samples of every 8th batch's kernels)
    part = lambda s: (pods[s * sl:(s + 1) * sl], synth.T0, ids[s * sl:(s + 1) * sl])  # noqa: E731
    placed, npipe, kss = 0, 0, []
    t0 = time.perf_counter()
    nxt = ev.submit(part(0)[0], part(0)[1], node_scores=part(0)[2])
    for s in range(steps):
        cur = nxt
        nxt = ev.submit(part(s + 1)[0], part(s + 1)[1], node_scores=part(s + 1)[2]) if s + 1 < steps else None
        chosen, _ = ev.wait(cur)
        placed += int((chosen >= 0).sum())
        kss.append(ev.kernel_stats())
        npipe += kss[-1]["pipelined_batches"]
    dt = time.perf_counter() - t0
    ev.close()
    n = steps * sl
    mean = lambda key: float(np.mean([k[key] for k in kss]))  # noqa: E731
    return {"value": n * cl.n_nodes / dt, "ms_per_pod": dt / n * 1e3, "placed": placed, "pipelined_batches": npipe,
            # per batch: the sampled eval and select kernels, the Reserve chain, its wait for the lists
            "kernel_ms_per_batch": {k: mean(k) for k in ("eval_ms", "select_ms", "resolve_ms", "handoff_ms")},
            "spec_failed_rounds_per_batch": mean("spec_failed_rounds")}


def oracle_prefix(cfg, cl, tables, pods, ids, n):
    from oracle.binding import Oracle  # checker only

    ev, o = Evaluator(cfg), Oracle(cfg, cl.n_nodes)
    synth.load_into(ev, cl)
    synth.load_into(o, cl)
    ev.node_scores_load(tables)
    c1, s1 = ev.schedule(pods[:n], synth.T0, node_scores=ids[:n])
    off = np.concatenate([np.zeros((1, cl.n_nodes), np.int64), tables.astype(np.int64)])
    for p in range(n):
        t = o.eval(pods[p:p + 1], synth.T0, n_threads=16)["total"][0].astype(np.int64)
        t = np.where(t >= 0, t + off[ids[p]], -1)
        node = int(np.argmax(t))
        want = (node, int(t[node])) if t[node] >= 0 else (-1, -1)
        if (int(c1[p]), int(s1[p])) != want:
            return False
        if t[node] >= 0:
            o.assign_bulk([node], pods[p:p + 1], [synth.T0])
            req = o.node_info_requested(node)[0]
            o.set_requested(node, int(req[0]) + int(pods["requests"][p, abi.RES_CPU]),
                            int(req[1]) + int(pods["requests"][p, abi.RES_MEMORY]))
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=synth.CONFIGS[3]["nodes"])
    ap.add_argument("--pods", type=int, default=synth.CONFIGS[3]["pods"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tables", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=1, help="runs of each kind, alternating (the best of each is reported)")
    ap.add_argument("--check-pods", type=int, default=128, help="lock-step oracle prefix of the run with offsets (0 = off)")
    a = ap.parse_args()
    cl = synth.make_cluster(a.nodes, synth.BASE_SEED + 3)
    pods = synth.make_pods(a.pods, synth.BASE_SEED + 103)
    rng = np.random.default_rng(synth.BASE_SEED + 1503)
    tables = rng.integers(0, 201, (a.tables, a.nodes)).astype(np.uint16)
    ids = rng.integers(0, a.tables + 1, a.pods).astype(np.int32)
    cfg = synth.config(a.nodes)
    runs = [(run(cfg, cl, tables, pods, np.zeros(a.pods, np.int32), a.steps, a.warmup),
             run(cfg, cl, tables, pods, ids, a.steps, a.warmup)) for _ in range(max(1, a.repeats))]
    base = max((r[0] for r in runs), key=lambda r: r["value"])
    with_scores = max((r[1] for r in runs), key=lambda r: r["value"])
    out = {"workload": f"{a.nodes} nodes x {a.pods} pods (config-3 shape), {a.tables} random score tables of values 0..200",
           "unit": "pod-node evals/s", "ids_all_zero": base, "ids_random": with_scores,
           "offset_cost": base["value"] / with_scores["value"],
           "all_values": {"ids_all_zero": [r[0]["value"] for r in runs], "ids_random": [r[1]["value"] for r in runs]},
           "all_kernel_ms_per_batch": {"ids_all_zero": [r[0]["kernel_ms_per_batch"] for r in runs],
                                       "ids_random": [r[1]["kernel_ms_per_batch"] for r in runs]}}
    if a.check_pods:
        out["oracle_prefix_equal"] = oracle_prefix(cfg, cl, tables, pods, ids, a.check_pods)
        out["oracle_prefix_pods"] = a.check_pods
    print(json.dumps(out))


if __name__ == "__main__":
    main()
