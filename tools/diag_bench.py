"""ke_diagnose against the ke_eval route to the same FitError diagnosis.

The bench's 50k-node cluster (BASELINE config 3) with its queue placed, the profile carrying NodeResourcesFit's
Filter so that a pod can fit nowhere; then, for 64 and 512 pending pods that fit nowhere, the wall time of
  (a) ke_eval with only its status + reason outputs, plus the numpy reduction to the counts, the reason histogram
      and the plugin mask (the only way to a diagnosis before ke_diagnose);
  (b) ke_diagnose without bitmaps and with all three.
Each gets 3 warm-ups and >= 7 repeats in the same process and state, buffers allocated ahead.  A second pair of
ke_diagnose series runs on a second context in the same state, created under KOORDEVAL_DIAG_XCD=0 (the plain block
mapping instead of the XCD-aware default; the knob is read when a context is created).  Every diagnosis series is
checked against the reduction.  Prints min / median / max in ms as one JSON line.
Usage: python tools/diag_bench.py [--nodes 50000 --pods 100000 --diag-pods 64 512 --repeats 7 --warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from koordinator_amd import Evaluator, abi, reason_plugin, synth  # noqa: E402


def nowhere_pods(n, seed):
    """Pending pods no node of a filled cluster takes: half ask for more cpu, half for more memory than a node has."""
    pods = synth.add_fit_defaults(synth.make_pods(n, seed, key_base=9_000_000_000))
    pods["is_daemonset"] = 0
    big_cpu = np.arange(n) % 2 == 0
    for k in ("requests", "limits"):
        pods[k][big_cpu, abi.RES_CPU] = 4_000_000
        pods[k][~big_cpu, abi.RES_MEMORY] = 1 << 44
    return pods


def series(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"min": min(ms), "median": float(np.median(ms)), "max": max(ms), "all": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=synth.CONFIGS[3]["nodes"])
    ap.add_argument("--pods", type=int, default=synth.CONFIGS[3]["pods"])
    ap.add_argument("--diag-pods", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    N = a.nodes
    cl = synth.make_cluster(N, synth.BASE_SEED + 3)
    queue = synth.add_fit_defaults(synth.make_pods(a.pods, synth.BASE_SEED + 103))

    def context(knob):
        """A context with the queue placed; `knob`: KOORDEVAL_DIAG_XCD while it is created (None = unset)."""
        if knob is not None:
            os.environ["KOORDEVAL_DIAG_XCD"] = knob
        ev = Evaluator(synth.fit_config(synth.config(N)))
        os.environ.pop("KOORDEVAL_DIAG_XCD", None)
        synth.load_into(ev, cl)
        placed, sl = 0, max(1, a.pods // 20)
        for s in range(0, a.pods, sl):
            placed += int((ev.schedule(queue[s:s + sl], synth.T0)[0] >= 0).sum())
        return ev, placed

    (ev, placed), (ev_plain, placed_plain) = context(None), context("0")
    assert placed == placed_plain
    lib, now = ev.lib, int(synth.T0)
    plug = np.array([reason_plugin(r) for r in range(abi.DIAG_REASONS)], np.uint32)
    out = {"workload": f"{N} nodes, {a.pods} pods of the config-3 queue placed ({placed} on a node), NodeResourcesFit "
                       "Filter on; pending pods that fit nowhere", "unit": "ms wall per call", "repeats": a.repeats,
           "warmup": a.warmup, "pods": {}}
    ok = True
    for P in a.diag_pods:
        pods = nowhere_pods(P, synth.BASE_SEED + 1503)
        wpp = (N + 63) // 64
        status, reason = np.zeros((P, N), np.uint8), np.zeros((P, N), np.uint8)
        rec = np.zeros(P, abi.POD_DIAGNOSIS_DTYPE)
        words = [np.zeros((P, wpp), np.uint64) for _ in range(3)]
        red = {}

        def eval_route():
            ev._check(lib.ke_eval(ev.h, P, abi.ptr(pods), now, abi.ptr(status), abi.ptr(reason), None, None, None, None,
                                  None))
            for k, c in (("n_feasible", abi.CODE_SUCCESS), ("n_unschedulable", abi.CODE_UNSCHEDULABLE),
                         ("n_unresolvable", abi.CODE_UNSCHEDULABLE_AND_UNRESOLVABLE), ("n_error", abi.CODE_ERROR)):
                red[k] = np.count_nonzero(status == c, axis=1)
            idx = reason.astype(np.int32) + (np.arange(P, dtype=np.int32)[:, None] << 7)
            red["reason_nodes"] = np.bincount(idx.ravel(), minlength=P * abi.DIAG_REASONS).reshape(P, abi.DIAG_REASONS)
            hit = red["reason_nodes"] > 0
            hit[:, 0] = False
            red["plugins"] = np.bitwise_or.reduce(np.where(hit, plug[None, :], 0), axis=1)

        def diagnose(e, bitmaps):
            ptrs = [abi.ptr(w) for w in words] if bitmaps else [None] * 3
            e._check(lib.ke_diagnose(e.h, P, abi.ptr(pods), now, abi.ptr(rec), wpp, *ptrs))

        r = {"ke_eval_status_reason_plus_numpy": series(eval_route, a.warmup, a.repeats)}
        for e, tag in ((ev, ""), (ev_plain, "_plain_mapping")):
            for bitmaps, name in ((False, "ke_diagnose"), (True, "ke_diagnose_3_bitmaps")):
                rec[:] = 0
                r[name + tag] = series(lambda: diagnose(e, bitmaps), a.warmup, a.repeats)
                same = all(np.array_equal(rec[k], red[k]) for k in red)
                r[name + tag + "_equals_the_reduction"] = bool(same)
                ok = ok and same
        r["fit_nowhere"] = bool((rec["n_feasible"] == 0).all())
        r["reasons"] = {int(k): int(v) for k, v in enumerate(rec["reason_nodes"].sum(0)) if v}
        base = r["ke_eval_status_reason_plus_numpy"]["min"]
        r["condition_slowest_diagnose_faster_than_fastest_eval_route"] = bool(
            max(r["ke_diagnose"]["max"], r["ke_diagnose_3_bitmaps"]["max"]) < base)
        r["speedup_median"] = {k: r["ke_eval_status_reason_plus_numpy"]["median"] / r[k]["median"]
                               for k in r if k.startswith("ke_diagnose") and isinstance(r[k], dict)}
        out["pods"][str(P)] = r
    print(json.dumps(out))
    ev.close()
    ev_plain.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
