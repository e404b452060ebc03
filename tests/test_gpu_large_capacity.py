"""Contexts whose node capacity exceeds the replay's LDS changed-node bitmap (811,008 node ids): the changed-node set
lives in device memory (ChgSet.glb -- chg_set / chg_or with the store drain, chg_load_word, the withdrawn
predictions' fetch_and, chg_clear_word, the memset after an abandoned replay), and above 2^20 the pipelined run has one
eval stream.  The capacity comes from the config while the kernels run over the populated index range, so these are
small workloads: every case is bit-exact with the oracle in placements and scores and leaves exact records and rows
(the bitmap is zero again between batches and calls, or the next batch's replay would skip or re-fetch rows).
Nothing in the ABI tells which bitmap a context allocated: landscapes.CHG_LDS_NODES restates CHG_LDS_WORDS * 32 of
ke_kernels.hip and must be kept in step with it, or these cases run the LDS path unnoticed."""
import numpy as np
import pytest

import landscapes as L
from koordinator_amd import Evaluator, abi, synth
from oracle.binding import Oracle
from test_gpu_select_landscapes import MODES, assert_placed, assert_state_exact, run_hot

pytestmark = pytest.mark.gpu
T0 = synth.T0
CAP = 811_009  # rounds to 811,264 > 811,008: the global bitmap


def _plain(n):
    def make():
        cl = synth.make_cluster(n, synth.BASE_SEED + 9421 + n)
        pods = synth.make_pods(1500, synth.BASE_SEED + 9422 + n)
        o = Oracle(synth.config(n), n)
        synth.load_into(o, cl)
        return dict(n=n, cl=cl, pods=pods, want=o.schedule(pods, T0))
    return L.cached(("plain", n), make)


def _ctx(c, capacity=CAP, batch=64):
    ev = Evaluator(synth.config(capacity, pod_batch=batch))
    synth.load_into(ev, c["cl"])
    assert ev.num_nodes == c["n"]
    return ev


@pytest.mark.parametrize("mode,batch", [("stale-slots", 64), ("fixup", 64), ("serial", 64), ("stale-slots", 7)])
@pytest.mark.parametrize("n", [3000, 150])
def test_plain_queue(gpu, n, mode, batch):
    c = _plain(n)
    ev = _ctx(c, batch=batch)
    ev.set_pipeline(MODES[mode])
    got = ev.schedule(c["pods"], T0)
    assert (ev.kernel_stats()["pipelined_batches"] > 0) == (mode != "serial")
    assert_placed(got, c["want"])
    assert (got[0] >= 0).sum() > 1000
    assert_state_exact(ev)
    ev.close()


@pytest.mark.parametrize("mode", ["stale-slots", "serial"])
def test_hot_nodes_withdraw_predictions(gpu, mode):
    """Failed speculative rounds on the global bitmap: dropped predictions are withdrawn from it by fetch_and."""
    run_hot(synth.config(CAP), mode)


@pytest.mark.parametrize("mode", ["stale-slots", "serial"])
def test_all_tie_shares_bitmap_words(gpu, mode):
    """Identical nodes: pod j of a batch predicts node j, so consecutive predictions set bits of one bitmap word that
    the next pods' loads read straight after (the ordering chg_or<true>'s store drain is there for)."""
    n = L.CONFIGS["one-part"][0]
    c = L.landscape_reference("all-tie", n, 1)
    assert np.array_equal(c["want"][0], np.arange(L.N_PODS))
    ev = _ctx(c)
    ev.set_pipeline(MODES[mode])
    got = ev.schedule(c["pods"], T0)
    assert_placed(got, c["want"])
    assert_state_exact(ev)
    ev.close()


def test_consecutive_calls_and_submit_ahead(gpu):
    """Two calls on one context, then on a fresh one four submitted slices with one kept in flight: both equal the
    oracle's single schedule of the queue (which the single call equals, test_plain_queue)."""
    c = _plain(3000)
    pods, want = c["pods"][:1200], (c["want"][0][:1200], c["want"][1][:1200])
    ev = _ctx(c)
    a, b = ev.schedule(pods[:600], T0), ev.schedule(pods[600:], T0)
    assert_placed((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])), want)
    assert_state_exact(ev)
    ev.close()
    ev = _ctx(c)
    out, prev = [], None
    for s in range(0, 1200, 300):
        t = ev.submit(pods[s:s + 300], T0)
        if prev is not None:
            out.append(ev.wait(prev))
        prev = t
    out.append(ev.wait(prev))
    assert_placed((np.concatenate([x[0] for x in out]), np.concatenate([x[1] for x in out])), want)
    assert_state_exact(ev)
    ev.close()


# ---- one queue each through the other replay instantiations that take the global bitmap ------------------------------
def _both(cfg_ev, n, cl, load):
    ev, o = Evaluator(cfg_ev), Oracle(cfg_ev, n)
    for h in (ev, o):
        synth.load_into(h, cl)
        load(h)
    return ev, o


def test_deviceshare_queue(gpu):
    n = 900
    cl = synth.make_cluster(n, synth.BASE_SEED + 93)
    dv = synth.make_devices(n, synth.BASE_SEED + 143)
    pods = synth.make_ds_pods(400, synth.BASE_SEED + 94, device_fraction=0.7)
    ev, o = _both(synth.config(CAP), n, cl, lambda h: synth.load_devices(h, dv))
    assert_placed(ev.schedule(pods, T0), o.schedule(pods, T0))
    assert np.array_equal(ev.last_device_allocations, o.last_device_allocations)
    assert (ev.last_device_allocations != 0).sum() > 50
    assert_state_exact(ev)
    ev.close()


def test_numa_policy_queue(gpu):
    n = 300
    cl = synth.make_cluster(n, synth.BASE_SEED + 100, amplified_fraction=0.3)
    zs = synth.make_numa(cl, synth.BASE_SEED + 150, zone_counts=(1, 2, 4), status_fraction=0.4)
    pods = synth.make_numa_pods(256, synth.BASE_SEED + 101, policy_fraction=0.5)
    ev, o = _both(synth.config(CAP), n, cl, lambda h: synth.load_numa(h, zs))
    assert_placed(ev.schedule(pods, T0), o.schedule(pods, T0))
    assert np.array_equal(ev.last_numa_allocations, o.last_numa_allocations)
    assert np.any(ev.last_numa_allocations != 0)
    assert_state_exact(ev)
    ev.close()


def test_cpuset_queue(gpu):
    n = 300
    cl = synth.make_cluster(n, synth.BASE_SEED + 211, amplified_fraction=0.3)
    tabs = synth.make_cpus(cl, synth.BASE_SEED + 212)
    pods = synth.make_cpuset_pods(160, synth.BASE_SEED + 213)
    ev, o = _both(synth.config(CAP), n, cl, lambda h: synth.load_cpus(h, tabs))
    got = ev.schedule(pods, T0)
    assert_placed(got, o.schedule(pods, T0))
    assert np.array_equal(ev.last_cpusets, o.last_cpusets) and np.any(ev.last_cpusets != 0)
    assert (got[0] >= 0).sum() > 100
    assert_state_exact(ev)
    ev.close()


def test_quota_queue(gpu):
    n = 600
    cl = synth.make_cluster(n, synth.BASE_SEED + 95)
    pods = synth.make_pods(900, synth.BASE_SEED + 195)
    tc = int(pods["requests"][:, abi.RES_CPU].sum() * 0.4)
    tm = int(pods["requests"][:, abi.RES_MEMORY].sum() * 0.4)
    q = synth.make_quota_tree(305, 64, 8, tc, tm)
    pods = synth.assign_quotas(pods, q, 306)
    ev, o = _both(synth.config(CAP), n, cl, lambda h: h.quotas_load(synth.quota_args(tc, tm), q))
    got = ev.schedule(pods, T0)
    assert ev.kernel_stats()["pipelined_batches"] > 0
    assert_placed(got, o.schedule(pods, T0))
    for i in range(len(q)):
        a, b = ev.quota_state(i), o.quota_state(i)
        for k in ("limit", "used", "np_used"):
            assert np.array_equal(a[k], b[k]), (i, k)
    refused = int(((got[0] < 0) & (pods["quota"] > 0)).sum())
    assert 0 < refused < len(pods)
    assert_state_exact(ev)
    ev.close()


# ---- node ids above the LDS bitmap's range -----------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [64, 16])
def test_sparse_high_ids(gpu, batch):
    """Nodes at [0, 300) and [811,008, 811,308): bitmap words above the LDS range are set and cleared, and the select
    streams over four parts (five to eight with 16-pod batches) of about 200k nodes that hold almost no node."""
    def make():
        cl = synth.make_cluster(600, synth.BASE_SEED + 5)
        pods = synth.make_pods(200, synth.BASE_SEED + 6)
        ids = L.sparse_ids()
        return dict(cl=cl, pods=pods, ids=ids, want=L.compact_reference(synth.config(600), cl, ids, pods))
    c = L.cached("sparse", make)
    n = int(c["ids"][-1]) + 1
    parts = L.select_parts(n, batch)
    assert parts >= 4 and L.select_boundaries(n, parts)["streamed"]
    assert int((c["want"][0] >= L.CHG_LDS_NODES).sum()) >= 20
    ev = Evaluator(synth.config(811_520, pod_batch=batch))
    L.load_sparse(ev, c["cl"], c["ids"])
    assert ev.num_nodes == n
    got = ev.schedule(c["pods"], T0)
    assert ev.kernel_stats()["pipelined_batches"] > 0
    assert_placed(got, c["want"])
    assert int((got[0] >= L.CHG_LDS_NODES).sum()) >= 20
    assert_state_exact(ev)
    ev.close()


def test_capacity_above_2_pow_20_single_eval_stream(gpu):
    """Above 2^20 nodes of capacity the second score buffer and eval stream are not allocated: the pipelined run's
    evals wait for the done flag themselves."""
    c = _plain(3000)
    ev = _ctx(c, capacity=(1 << 20) + 1)
    got = ev.schedule(c["pods"], T0)
    assert ev.kernel_stats()["pipelined_batches"] > 0
    assert_placed(got, c["want"])
    assert_state_exact(ev)
    ev.close()
