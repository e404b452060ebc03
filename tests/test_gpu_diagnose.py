"""ke_diagnose on the device: the per-pod reductions (class counts, reason histogram, plugin mask, the three class
bitmaps) equal, exactly, the numpy reduction of the oracle's eval status / reason -- and of Evaluator.eval's -- for
every pod kind ke_eval takes, with node sets, deleted node slots, the NUMA deferral, after a saturated queue and
without side effects.  Each case first asserts on the reference alone that it is worth running (>= 3 reasons with
non-zero counts, feasible and infeasible pairs)."""
import ctypes as C

import numpy as np
import pytest

from koordinator_amd import Evaluator, abi, reason_plugin, synth
from koordinator_amd.evaluator import as_pod_array, unpack_node_sets
from oracle.binding import Oracle
from test_gpu_cpuset import NUMA_VARIANTS, numa_cpuset_both

pytestmark = pytest.mark.gpu
T0 = synth.T0
S = synth.BASE_SEED + 9400
COUNTS = ("n_nodes", "n_absent", "n_feasible", "n_unschedulable", "n_unresolvable", "n_error")
BITMAPS = ("feasible", "unschedulable", "unresolvable")
CODE_OF = {"feasible": abi.CODE_SUCCESS, "unschedulable": abi.CODE_UNSCHEDULABLE,
           "unresolvable": abi.CODE_UNSCHEDULABLE_AND_UNRESOLVABLE}


def plugin_of(r):
    """include/koord_eval.h's ranges, restated."""
    for lo, hi, bit in ((1, 15, abi.PLUGIN_LOADAWARE), (16, 31, abi.PLUGIN_NODENUMARESOURCE),
                        (32, 49, abi.PLUGIN_DEVICESHARE), (50, 63, abi.PLUGIN_RESERVATION),
                        (64, 95, abi.PLUGIN_NODERESOURCESFIT), (96, 96, abi.PLUGIN_NODE_SET)):
        if lo <= r <= hi:
            return bit
    return 0


def reduce_eval(status, reason, present=None, elig=None):
    """The reference: ke_diagnose's outputs from a [P, N] status / reason pair.  `present`: bool [N], the populated
    node slots (default all); `elig`: bool [P, N], the pods' node sets (a pair outside is KE_REASON_NODE_SET,
    unresolvable, as test_gpu_node_sets.py masks the oracle)."""
    status, reason = np.array(status, np.int64), np.array(reason, np.int64)
    P, N = status.shape
    present = np.ones(N, bool) if present is None else np.asarray(present, bool)
    if elig is not None:
        status[~elig] = abi.CODE_UNSCHEDULABLE_AND_UNRESOLVABLE
        reason[~elig] = abi.REASON_NODE_SET
    out = {"n_nodes": np.full(P, present.sum(), np.int32), "n_absent": np.full(P, N - present.sum(), np.int32)}
    for k, code in (("n_feasible", abi.CODE_SUCCESS), ("n_unschedulable", abi.CODE_UNSCHEDULABLE),
                    ("n_unresolvable", abi.CODE_UNSCHEDULABLE_AND_UNRESOLVABLE), ("n_error", abi.CODE_ERROR)):
        out[k] = ((status == code) & present).sum(1).astype(np.int32)
    out["reason_nodes"] = np.stack([np.bincount(reason[p][present], minlength=abi.DIAG_REASONS)
                                    for p in range(P)]).astype(np.int32).reshape(P, abi.DIAG_REASONS)
    out["plugins"] = np.array([np.bitwise_or.reduce([plugin_of(r) for r in np.nonzero(row[1:])[0] + 1] or [0])
                               for row in out["reason_nodes"]], np.uint32)
    for k in BITMAPS:
        out[k] = (status == CODE_OF[k]) & present
    return out


def worth_running(want, reasons=3):
    assert (want["reason_nodes"][:, 1:].sum(0) > 0).sum() >= reasons, np.nonzero(want["reason_nodes"].sum(0))[0]
    assert want["n_feasible"].sum() > 0 and (want["n_unschedulable"] + want["n_unresolvable"]).sum() > 0


def assert_same(got, want, what=""):
    for k in COUNTS + ("reason_nodes", "plugins") + BITMAPS:
        if k in got:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            bad = np.argwhere(got[k] != want[k])
            assert len(bad) == 0, f"{what} {k}: {len(bad)} mismatches, first {bad[:5].tolist()}"
    # the struct's invariants
    assert np.array_equal(got["n_feasible"] + got["n_unschedulable"] + got["n_unresolvable"] + got["n_error"],
                          got["n_nodes"])
    assert np.array_equal(got["reason_nodes"][:, 1:].sum(1), got["n_unschedulable"] + got["n_unresolvable"])
    assert np.array_equal(got["reason_nodes"][:, 0], got["n_feasible"] + got["n_error"])


def check(ev, o, pods, now=T0, ids=None, sets=None, present=None, what=""):
    """diagnose (with bitmaps) == the reduction of the oracle's eval == the reduction of the device's eval."""
    elig = None if ids is None else np.concatenate([np.ones((1, sets.shape[1]), bool), sets])[np.asarray(ids)]
    ref = o.eval(pods, now)
    want = reduce_eval(ref["status"], ref["reason"], present, elig)
    got = ev.diagnose(pods, now, node_sets=ids, bitmaps=True)
    assert_same(got, want, what + " vs oracle")
    assert np.array_equal(got["n_nodes"] + got["n_absent"], np.full(len(pods), ev.num_nodes))
    dev = ev.eval(pods, now, node_sets=ids)
    assert_same(got, reduce_eval(dev["status"], dev["reason"], present), what + " vs ke_eval")
    return got, want


def raw_diagnose(ev, pods, now, which=(True, True, True), extra_words=0):
    """ke_diagnose through the C ABI with any subset of the bitmaps and words_per_pod = the minimum + extra_words;
    the words come back as they are (uint64 [P, words_per_pod], None for a bitmap not asked for)."""
    pods = as_pod_array(pods)
    P, N = len(pods), ev.num_nodes
    wpp = (N + 63) // 64 + extra_words
    rec = np.zeros(P, abi.POD_DIAGNOSIS_DTYPE)
    words = [np.full((P, wpp), 0xA5A5A5A5A5A5A5A5, np.uint64) if w else None for w in which]
    ev._check(ev.lib.ke_diagnose(ev.h, P, abi.ptr(pods), int(now), abi.ptr(rec), wpp, *[abi.ptr(w) for w in words]))
    return rec, words


def both(cfg, n, loaders):
    ev, o = Evaluator(cfg), Oracle(cfg, n)
    for h in (ev, o):
        for load in loaders:
            load(h)
    return ev, o


def plain(n, k, cfg=None):
    cl = synth.make_cluster(n, S + k)
    return both(cfg or synth.config(n), n, [lambda h: synth.load_into(h, cl)]) + (cl,)


# ---- 1 plain: two eval blocks, a 13-lane last wave, a partial last word ----------------------------------------------
def test_plain(gpu):
    ev, o, _ = plain(333, 1)
    pods = synth.make_pods(40, S + 2)
    got, want = check(ev, o, pods, what="plain")
    worth_running(want)
    assert got["plugins"].max() == abi.PLUGIN_LOADAWARE  # LoadAware reasons only in a plain cluster
    assert [reason_plugin(r) for r in (1, 2, 3)] == [abi.PLUGIN_LOADAWARE] * 3


@pytest.mark.parametrize("n", [333, 2300])
def test_block_mappings_agree(gpu, n, monkeypatch):
    """The XCD-aware block mapping (the default) and the plain one (a context created under KOORDEVAL_DIAG_XCD=0)
    give the same diagnosis.  333 nodes are 2 tiles padded to 8 (dead tiles).  2300 nodes are beyond the cases listed
    for this file and above its 400-node bound on purpose: the decode's second row of eight tiles (9 tiles padded to
    16) exists only past 2048 nodes, and 20 pods there still run in well under a second."""
    cl = synth.make_cluster(n, S + 3)
    cfg = synth.config(n)
    o = Oracle(cfg, n)
    synth.load_into(o, cl)
    pods = synth.make_pods(20, S + 4)
    ref = o.eval(pods, T0)
    want = reduce_eval(ref["status"], ref["reason"])
    worth_running(want)
    for knob in ("1", "0", None):  # read once, when the context is created
        if knob is None:
            monkeypatch.delenv("KOORDEVAL_DIAG_XCD", raising=False)
        else:
            monkeypatch.setenv("KOORDEVAL_DIAG_XCD", knob)
        with Evaluator(cfg) as ev:
            synth.load_into(ev, cl)
            assert_same(ev.diagnose(pods, T0, bitmaps=True), want, f"mapping {knob}")


# ---- 2 edges: the wave / block / EVAL_PPB boundaries, words_per_pod exact and larger ---------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_edges(gpu, n):
    ev, o, _ = plain(n, 10 + n)
    all_pods = synth.make_pods(9, S + 11)
    for P in (1, 8, 9):
        pods = all_pods[:P]
        ref = o.eval(pods, T0)
        want = reduce_eval(ref["status"], ref["reason"])
        for extra in (0, 3):
            rec, words = raw_diagnose(ev, pods, T0, extra_words=extra)
            wpp = (n + 63) // 64
            for k in COUNTS + ("reason_nodes", "plugins"):
                assert np.array_equal(rec[k], want[k]), (n, P, extra, k)
            for k, w in zip(BITMAPS, words):
                assert w.shape == (P, wpp + extra)
                assert np.array_equal(unpack_node_sets(w[:, :wpp], n), want[k]), (n, P, extra, k)
                assert (w[:, wpp:] == 0).all(), (n, P, extra, k)  # the extra words
                assert (unpack_node_sets(w[:, :wpp], wpp * 64)[:, n:] == 0).all(), (n, P, extra, k)  # the tail bits


# ---- 3 deleted node slots and capacity above the populated range -----------------------------------------------------
def test_deleted_nodes(gpu):
    n, cap = 200, 320
    cl = synth.make_cluster(n, S + 20)
    cfg = synth.config(cap)
    ev, o = both(cfg, n, [lambda h: synth.load_into(h, cl)])
    gone = [0, 63, 64, 130, 199]
    for h in (ev, o):
        for i in gone:
            h.delete_node(i)
    present = np.ones(ev.num_nodes, bool)
    present[gone] = False
    assert ev.num_nodes == n
    pods = synth.make_pods(24, S + 21)
    got, want = check(ev, o, pods, present=present, what="deleted")
    worth_running(want)
    assert (got["n_absent"] == len(gone)).all() and (got["n_nodes"] == n - len(gone)).all()
    for k in BITMAPS:
        assert not got[k][:, gone].any(), k


# ---- 4 node sets -----------------------------------------------------------------------------------------------------
def test_node_sets(gpu):
    n = 333
    ev, o, _ = plain(n, 30)
    pods = synth.make_pods(40, S + 31)
    rng = np.random.default_rng(S + 32)
    sets = rng.random((3, n)) < 0.45
    ids = rng.integers(0, 4, len(pods))
    ids[:4] = [0, 1, 2, 3]
    ev.node_sets_load(sets)
    got, want = check(ev, o, pods, ids=ids, sets=sets, what="sets")
    worth_running(want)
    elig = np.concatenate([np.ones((1, n), bool), sets])[ids]
    assert np.array_equal(got["reason_nodes"][:, abi.REASON_NODE_SET], (~elig).sum(1))
    assert np.array_equal((got["plugins"] & abi.PLUGIN_NODE_SET) != 0, (~elig).any(1))
    # the ids were consumed: the next call is the plain one
    ref = o.eval(pods, T0)
    again = ev.diagnose(pods, T0, bitmaps=True)
    assert_same(again, reduce_eval(ref["status"], ref["reason"]), "after the sets")
    assert (again["reason_nodes"][:, abi.REASON_NODE_SET] == 0).all()


# ---- 5 NUMA policies: the deferred pairs finish in k_numa_finish's diagnosis mode ------------------------------------
def test_numa(gpu):
    n = 200
    cl = synth.make_cluster(n, S + 40, amplified_fraction=0.3)
    zs = synth.make_numa(cl, S + 41, zone_counts=(8,))
    ev, o = both(synth.config(n), n, [lambda h: synth.load_into(h, cl), lambda h: synth.load_numa(h, zs)])
    pods = synth.make_numa_pods(40, S + 42)
    got, want = check(ev, o, pods, what="numa")
    worth_running(want)
    assert (got["plugins"] & abi.PLUGIN_NODENUMARESOURCE).any() and (got["plugins"] & abi.PLUGIN_LOADAWARE).any()
    assert want["n_unresolvable"].sum() > 0 and want["n_unschedulable"].sum() > 0
    ev.diagnose(pods, T0)
    assert ev.numa_deferred() > 0  # the deferred mode ran (and its pairs are in the counts compared above)


# ---- 6 DeviceShare, and a pod whose PreFilter failed -----------------------------------------------------------------
def test_deviceshare(gpu):
    n = 96
    cl = synth.make_cluster(n, S + 50)
    dv = synth.make_devices(n, S + 51)
    ev, o = both(synth.config(n), n, [lambda h: synth.load_into(h, cl), lambda h: synth.load_devices(h, dv)])
    pods = synth.make_ds_pods(36, S + 52, device_fraction=0.8)
    bad = synth.make_ds_pods(1, S + 53, device_fraction=0.0)
    bad["device_requests"][0][abi.PDR["koordinator.sh/gpu-memory-ratio"]] = 150  # invalid: > 100, not a multiple
    bad["has_other_requests"][0] = 1
    pods = np.concatenate([pods, bad])
    got, want = check(ev, o, pods, what="deviceshare")
    worth_running(want)
    assert (got["plugins"] & abi.PLUGIN_DEVICESHARE).any()
    # the PreFilter failure: every node unresolvable with the host's reason
    assert got["n_unresolvable"][-1] == n and got["reason_nodes"][-1, abi.REASON_DS_INVALID_REQUEST] == n
    assert got["unresolvable"][-1].all() and got["plugins"][-1] == abi.PLUGIN_DEVICESHARE


# ---- 7 cpuset pods ---------------------------------------------------------------------------------------------------
def test_cpuset(gpu):
    n = 120
    cl = synth.make_cluster(n, S + 60, amplified_fraction=0.3)
    tabs = synth.make_cpus(cl, S + 61)
    ev, o = both(synth.config(n), n, [lambda h: synth.load_into(h, cl), lambda h: synth.load_cpus(h, tabs)])
    pods = synth.make_cpuset_pods(40, S + 63)
    got, want = check(ev, o, pods, what="cpuset")
    worth_running(want, reasons=5)
    assert (want["n_feasible"] == 0).any()  # a pod with no feasible node


# ---- 7b NUMA state and cpuset pods together: k_diag_eval<NUMA, CPU> and the cpuset finish into the diagnosis ----------
def test_numa_cpuset(gpu):
    """The cluster and pods of test_gpu_cpuset.py::test_numa_cpuset_eval_matrix_parity[mixed] (the `mixed` variant
    defers pairs, so it is the one used)."""
    ev, o = numa_cpuset_both(240, 401, **NUMA_VARIANTS["mixed"])
    pods = synth.make_numa_cpuset_pods(72, synth.BASE_SEED + 403)
    got, want = check(ev, o, pods, what="numa + cpuset")
    worth_running(want)
    ev.diagnose(pods, T0)
    assert ev.numa_deferred() > 0  # the deferral ran with binding pods (its pairs are in the counts compared above)


# ---- 8 NodeResourcesFit's Filter after a saturated queue -------------------------------------------------------------
@pytest.fixture(scope="module")
def saturated():
    n = 10
    cl = synth.make_cluster(n, synth.BASE_SEED + 41)
    cfg = synth.fit_config(synth.config(n))
    tables = synth.make_node_resources(cl, synth.BASE_SEED + 43)
    pods = synth.add_fit_defaults(synth.add_pod_xres(synth.make_pods(600, synth.BASE_SEED + 42), synth.BASE_SEED + 44))
    loaders = [lambda h: synth.load_into(h, cl), lambda h: synth.load_node_resources(h, tables)]
    # the lock-step oracle: one pod at a time, a failed pod's as-of eval taken at its own turn
    step = Oracle(cfg, n)
    for load in loaders:
        load(step)
    chosen, asof = np.zeros(len(pods), np.int32), {}
    for p in range(len(pods)):
        chosen[p] = step.schedule(pods[p:p + 1], T0)[0][0]
        if chosen[p] < 0:
            e = step.eval(pods[p:p + 1], T0)
            asof[p] = (e["status"][0].copy(), e["reason"][0].copy())
    return cfg, n, loaders, pods, chosen, asof


def test_fit_filter_after_a_saturated_queue(gpu, saturated):
    cfg, n, loaders, pods, step_chosen, asof = saturated
    ev, o = both(cfg, n, loaders)
    c1, c0 = ev.schedule(pods, T0)[0], o.schedule(pods, T0)[0]
    assert np.array_equal(c1, c0) and np.array_equal(c0, step_chosen)
    failed = np.nonzero(c1 < 0)[0]
    assert len(failed) > 400
    asof_reasons = np.unique(np.concatenate([asof[p][1] for p in failed]))
    assert {abi.REASON_FIT_INSUFFICIENT_MEMORY, abi.REASON_FIT_INSUFFICIENT_SCALAR} <= set(asof_reasons.tolist())
    assert len(asof_reasons[asof_reasons > 0]) >= 3
    # the diagnosis is of the state at the call: the oracle's eval at the end of its own queue
    ref = o.eval(pods[failed], T0)
    want = reduce_eval(ref["status"], ref["reason"])
    got = ev.diagnose(pods[failed], T0, bitmaps=True)
    assert (want["reason_nodes"][:, 1:].sum(0) > 0).sum() >= 3  # the end-of-queue reference is mixed-reason too
    assert_same(got, want, "saturated")
    assert (got["n_feasible"] == 0).all()
    assert (got["plugins"] & abi.PLUGIN_NODERESOURCESFIT).any()
    # ... and agrees with a failed pod's own view on every node no later pod of the queue chose
    for j, p in enumerate(failed):
        later = np.zeros(n, bool)
        tail = step_chosen[p + 1:]
        later[tail[tail >= 0]] = True
        st = asof[p][0]
        for k in BITMAPS:
            assert np.array_equal(got[k][j][~later], (st == CODE_OF[k])[~later]), (p, k)


# ---- 9 time: now_ns past the NodeMetric expiry -----------------------------------------------------------------------
def test_time_moves_nodes_to_expired(gpu):
    ev, o, _ = plain(300, 70)
    pods = synth.make_pods(16, S + 71)
    g0, w0 = check(ev, o, pods, now=T0, what="now")
    worth_running(w0)
    late = T0 + 3600 * synth.NS
    g1, w1 = check(ev, o, pods, now=late, what="late")
    r = abi.REASON_LA_NODEMETRIC_EXPIRED
    assert w1["reason_nodes"][:, r].sum() > w0["reason_nodes"][:, r].sum()
    assert g1["reason_nodes"][:, r].sum() > g0["reason_nodes"][:, r].sum()


# ---- 10 no side effects ----------------------------------------------------------------------------------------------
def test_no_side_effects(gpu):
    n = 300
    ev, o, _ = plain(n, 80, synth.config(n))
    pods = synth.make_pods(200, S + 81)
    probe = synth.make_pods(24, S + 82, key_base=7_000_000_000)
    ref = o.eval(probe, T0)
    worth_running(reduce_eval(ref["status"], ref["reason"]))
    before = ev.eval(probe, T0)
    ev.diagnose(probe, T0, bitmaps=True)
    ev.diagnose(pods[:9], T0)
    after = ev.eval(probe, T0)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert ev.check_records(T0) == 0
    got, want = ev.schedule(pods[:100], T0), o.schedule(pods[:100], T0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # between submit and wait: the diagnosis completes the call in flight and sees its Reserves
    t = ev.submit(pods[100:], T0)
    mid = ev.diagnose(probe, T0, bitmaps=True)
    got = ev.wait(t)
    want = o.schedule(pods[100:], T0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    ref = o.eval(probe, T0)
    assert_same(mid, reduce_eval(ref["status"], ref["reason"]), "in flight")
    assert ev.check_records(T0) == 0


# ---- 11 any subset of the bitmaps gives the same counts --------------------------------------------------------------
def test_bitmap_subsets(gpu):
    n = 130
    ev, o, _ = plain(n, 90)
    pods = synth.make_pods(12, S + 91)
    ref = o.eval(pods, T0)
    want = reduce_eval(ref["status"], ref["reason"])
    worth_running(want)
    for mask in range(8):
        which = tuple(bool(mask >> b & 1) for b in range(3))
        rec, words = raw_diagnose(ev, pods, T0, which=which)
        for k in COUNTS + ("reason_nodes", "plugins"):
            assert np.array_equal(rec[k], want[k]), (which, k)
        for k, w, on in zip(BITMAPS, words, which):
            assert (w is not None) == on
            if on:
                assert np.array_equal(unpack_node_sets(w, n), want[k]), (which, k)
    # without a bitmap words_per_pod is ignored
    pa = as_pod_array(pods)
    rec = np.zeros(len(pa), abi.POD_DIAGNOSIS_DTYPE)
    ev._check(ev.lib.ke_diagnose(ev.h, len(pa), abi.ptr(pa), int(T0), abi.ptr(rec), -5, None, None, None))
    assert np.array_equal(rec["reason_nodes"], want["reason_nodes"])
    assert C.sizeof(abi.PodDiagnosis) == 32 + 4 * abi.DIAG_REASONS
