"""The boundary between consecutive ke_schedule_submit calls: a plain call enqueues one packed
upload, one call-begin kernel and one read-back (plus the context's error word), and no fill, on the Reserve
stream, whatever its run structure, and places exactly as the oracle and as one ke_schedule over the whole queue.
No batch of a call starts ahead of the previous call's end (priming the first two batches during the previous
run's tail was built and measured slower; the cases below are the ones it had to pass).  Small
batches (pod_batch = 8) make a 40-pod slice a 5-batch run, so each call boundary lies between two pipelined runs."""
import numpy as np
import pytest

from koordinator_amd import Evaluator, abi, synth
from oracle.binding import Oracle

pytestmark = pytest.mark.gpu

B = 8


def _pair(n, seed, twin=False):
    cl = synth.make_cluster(n, synth.BASE_SEED + seed)
    cfg = synth.config(n, pod_batch=B)
    hs = [Evaluator(cfg), Oracle(cfg, n)] + ([Evaluator(cfg)] if twin else [])
    for h in hs:
        synth.load_into(h, cl)
    return hs


def _plain_boundary(cb, behind):
    """A plain call's ke_debug_call_boundary figures: no batch ahead of the previous call's end, three copies and no
    fill on the Reserve stream, and a device-side boundary only behind a call in flight."""
    assert cb["primed_batches"] == 0, cb
    assert cb["reserve_stream_copies"] == 3 and cb["reserve_stream_fills"] == 0, cb
    if behind:
        assert 0 < cb["boundary_ns"] < 2_000_000_000, cb
    else:
        assert cb["boundary_ns"] == 0, cb


def _one_ahead(ev, slices, now=synth.T0):
    """Submit every slice one ahead of the previous one's collection; returns (chosen, score, boundary) per slice."""
    out, prev = [], None
    for i, q in enumerate(slices):
        t = ev.submit(q, now[i] if isinstance(now, (list, tuple)) else now)
        if prev is not None:
            out.append(ev.wait(prev) + (ev.call_boundary(),))
        prev = t
    out.append(ev.wait(prev) + (ev.call_boundary(),))
    return out


def test_six_runs_one_ahead(gpu):
    ev, o, one = _pair(600, 1401, twin=True)
    pods = synth.make_pods(240, synth.BASE_SEED + 1402)
    got = _one_ahead(ev, [pods[i * 40:(i + 1) * 40] for i in range(6)])
    c0, s0 = o.schedule(pods, synth.T0)
    c1, s1 = one.schedule(pods, synth.T0)
    gc, gs = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
    assert np.array_equal(gc, c0) and np.array_equal(gs, s0)
    assert np.array_equal(gc, c1) and np.array_equal(gs, s1)
    for i, g in enumerate(got):
        _plain_boundary(g[2], behind=i > 0)
    assert ev.kernel_stats()["pipelined_batches"] == 5
    dev, host = ev.debug_rows(synth.T0)
    assert np.array_equal(dev, host)
    assert ev.check_records(synth.T0) == 0
    ev.close()
    one.close()


def test_run_lengths(gpu):
    """Slices of 16, 24, 27, 8 and 40 pods: runs of 2 and 3 batches, 3 full batches and a partial one, a single
    batch (serial, no run) and 5."""
    ev, o = _pair(600, 1403)
    lens = [16, 24, 27, 8, 40]
    pods = synth.make_pods(sum(lens), synth.BASE_SEED + 1404)
    cuts = np.cumsum([0] + lens)
    sl = [pods[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    got = _one_ahead(ev, sl)
    for i, (q, g) in enumerate(zip(sl, got)):
        c0, s0 = o.schedule(q, synth.T0)
        assert np.array_equal(g[0], c0) and np.array_equal(g[1], s0), i
        _plain_boundary(g[2], behind=i > 0)
    dev, host = ev.debug_rows(synth.T0)
    assert np.array_equal(dev, host)
    assert ev.check_records(synth.T0) == 0
    ev.close()


CONTENDED_SEED = 1405


def contended_queue(o, n_calls=8, per_call=24):
    """48 nodes, 24-pod slices: returns the slices and the oracle's (chosen, score) per slice, after checking that
    in every call but the first some pod of the first batch lands on a node that one of the previous call's last
    two batches reserved -- the nodes a first batch gets wrong if it does not see all of the previous call's
    Reserves."""
    pods = synth.make_pods(n_calls * per_call, synth.BASE_SEED + CONTENDED_SEED + 1)
    sl = [pods[i * per_call:(i + 1) * per_call] for i in range(n_calls)]
    exp = [o.schedule(q, synth.T0) for q in sl]
    for i in range(1, n_calls):
        tail = exp[i - 1][0][-2 * B:]
        head = exp[i][0][:B]
        assert np.intersect1d(head[head >= 0], tail[tail >= 0]).size > 0, i
    return sl, exp


def test_boundary_contention(gpu):
    ev, o = _pair(48, CONTENDED_SEED)
    sl, exp = contended_queue(o)
    got = _one_ahead(ev, sl)
    for i, (g, (c0, s0)) in enumerate(zip(got, exp)):
        assert np.array_equal(g[0], c0) and np.array_equal(g[1], s0), i
        _plain_boundary(g[2], behind=i > 0)
    dev, host = ev.debug_rows(synth.T0)
    assert np.array_equal(dev, host)
    assert ev.check_records(synth.T0) == 0
    ev.close()


def test_event_between_submissions_and_moving_clock(gpu):
    """An informer event between two submissions completes the call in flight (the next call is not behind
    one); a different now_ns per call keeps the later ones behind each other."""
    ev, o = _pair(600, 1407)
    q = [synth.make_pods(40, synth.BASE_SEED + 1408 + i, key_base=5_000_000_000 + i * 10_000) for i in range(4)]
    now = [synth.T0 + i * 1_000_000 for i in range(4)]
    other = abi.Pod.from_buffer_copy(synth.make_pods(1, synth.BASE_SEED + 1412, key_base=7_000_000_000)[0].tobytes())
    t0 = ev.submit(q[0], now[0])
    exp0 = o.schedule(q[0], now[0])
    for h in (ev, o):  # (the call in flight completes before the event applies)
        h.assign(17, other, now[0])
    t1 = ev.submit(q[1], now[1])
    t2 = ev.submit(q[2], now[2])
    g0 = ev.wait(t0)
    g1 = ev.wait(t1)
    cb1 = ev.call_boundary()
    t3 = ev.submit(q[3], now[3])
    g2 = ev.wait(t2)
    cb2 = ev.call_boundary()
    g3 = ev.wait(t3)
    cb3 = ev.call_boundary()
    exp = [exp0] + [o.schedule(q[i], now[i]) for i in (1, 2, 3)]
    for g, (c0, s0) in zip((g0, g1, g2, g3), exp):
        assert np.array_equal(g[0], c0) and np.array_equal(g[1], s0)
    _plain_boundary(cb1, behind=False)  # the event drained the call in flight
    _plain_boundary(cb2, behind=True)
    _plain_boundary(cb3, behind=True)
    dev, host = ev.debug_rows(now[3])
    assert np.array_equal(dev, host)
    ev.close()


@pytest.mark.parametrize("pipeline", [False, "fixup"])
def test_other_schedules_keep_the_packed_boundary(gpu, pipeline):
    ev, o = _pair(600, 1413)
    ev.set_pipeline(pipeline)
    pods = synth.make_pods(120, synth.BASE_SEED + 1414)
    sl = [pods[i * 40:(i + 1) * 40] for i in range(3)]
    got = _one_ahead(ev, sl)
    for i, (q, g) in enumerate(zip(sl, got)):
        c0, s0 = o.schedule(q, synth.T0)
        assert np.array_equal(g[0], c0) and np.array_equal(g[1], s0), i
        # (without the pipeline a submission runs at once: never behind a call in flight)
        _plain_boundary(g[2], behind=i > 0 and pipeline is not False)
    assert ev.check_records(synth.T0) == 0
    ev.close()


def test_deviceshare_slice_between_plain_ones(gpu):
    """A DeviceShare slice runs at once behind the completed plain one (its own copies on top of the packed
    three); the plain slice after it starts with no call in flight."""
    from test_gpu_parity import ds_both
    ev, o = ds_both(600, 1415, abi.STRATEGY_LEAST_ALLOCATED)
    qs = [synth.make_pods(40, synth.BASE_SEED + 1416), synth.make_ds_pods(24, synth.BASE_SEED + 1417, key_base=6_000_000_000),
          synth.make_pods(40, synth.BASE_SEED + 1418, key_base=6_100_000_000)]
    ts = [ev.submit(q, synth.T0) for q in qs]
    exp = [o.schedule(q, synth.T0) for q in qs]
    cbs = []
    for t, (c0, s0) in zip(ts, exp):
        c, s = ev.wait(t)
        cbs.append(ev.call_boundary())
        assert np.array_equal(c, c0) and np.array_equal(s, s0)
    assert all(cb["primed_batches"] == 0 for cb in cbs)
    assert ev.check_records(synth.T0) == 0
    ev.close()
