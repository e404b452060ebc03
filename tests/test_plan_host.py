"""The host plan of a ke_schedule call (koordinator_amd/csrc/ke_plan.h: the select's geometry, the batch segmentation
and pipelined runs, the staging layouts, the call's statistics) compiled for the host with g++
(tests/plan/plan_check.cpp) and compared with restatements here and in landscapes.py."""
import os
import random
import subprocess

import pytest

import landscapes as L

HERE = os.path.dirname(os.path.abspath(__file__))
PST = 16
DS, CPUSET, HINT = 1, 2, 4


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(HERE, "plan", "plan_check.cpp")], check=True)
    return exe


def run(exe, mode, text=""):
    r = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.splitlines()


# ---- geometry --------------------------------------------------------------------------------------------------------
NODES = (4095, 4096, 8200, 20000, 24575, 24576, 50000, 66061, 140003, 196608, 811264, 1048832)
BATCHES = (1, 2, 7, 32, 64)
KNOBS = (None, "1", "2", "8")
LIST_LEN = (64, 128, 192)


def test_select_geometry_equals_landscapes(plan_check):
    rows = {}
    for line in run(plan_check, "geometry"):
        f = line.split()
        key = (int(f[0]), int(f[1]), None if f[2] == "-" else f[2], int(f[3]))
        rows[key] = dict(kext=int(f[4]), parts=int(f[5]), part=int(f[6]), rc_one=int(f[7]), rc_split=int(f[8]),
                         sorted=int(f[9]), segs=[int(x) for x in f[10:]])
    assert len(rows) == len(NODES) * len(BATCHES) * len(KNOBS) * len(LIST_LEN)
    for n in NODES:
        for batch in BATCHES:
            for knob in KNOBS:
                for ll in LIST_LEN:
                    got = rows[(n, batch, knob, ll)]
                    parts = L.select_parts(n, batch, knob, ll)
                    g = L.select_boundaries(n, parts)
                    assert got["parts"] == parts, (n, batch, knob, ll)
                    assert got["part"] == g["part"], (n, batch, knob, ll)
                    assert got["segs"] == [p["seg"] for p in g["parts"]], (n, batch, knob, ll)
                    # register-resident exactly when the largest wave segment is not streamed
                    assert (got["rc_split"] if parts > 1 else got["rc_one"]) == (not g["streamed"]), (n, batch, knob, ll)
                    assert got["kext"] == ll - 64 and got["sorted"] == (ll == 192 or parts > 1)
                # what the sortedness of exact (64) and stale (128) lists rests on: the same parts for both lengths
                assert rows[(n, batch, knob, 64)]["parts"] == rows[(n, batch, knob, 128)]["parts"], (n, batch, knob)


# ---- segmentation and runs -------------------------------------------------------------------------------------------
def sequences():
    rnd = random.Random(20261019)
    out = []
    for _ in range(200):
        n = rnd.choice((0, 1, 2, 5, 64, 65, 130, 300, rnd.randrange(301)))
        p_special = rnd.choice((0.0, 0.02, 0.1, 0.5))
        out.append([rnd.choice((DS, CPUSET, HINT, DS | HINT, DS | CPUSET)) if rnd.random() < p_special else 0
                    for _ in range(n)])
    return out


def batches_of(flags, B, ds_batch, fused):
    """The segmentation rules restated: (pods, ds, cpu, cut, hint) per batch."""
    n = len(flags)

    def alone(p):
        f = flags[p]
        return bool(f & CPUSET) or bool(f & HINT) or (bool(f & DS) and not ds_batch) or (fused and p == n - 1)
    out, p = [], 0
    while p < n:
        if alone(p):
            out.append((1, int(bool(flags[p] & DS)), int(bool(flags[p] & CPUSET)), 0, int(bool(flags[p] & HINT))))
            p += 1
            continue
        q = p
        while q < n and q - p < B and not alone(q):
            q += 1
        has_ds = any(f & DS for f in flags[p:q])
        out.append((q - p, int(has_ds), 0, int(has_ds and q - p > 1), 0))
        p = q
    return out


def runs_of(batches, pipeline, numa, nodes, fused):
    """run_end restated: maximal stretches of >= 2 eligible batches."""
    nb = len(batches)
    ok = [pipeline and nodes > 0 and not numa and not b[1] and not b[2] and not (fused and i == nb - 1)
          for i, b in enumerate(batches)]
    out, i = [0] * nb, 0
    while i < nb:
        j = i
        while j < nb and ok[j]:
            j += 1
        if j - i >= 2:
            out[i] = j
        i = max(j, i + 1)
    return out


RUN_VARIANTS = ((True, False, 100), (False, False, 100), (True, True, 100), (True, False, 0))


def test_batches_and_runs(plan_check):
    cases = [(flags, B, ds_batch, fused) for flags in sequences() for B in (1, 7, 64) for ds_batch in (0, 1)
             for fused in (0, 1)]
    text = "".join("%d %d %d %d %s\n" % (B, ds_batch, fused, len(flags), " ".join(map(str, flags)))
                   for flags, B, ds_batch, fused in cases)
    lines = run(plan_check, "segment", text)
    assert len(lines) == len(cases)
    n_runs = 0
    for (flags, B, ds_batch, fused), line in zip(cases, lines):
        parts = line.split("|")
        f = [int(x) for x in parts[0].split()]
        got = [tuple(f[i:i + 5]) for i in range(0, len(f), 5)]
        assert got == batches_of(flags, B, ds_batch, fused), (flags, B, ds_batch, fused)
        # the invariants, on the program's output itself
        n = len(flags)
        assert sum(b[0] for b in got) == n  # (in order: plan_check checks the bases)
        p = 0
        for pods, ds, cpu, cut, hint in got:
            fl = flags[p:p + pods]
            assert 1 <= pods <= B
            single = [bool(x & (CPUSET | HINT)) or (bool(x & DS) and not ds_batch) for x in fl]
            assert pods == 1 or not any(single)
            assert pods == 1 or not (fused and p + pods == n)  # the fused last pod is alone
            assert ds == int(any(x & DS for x in fl)) and cpu == int(any(x & CPUSET for x in fl))
            assert hint == int(any(x & HINT for x in fl))
            assert cut == int(bool(ds) and pods > 1)
            p += pods
        for (pipeline, numa, nodes), rl in zip(RUN_VARIANTS, parts[1:]):
            run_end = [int(x) for x in rl.split()]
            assert run_end == runs_of(got, pipeline, numa, nodes, fused), (flags, B, ds_batch, fused)
            if not pipeline or numa or nodes == 0:
                assert not any(run_end)
            nb = len(got)
            elig = [not b[1] and not b[2] and not (fused and i == nb - 1) for i, b in enumerate(got)]
            covered = [False] * nb
            for s, e in enumerate(run_end):
                if e:
                    n_runs += 1
                    assert e - s >= 2 and all(elig[s:e]) and not any(covered[s:e])
                    assert (s == 0 or not elig[s - 1]) and (e == nb or not elig[e])  # maximal
                    covered[s:e] = [True] * (e - s)
            if pipeline and not numa and nodes > 0:  # every stretch of >= 2 eligible batches is in a run
                for i in range(nb - 1):
                    assert not (elig[i] and elig[i + 1]) or (covered[i] and covered[i + 1])
    assert n_runs > 1000


# ---- layouts ---------------------------------------------------------------------------------------------------------
def test_layouts(plan_check):
    out, sched, host = {}, {}, {}
    for line in run(plan_check, "layouts"):
        f = line.split()
        v = [int(x) for x in f[1:]]
        if f[0] == "out":
            out[(v[0], v[1])] = v[2:]
        elif f[0] == "sched":
            sched[v[0]] = v[1:]
        else:
            host[(v[0], v[1], v[2])] = v[3:]
    assert sorted(out) == [(1, 1), (64, 1), (5000, 79), (5000, 5000)]
    for (p, b), (score, chosen, err, fst, st, pst, est, end, total, total_pp) in out.items():
        sizes = [4 * p, 4 * p, 8, 16 * b, 8 * (b + 1), 8 * PST * b, 8 * b]
        offs = [score, chosen, err, fst, st, pst, est]  # the order the completion reads them in
        assert score == 0 and all(o % 16 == 0 for o in offs)
        for i in range(len(offs) - 1):
            assert offs[i] + sizes[i] <= offs[i + 1]  # disjoint, in order
        assert fst == err + 16  # k_call_begin zeroes the error word and the fixup stamps as one range [err, st)
        assert st == fst + 16 * b
        assert end == est + 8 * b and total == end + 8  # (one more eval stamp, not read back)
        assert total_pp >= total  # the block is allocated for (p, p): at most one batch per pod
    assert out[(5000, 5000)][-2] == out[(5000, 79)][-1] > out[(5000, 79)][-2]
    for b, (ready, done, tready, sstart, rres, words, tlist, tmx, total) in sched.items():
        arrays = [ready, done, tready, sstart, rres]
        assert arrays == [i * (b + 1) for i in range(5)] and rres + (b + 1) <= words  # [n] each with a spare word
        assert tlist == words and tlist % 2 == 0 and tmx % 2 == 0  # (int32 words: 8-byte aligned lists)
        assert tmx == tlist + 2 * (1 + 64) and total == tmx + 2 * 64
    for (p, b, ws), (blk0, blk_bytes, score, chosen, err, fst, st, pst, est, kerr, dev, cs, vf, numa, dcnt, total) in host.items():
        o = dict(zip(("score", "chosen", "err", "fst", "st", "pst", "est", "end"), out[(p, b)][:8]))
        assert blk0 == (o["score"] if ws else o["chosen"]) and blk_bytes == o["end"] - blk0
        assert [chosen, err, fst, st, pst, est] == [o[x] - blk0 for x in ("chosen", "err", "fst", "st", "pst", "est")]
        tail = [kerr, dev, cs, vf, numa, dcnt, total]
        sizes = [4, 8 * p, 32 * p, 2 * 16 * p, 8 * 16 * p, 4 * b]
        assert kerr >= blk_bytes and all(x % 16 == 0 for x in tail)
        for i in range(6):
            assert tail[i] + sizes[i] <= tail[i + 1]


# ---- the call's statistics -------------------------------------------------------------------------------------------
def test_call_stats(plan_check):
    """Three batches of 2, 3 and 1 pods: a serial batch (the one-wave replay) and a run of two (speculative replays).
    Every duration below is chosen here, in ticks of 1e-5 ms."""
    tick = 1e-5
    nb, pods = 3, (2, 3, 1)
    t0 = 1_000_000
    wait = (500, 300, 700)        # eval start -> the Reserve prologue's start
    est, p0, st = [], [], [t0]
    pro = (1000, 2000, 4000)      # prologue
    P, RS, V, later, wb = (0, 600, 800), (0, 1500, 1700), (0, 250, 350), (0, 0, 900), (5000, 400, 300)
    handoff = 120                 # batch 2's prologue starts this long after batch 1's end
    tset, loop, w1t, w0r = (0, 100, 140), (0, 300, 0), (0, 450, 470), (0, 80, 60)
    pst = []
    for b in range(nb):
        start = st[b] + (handoff if b == 2 else 2000)
        est.append(start - wait[b])
        p = [0] * PST
        p[0], p[4] = start, start + pro[b]
        if b > 0:
            p[1] = p[4] + P[b]
            p[2] = p[1] + RS[b]
            p[3] = p[2] + V[b]
            p[5] = p[3] + later[b]
            p[8] = p[4] + tset[b]
            p[9] = p[8] + loop[b]       # (0 for batch 2: counts as 0 whatever p[9] - p[8] is)
            p[10] = p[8] + w1t[b]
            p[11] = p[1] + w0r[b]
            p[12] = 1 if b == 2 else 0
            p[13], p[14], p[15] = 40, (30 << 32) | 20, p[8] + 900
            end = p[5] + wb[b]
        else:
            end = p[4] + wb[b]
        p[6] = ((b + 1) << 32) | (10 * (b + 1))  # rounds | rows fetched
        p[7] = 3 * (b + 1)
        pst += p
        p0.append(start)
        st.append(end)
    fst = [0, 0, 5000, 5000 + 777, 0, 0]
    dcnt = (1, 2, 4)
    span_ms = (st[nb] - st[0]) * tick
    sync_ms, prev_end, samples = 9.5, t0 - 2500, (0.25, 0.5, 0.75, 1.0)
    text = " ".join(map(str, [nb, sum(pods), 2, *pods, 0, 3, 0, *st, *pst, *est, *fst, *dcnt, repr(span_ms), sync_ms,
                              prev_end, 1, 3, 0, 1, 2, *samples]))
    got = {}
    for line in run(plan_check, "stats", text):
        f = line.split()
        got[f[0]] = [float(x) for x in f[1:]]
    ap = lambda x: pytest.approx(x, rel=1e-9, abs=1e-12)
    (total_ms, pipelined, prev_tick, eval_ms, select_ms, resolve_ms, fixup_ms, handoff_ms, spec_failed, rows_fetched,
     rows_changed, prologue_ms, loop_ms, numa_deferred, n_samples) = got["scalars"]
    assert total_ms == ap(span_ms) and pipelined == 2 and prev_tick == st[nb]
    assert got["batch_ms"] == ap([(st[b + 1] - est[b]) * tick for b in range(nb)])  # service: eval start -> Reserve end
    assert resolve_ms == ap(sum(st[b + 1] - p0[b] for b in range(nb)) * tick / nb)  # Reserve: prologue start -> end
    assert handoff_ms == ap(handoff * tick)  # (batch 2 alone: batch 1 is its run's first)
    assert fixup_ms == ap(777 * tick)
    assert prologue_ms == ap(sum(pro) * tick / nb)
    assert loop_ms == ap(sum(st[b + 1] - p0[b] - pro[b] for b in range(nb)) * tick / nb)
    # the phase sums; batch 0 (pst[1] <= pst[4], the one-wave replay) counts wholly as write-back
    assert got["phase"] == ap([sum(x) * tick / nb for x in (pro, P, RS, V, later, wb)])
    assert got["sub"] == ap([sum(tset) * tick / 2, sum(loop) * tick / 2, sum(w1t) * tick / 2, sum(w0r) * tick / 2, 1.0])
    assert got["wave1"] == ap([40 * tick, 20 * tick, 30 * tick, 900 * tick])  # (batch 2: the run's helper maxima)
    lat = [sync_ms - (st[nb] - st[b + 1]) * tick for b in range(nb)]
    assert got["pod_lat"] == ap([lat[0]] * 2 + [lat[1]] * 3 + [lat[2]])
    assert spec_failed == ap(2.0) and rows_fetched == ap(20.0) and rows_changed == ap(6.0)
    assert numa_deferred == 7 and n_samples == 2 and eval_ms == ap(0.5) and select_ms == ap(0.75)
    assert got["boundary"] == [0, 3, 0, pytest.approx((p0[0] - prev_end) * tick * 1e6, abs=1)]  # ns, truncated
