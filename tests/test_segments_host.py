"""The level above one device call (koordinator_amd/csrc/ke_segments.h: how ke_schedule cuts its queue into segments,
and the one record the segments' per-pod outputs are joined into) compiled for the host with g++
(tests/plan/segments_check.cpp) and compared with restatements written here from the rule's text."""
import itertools
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BARRIER, ALONE, IGNORED = 1, 2, 4
CS, VF, NUMA = 4, 32, 16
WIDTH = 1 + CS + VF + NUMA


@pytest.fixture(scope="module")
def segments_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("segments") / "segments_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(HERE, "plan", "segments_check.cpp")], check=True)
    return exe


def run(exe, mode, text=""):
    r = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.splitlines()


# ---- the segment plan ------------------------------------------------------------------------------------------------
def sequences():
    out = [list(s) for n in range(6) for s in itertools.product(range(8), repeat=n)]
    assert len(out) == 37449
    rnd = random.Random(20261021)
    for _ in range(200):
        n = rnd.choice((0, 1, 2, 5, 64, 65, 130, 300, rnd.randrange(301)))
        p_special = rnd.choice((0.0, 0.02, 0.1, 0.5))
        out.append([rnd.randrange(1, 8) if rnd.random() < p_special else 0 for _ in range(n)])
    return out


def takes(cls, p, ign):
    """The walk takes pod p: not a barrier, not alone, ignored as the segment's first pod."""
    return not cls[p] & BARRIER and not cls[p] & ALONE and bool(cls[p] & IGNORED) == ign


def segments_of(cls):
    """The rule restated: (s0, s1, ign, alone, barrier) per segment."""
    n = len(cls)
    if n == 0:
        return [(0, 0, 0, 0, 0)]  # one empty segment: the empty call still refreshes
    out, s0 = [], 0
    while s0 < n:
        ign = bool(cls[s0] & IGNORED)
        s1 = s0
        while s1 < n and takes(cls, s1, ign):
            s1 += 1
        if s1 < n:
            stop = cls[s1]
            if s1 == s0:  # the stopping pod joins an empty segment
                s1 += 1
            elif stop & BARRIER and not stop & ALONE and bool(stop & IGNORED) == ign:  # a barrier ends it inclusively
                s1 += 1
        out.append((s0, s1, int(ign), int(s1 - s0 == 1 and bool(cls[s0] & ALONE)), int(bool(cls[s1 - 1] & BARRIER))))
        s0 = s1
    return out


def test_segments(segments_check):
    seqs = sequences()
    text = "".join("%d %s\n" % (len(s), " ".join(map(str, s))) for s in seqs)
    lines = run(segments_check, "segments", text)
    assert len(lines) == len(seqs)
    n_multi = 0
    for cls, line in zip(seqs, lines):
        f = [int(x) for x in line.split()]
        got = [tuple(f[i:i + 5]) for i in range(0, len(f), 5)]
        assert got == segments_of(cls), cls
        # the properties, on the program's output itself
        n = len(cls)
        if n == 0:
            assert got == [(0, 0, 0, 0, 0)]
            continue
        assert got[0][0] == 0 and got[-1][1] == n
        n_multi += len(got) > 1
        for i, (s0, s1, ign, alone, barrier) in enumerate(got):
            assert s1 > s0 and (i == 0 or got[i - 1][1] == s0), cls  # the ranges tile [0, n) in order
            part = cls[s0:s1]
            assert len({bool(c & IGNORED) for c in part}) == 1 and ign == int(bool(part[0] & IGNORED)), cls
            for j, c in enumerate(part):
                assert not c & ALONE or len(part) == 1, cls        # an alone pod is a range of one
                assert not c & BARRIER or j == len(part) - 1, cls  # a barrier pod is the last of its range
            assert alone == int(len(part) == 1 and bool(part[0] & ALONE)) and barrier == int(bool(part[-1] & BARRIER))
            # no range could have been extended: it ends at a barrier, is an alone pod, or the next pod cannot join
            if s1 < n and not part[-1] & BARRIER and not part[0] & ALONE:
                nxt = cls[s1]
                assert nxt & ALONE or bool(nxt & IGNORED) != bool(ign), cls
    assert n_multi > 30000


# ---- the record ------------------------------------------------------------------------------------------------------
ABSENT = [0] + [0] * CS + [-1] * VF + [0] * NUMA


def make_pods(rnd, n):
    """Per pod: minors, 4 cpuset words, 32 VF ranks, 16 NUMA amounts -- every kind non-trivial for most pods."""
    pods = []
    for _ in range(n):
        dev = rnd.choice((0, rnd.getrandbits(64)))
        cs = [rnd.choice((0, rnd.getrandbits(64))) for _ in range(CS)]
        vf = [rnd.randrange(-1, 16) for _ in range(VF)]
        numa = [rnd.choice((0, rnd.randrange(-2 ** 62, 2 ** 62))) for _ in range(NUMA)]
        pods.append([dev] + cs + vf + numa)
    return pods


def masked(pod, has):
    """What a reader sees of a pod whose segment read back the kinds in `has` (dev, cpuset, VF, NUMA)."""
    out = list(ABSENT)
    for (a, b), h in zip(((0, 1), (1, 1 + CS), (1 + CS, 1 + CS + VF), (1 + CS + VF, WIDTH)), has):
        if h:
            out[a:b] = pod[a:b]
    return out


def draw_text(segs):
    """segs: (pods, cut, has); cut = 1: the last pod is a gated fused pod's, truncated away."""
    parts = [str(len(segs))]
    for pods, cut, has in segs:
        parts.append("%d %d %s" % (len(pods) - cut, cut, " ".join(str(int(h)) for h in has)))
        parts += [" ".join(map(str, p)) for p in pods]
    return "\n".join(parts) + "\n"


def parse_draws(lines):
    draws, i = [], 0
    while i < len(lines):
        tag, n = lines[i].split()
        assert tag == "D"
        n = int(n)
        rows = [[int(x) for x in ln.split()] for ln in lines[i + 1:i + 1 + 3 * (n + 2)]]
        draws.append((n, rows[:2 * (n + 2)], rows[2 * (n + 2):]))
        i += 1 + 3 * (n + 2)
    return draws


def check_draw(draw, truth):
    n, rows, allocs = draw
    assert n == len(truth)
    for p in range(n + 2):
        want = truth[p] if p < n else ABSENT
        assert rows[2 * p] == want, p       # the accessors
        assert rows[2 * p + 1] == want, p   # the flat views, the allocation record's VF ranks
        node, quota, vf_last = allocs[p][:3]
        got = allocs[p][3:4 + CS] + allocs[p][4 + CS + VF:]
        if p >= n or p % 7 == 3:            # beyond the call, or unreserved: a blank record
            assert (node, quota, vf_last) == (-1, 0, -1) and not any(got), p
        else:
            assert (node, quota, vf_last) == (100 + p, p % 2, want[CS + VF]), p
            assert got == want[:1 + CS] + want[1 + CS + VF:], p


def test_record_append_and_truncate(segments_check):
    rnd = random.Random(20261022)
    texts, truths = [], []
    for d in range(200):
        n = rnd.randrange(1, 41) if d else 40
        pods = make_pods(rnd, n)
        segs, truth, p = [], [], 0
        while p < n:
            ln = rnd.randrange(1, n - p + 1) if rnd.random() < 0.7 else 1
            has = [rnd.random() < 0.5 for _ in range(4)]
            segs.append((pods[p:p + ln], 0, has))
            truth += [masked(q, has) for q in pods[p:p + ln]]
            p += ln
        texts.append(draw_text(segs))
        truths.append(truth)
        # the last pod once more as a gated fused pod: read back with the segment before it, truncated away, then
        # appended as a segment of its own -- the same as never having fused it
        if len(segs) >= 2 and len(segs[-1][0]) == 1:
            before, last = segs[-2], segs[-1]
            fused = (before[0] + make_pods(rnd, 1), 1, before[2])
            texts.append(draw_text(segs[:-2] + [fused, last]))
            truths.append(truth)
    assert len(texts) > 250
    draws = parse_draws(run(segments_check, "record", "".join(texts)))
    assert len(draws) == len(texts)
    for draw, truth in zip(draws, truths):
        check_draw(draw, truth)


def test_record_restore_across_generations(segments_check):
    resv = [0, 3, 1, 0, 7]
    same = run(segments_check, "restore", "5 4 4 " + " ".join(map(str, resv)))
    changed = run(segments_check, "restore", "5 4 5 " + " ".join(map(str, resv)))
    assert [int(x) for x in same[0].split()] == resv
    assert [int(x) for x in changed[0].split()] == [0] * 5  # a reservation set loaded since: resv all zero
    rest = [int(x) for x in same[1].split()]
    assert rest == [v for p in range(5) for v in (10 + p, 500 + p, 1, 7 + p)]
    assert changed[1] == same[1]                             # everything else kept


def test_call_times(segments_check):
    total, batch_ms, pod_lat = run(segments_check, "times")
    assert float(total) == 3.875
    assert [float(x) for x in batch_ms.split()] == [0.5, 1.0, 2.0]
    assert [float(x) for x in pod_lat.split()] == [0.25, 0.5, 0.75, 4.0]
