"""Gang runs (include/koord_eval.h "gangs"): the reference and the inputs of test_gang_host.py and
test_gpu_gangs.py.

The reference follows pkg/scheduler/plugins/coscheduling/core/core.go in plain Python over the existing oracle, one pod
at a time: a member behind a failed member of its run is not tried (PreFilter, core.go:295-297); every other pod is
Oracle.schedule([pod]); a member placed nowhere before its run is satisfied fails the run (PostFilter,
core.go:304-341), and in strict mode every placed member is released with Oracle.release(..., RELEASE_UNRESERVE) from
its last_allocations record (rejectGangGroup -> Unreserve); a placed member raises the waiting count (Permit,
core.go:346-374).  With node sets / score tables the pod's step is the lock-step of test_node_scores_host.py (eval,
offset, masked argmax, Reserve by hand) and the release its inverse by hand.

Every input is made once per process and its reference once (reference()): the tests share them unchanged."""
import numpy as np

from koordinator_amd import abi, synth
from oracle.binding import Oracle
from preempt_ref import full_nodes, plain_pods
from test_node_scores_host import offsets_of
from test_node_sets_host import manual_reserve, masked_argmax

T0 = synth.T0
STRICT, NON_STRICT = abi.GANG_STRICT, abi.GANG_NON_STRICT
NONE, PLACED, WAITING, FAILED, SKIPPED, ROLLED_BACK = range(6)
S = synth.BASE_SEED + 77_000


def norm_runs(runs):
    """(first, count, min_member, assumed, mode) per run."""
    return [tuple(r) + (0,) * (5 - len(r)) for r in runs]


def machine(n, runs, place, undo):
    """The five rules over a queue of n pods: place(p) -> node or -1, undo(p, node).  Returns chosen, status, tried and
    the counts (runs, rolled-back runs, inverse Reserves)."""
    chosen, status, tried = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.full(n, -1, np.int32)
    run_of = {}
    for r in norm_runs(runs):
        for p in range(r[0], r[0] + r[1]):
            run_of[p] = r
    rolled = inverses = 0
    waiting, failed, satisfied = 0, False, False
    for p in range(n):
        r = run_of.get(p)
        if r is None:
            chosen[p] = place(p)
            continue
        first, count, min_member, assumed, mode = r
        need = max(min_member - assumed, 0)
        if p == first:
            waiting, failed, satisfied = 0, False, need == 0
        if failed:
            status[p] = SKIPPED
            continue
        chosen[p] = place(p)
        if chosen[p] < 0:
            status[p] = FAILED
            if satisfied:
                continue
            failed = True
            if mode == STRICT:
                rolled += 1
                for m in range(first, p):
                    if chosen[m] >= 0:
                        undo(m, int(chosen[m]))
                        tried[m], chosen[m], status[m] = chosen[m], -1, ROLLED_BACK
                        inverses += 1
            continue
        waiting += 1
        status[p] = PLACED if satisfied else WAITING
        if not satisfied and waiting >= need:
            satisfied = True
            for m in range(first, p + 1):
                if status[m] == WAITING:
                    status[m] = PLACED
    return chosen, status, tried, dict(runs=len(runs), rolled_back=rolled, inverse_reserves=inverses)


def run_reference(o, pods, runs, elig=None, off=None):
    """The queue on oracle `o` (which keeps the result's state).  `elig` bool [P, n] / `off` int64 [P, n]: the pods' node
    sets and score offsets (a plain profile; both None: Oracle.schedule places the pod).  Returns dict(chosen, score,
    status, tried, counts)."""
    P = len(pods)
    score = np.full(P, -1, np.int32)
    allocs = {}
    lock = elig is not None or off is not None

    def place(p):
        if not lock:
            c, s = o.schedule(pods[p:p + 1], T0)
            allocs[p] = o.last_allocations(1)[0].copy()
            score[p] = s[0]
            return int(c[0])
        t = o.eval(pods[p:p + 1], T0)["total"][0].astype(np.int64)
        if off is not None:
            t = np.where(t >= 0, t + off[p], -1)
        c, s = masked_argmax(t, np.ones(len(t), bool) if elig is None else elig[p])
        score[p] = s
        if c >= 0:
            manual_reserve(o, int(c), pods[p])
        return int(c)

    def undo(p, node):
        score[p] = -1
        if not lock:
            o.release(pods[p], allocs[p], abi.RELEASE_UNRESERVE)
            return
        o.unassign(node, int(pods[p]["uid"]))
        req = o.node_info_requested(node)[0]
        o.set_requested(node, int(req[0]) - int(pods[p]["requests"][abi.RES_CPU]),
                        int(req[1]) - int(pods[p]["requests"][abi.RES_MEMORY]))

    chosen, status, tried, counts = machine(P, runs, place, undo)
    return dict(chosen=chosen, score=score, status=status, tried=tried, counts=counts)


# ---- the cut rule of plan_batches, restated ----------------------------------------------------------------------------
def plan_cut(P, B, runs):
    """Batch sizes of P plain pods with `runs` at batch size B, and the batches the cut rule ended early."""
    start = {r[0]: r[1] for r in norm_runs(runs)}
    sizes, cuts, p = [], 0, 0
    while p < P:
        bp = 0
        while p + bp < P and bp < B:
            if bp > 0 and (p + bp) in start and bp + start[p + bp] > B:
                cuts += 1
                break
            bp += 1
        sizes.append(bp)
        p += bp
    return sizes, cuts


# ---- inputs ------------------------------------------------------------------------------------------------------------
NEARLY_FULL = dict(slack_cpu=(0, 1000, 3000, 9000), slack_mem=(0, 2, 6, 20))
MEDIUM = dict(slack_cpu=(0, 3000, 9000, 40000), slack_mem=(0, 6, 20, 128))
ROOMY = dict(slack_cpu=(20000, 40000, 64000), slack_mem=(64, 128, 256))
POISON_CPU = 10_000_000  # milli-CPU no node of the synthetic cluster has: NodeResourcesFit's Filter fails it everywhere


class Input:
    """One queue with its cluster: load(h) makes the same calls into an Evaluator or an Oracle; kw() are schedule()'s
    attachment keywords (the Evaluator's); elig / off the reference's view of them."""

    def __init__(self, name, n, P, B, runs, profile="fit", slack=ROOMY, capacity=None, seed=0):
        self.name, self.n, self.P, self.B, self.runs, self.profile = name, n, P, B, norm_runs(runs), profile
        seed = S + seed
        self.cl = synth.make_cluster(n, seed + 1)
        self.cl.nodes = full_nodes(self.cl, [[] for _ in range(n)], seed + 2, **slack)
        cap = capacity or n
        cfg = synth.config(cap, pod_batch=B)
        if profile in ("fit", "fitplus"):
            cfg = synth.fit_config(cfg, filter=True)
        if profile == "fitplus":
            cfg = synth.ext_config(cfg)
        self.cfg = cfg
        self.tables = synth.make_node_resources(self.cl, seed + 3) if profile != "plain" else None
        self.pods = plain_pods(P, seed + 4)
        self.pods["priority_class"][1::3] = abi.PRIORITY_NONE  # prod and non-prod pods: both halves of the LoadAware assign
        self.quota = None
        self.sets = self.sids = self.tabs = self.tids = None

    def poison(self, *positions):
        """The pods at `positions` fit nowhere (NodeResourcesFit's Filter: fit / fitplus profiles)."""
        assert self.profile != "plain"
        for p in positions:
            self.pods["requests"][p, abi.RES_CPU] = self.pods["limits"][p, abi.RES_CPU] = POISON_CPU

    def load(self, h):
        synth.load_into(h, self.cl)
        if self.tables is not None:
            synth.load_node_resources(h, self.tables)
        if self.quota is not None:
            h.quotas_load(*self.quota)

    def load_ev(self, ev):
        self.load(ev)
        if self.sets is not None:
            ev.node_sets_load(self.sets, self.n)
        if self.tabs is not None:
            ev.node_scores_load(self.tabs)

    def kw(self, a=0, b=None):
        kw = {}
        if self.sids is not None:
            kw["node_sets"] = self.sids[a:b]
        if self.tids is not None:
            kw["node_scores"] = self.tids[a:b]
        return kw

    def elig(self):
        return None if self.sets is None else np.concatenate([np.ones((1, self.n), bool), self.sets])[self.sids]

    def off(self):
        return None if self.tabs is None else offsets_of(self.tabs, self.tids, self.n)

    def oracle(self):
        o = Oracle(self.cfg, self.n)
        self.load(o)
        return o

    def run_words(self):
        """Per pod: the index of its run, or -1."""
        w = np.full(self.P, -1, np.int32)
        for i, r in enumerate(self.runs):
            w[r[0]:r[0] + r[1]] = i
        return w


def layout_runs(B, P):
    """Runs of 1, 2, B - 1 and B members and a last one of 2: at batch position 0; in mid-batch and fitting; where the
    cut rule must end the batch (twice); ending the call."""
    a = B + 2            # batch 1 starts at B: the run of B - 1 from its position 2 on does not fit
    b = a + (B - 1) + 1 + 3  # the batch the cut opened holds the run and one more pod; the run of B from position 3
    assert b + B <= P - 2
    return [(0, 1, 1), (3, 2, 2), (a, B - 1, B - 1), (b, B, B), (P - 2, 2, 2)]


# one node with room for a few pods; 63 and 65 roomy nodes (only the poisoned member fails); 64 nearly full ones (members
# fail early); 300 of mixed fill (long runs place many members, then fail)
LAYOUT_SLACK = {1: dict(slack_cpu=(64000,), slack_mem=(256,)), 63: ROOMY, 64: NEARLY_FULL, 65: ROOMY, 300: MEDIUM}


def _layout(n, B):
    P = 256 if B == 64 else 64
    runs = layout_runs(B, P)
    inp = Input(f"layout-{n}-{B}", n, P, B, runs, "fit", LAYOUT_SLACK[n], seed=1000 * B + n)
    inp.poison(runs[2][0] + runs[2][1] - 1)  # the run of B - 1 fails at its last member at the latest
    return inp


def _two_runs(order):
    inp = Input(f"two-runs-{order}", 65, 40, 64, [(2, 8, 4), (12, 8, 8)] if order == "sat-rb" else [(2, 8, 8), (12, 8, 4)],
                "fitplus", seed=11)
    inp.poison(12 + 6 if order == "sat-rb" else 2 + 6)
    return inp


def _same_node():
    """One roomy node: every placement lands on it.  Two plain pods change it first, then a strict run of four places
    three members there and fails: three inverse Reserves on one slot, the plain pods' Reserves stay; then plain pods."""
    inp = Input("same-node", 1, 12, 64, [(2, 4, 4)], "fit", dict(slack_cpu=(64000,), slack_mem=(256,)), seed=12)
    inp.pods["requests"][:, abi.RES_CPU] = inp.pods["limits"][:, abi.RES_CPU] = 2000
    inp.pods["requests"][:, abi.RES_MEMORY] = inp.pods["limits"][:, abi.RES_MEMORY] = 4 * synth.GI
    inp.poison(5)
    return inp


def _thresholds():
    """min_member below the run length with the failure behind the threshold; assumed > 0; need = 0; a non-strict run;
    a run that ends waiting; a run whose first member fails."""
    runs = [(0, 8, 4), (10, 6, 8, 5), (18, 4, 2, 2), (24, 6, 6, 0, NON_STRICT), (32, 4, 8), (38, 3, 3)]
    inp = Input("thresholds", 64, 44, 64, runs, "fit", seed=13)
    inp.poison(6, 10 + 4, 18, 24 + 3, 38)
    return inp


def _quota(B=64):
    """The plain profile (no NodeResourcesFit): members fail by ElasticQuota's PreFilter.  Leaf 2 (ke_pod.quota 2) holds
    three members' requests but not four: the run's fourth member is refused, the run rolled back; pod 6 of the same
    quota asks for more than was left beside the run and is admitted only because the rollback returned the used."""
    inp = Input(f"quota-{B}", 64, 16, B, [(1, 4, 4), (8, 4, 4)], "plain", seed=14 + B)
    q = np.zeros(3, abi.QUOTA_DTYPE)
    for i, (parent, cpu) in enumerate(((-1, 1_000_000), (0, 10_000), (0, 500_000))):
        q[i]["parent"], q[i]["has_max"], q[i]["max"] = parent, (1, 1), (cpu, 4000 * synth.GI)
        q[i]["has_min"], q[i]["min"], q[i]["shared_weight"] = (1, 1), (0, 0), q[i]["max"]
        q[i]["allow_lent_resource"] = 1
    inp.quota = (synth.quota_args(1_000_000, 4000 * synth.GI, runtime=False), q)
    inp.pods["requests"][:, abi.RES_CPU] = inp.pods["limits"][:, abi.RES_CPU] = 3000
    inp.pods["requests"][:, abi.RES_MEMORY] = inp.pods["limits"][:, abi.RES_MEMORY] = 4 * synth.GI
    inp.pods["quota"][:] = 3
    inp.pods["quota"][1:5] = 2   # the first run: 4 x 3000 > 10000
    inp.pods["quota"][6] = 2
    inp.pods["requests"][6, abi.RES_CPU] = inp.pods["limits"][6, abi.RES_CPU] = 8000  # 3 x 3000 + 8000 > 10000
    inp.pods["quota"][0] = 0
    return inp


def _sets_scores():
    """The plain profile with node sets and score tables on members and plain pods; set 3 is empty: a member of it is
    placed nowhere."""
    inp = Input("sets-scores", 65, 40, 64, [(3, 6, 6), (12, 8, 4), (24, 5, 5)], "plain", seed=15)
    rng = np.random.default_rng(S + 150)
    inp.sets = rng.random((3, 65)) < 0.5
    inp.sets[2] = False
    inp.sids = rng.integers(0, 3, 40).astype(np.int32)
    inp.sids[3 + 4] = 3      # the first run fails at its fifth member
    inp.sids[12 + 6] = 3     # the second behind its threshold
    inp.tabs = rng.integers(0, 200, (2, 65)).astype(np.uint16)
    inp.tids = rng.integers(0, 3, 40).astype(np.int32)
    return inp


def _capacity():
    inp = Input("capacity", 300, 64, 64, [(4, 16, 16), (30, 20, 10)], "fit", capacity=811_009, seed=16)
    inp.poison(4 + 12, 30 + 15)
    return inp


def _mixed():
    """Five plain batches, a rolled-back run in the sixth, five more plain batches."""
    inp = Input("mixed", 300, 64 * 11, 64, [(64 * 5 + 8, 12, 12)], "fit", seed=17)
    inp.poison(64 * 5 + 8 + 9)
    return inp


def _slices():
    """Two slices of 40 pods for two submits in flight, each with its own runs."""
    inp = Input("slices", 65, 80, 64, [(2, 8, 8), (20, 6, 3), (40 + 5, 10, 10), (40 + 30, 4, 8)], "fit", seed=18)
    inp.poison(2 + 5, 20 + 4, 45 + 7)
    return inp


BUILDERS = {f"layout-{n}-{B}": (lambda n=n, B=B: _layout(n, B)) for n in (1, 63, 64, 65, 300) for B in (7, 64)}
BUILDERS.update({"two-runs-sat-rb": lambda: _two_runs("sat-rb"), "two-runs-rb-sat": lambda: _two_runs("rb-sat"),
                 "same-node": _same_node, "thresholds": _thresholds, "quota-64": lambda: _quota(64),
                 "quota-7": lambda: _quota(7), "sets-scores": _sets_scores, "capacity": _capacity, "mixed": _mixed,
                 "slices": _slices})
_INPUTS, _REFS = {}, {}


def make_input(name):
    if name not in _INPUTS:
        _INPUTS[name] = BUILDERS[name]()
    return _INPUTS[name]


def reference(name):
    """(input, result, oracle after the queue) -- computed once; nobody changes them.  "slices": the two halves as two
    calls on one oracle, result = [first, second]."""
    if name not in _REFS:
        inp = make_input(name)
        o = inp.oracle()
        if name == "slices":
            e, f = inp.elig(), inp.off()
            res = []
            for a, b in ((0, 40), (40, 80)):
                runs = [(r[0] - a,) + r[1:] for r in inp.runs if a <= r[0] < b]
                res.append(run_reference(o, inp.pods[a:b], runs, e, f))
        else:
            res = run_reference(o, inp.pods, inp.runs, inp.elig(), inp.off())
        _REFS[name] = (inp, res, o)
    return _REFS[name]
