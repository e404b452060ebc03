"""Gang runs with DeviceShare members (ke_set_gang_devices, DESIGN.md §4w "DeviceShare members"): the inputs and the
reference of test_gang_devices_host.py and test_gpu_gang_devices.py.

The reference is gang_ref.machine -- core.go's run rules -- over the existing oracle one pod at a time: a pod's step is
Oracle.schedule([pod]) with its last_allocations record kept, a rolled-back member's Unreserve is
Oracle.release(pod, record, RELEASE_UNRESERVE), which returns its devices through the reference's updateCacheUsed(...,
false).  Besides placements, scores, statuses and tried nodes it answers the minors every pod holds at the end (0 for a
rolled-back member) and the log of the rollbacks.

Every input is made once per process and its reference once (reference()): the tests share them unchanged."""
import numpy as np

import gang_ref as G
from koordinator_amd import abi, synth
from oracle.binding import Oracle
from preempt_ref import full_nodes, plain_pods

T0 = synth.T0
S = synth.BASE_SEED + 88_000
GPU, SHARED, CORE, MEM, RATIO, RDMA = (abi.PDR[k] for k in (
    "nvidia.com/gpu", "koordinator.sh/gpu.shared", "koordinator.sh/gpu-core", "koordinator.sh/gpu-memory",
    "koordinator.sh/gpu-memory-ratio", "koordinator.sh/rdma"))
POISON_CPU = G.POISON_CPU


def devices(n, gpus=8, rdmas=2, used=None, have=None):
    """Per node `gpus` healthy GPUs and `rdmas` NICs; used(i, m) -> percent of GPU m of node i taken (0: no used keys);
    have(i) False: the node has no device cache entry."""
    out = []
    for i in range(n):
        if have is not None and not have(i):
            out.append(None)
            continue
        devs = np.zeros(gpus + rdmas, abi.DEVICE_DTYPE)
        for m in range(gpus):
            d = devs[m]
            d["type"], d["minor"], d["health"] = abi.DEV_GPU, m, 1
            d["has_total"][:] = 1
            d["total"][:] = [100, synth.GPU_MEM, 100]
            u = used(i, m) if used else 0
            if u:
                d["has_used"][:] = 1
                d["used"][:] = [u, synth.GPU_MEM * u // 100, u]
        for r in range(rdmas):
            d = devs[gpus + r]
            d["type"], d["minor"], d["health"] = abi.DEV_RDMA, r, 1
            d["has_total"][0], d["total"][0] = 1, 100
        out.append(devs)
    return out


class Input:
    """One queue with its cluster and devices: load(h) makes the same calls into an Evaluator or an Oracle."""

    def __init__(self, name, n, P, B, runs, devs, slack=G.ROOMY, strategy=abi.STRATEGY_LEAST_ALLOCATED, seed=0):
        self.name, self.n, self.P, self.B, self.runs = name, n, P, B, G.norm_runs(runs)
        seed = S + seed
        cfg = synth.fit_config(synth.config(n, pod_batch=B), filter=True)
        cfg.deviceshare.strategy = strategy
        self.cfg = cfg
        self.devs = devs
        for bump in range(200):  # a small cluster: the first seed at which every node takes a small plain pod
            self.cl = synth.make_cluster(n, seed + 1 + 7919 * bump)
            self.cl.nodes = full_nodes(self.cl, [[] for _ in range(n)], seed + 2 + 7919 * bump, **slack)
            self.tables = synth.make_node_resources(self.cl, seed + 3)
            if n > 8:
                break
            self.parts = None
            probe = plain_pods(1, seed + 5, cpu=(1,), mem=(1,))
            if (self.oracle().eval(probe, T0)["total"][0] >= 0).all():
                break
        else:
            raise AssertionError("no usable small cluster")
        self.parts = None  # per node (has_table, honor, partitions)
        self.pods = plain_pods(P, seed + 4, cpu=(1, 2), mem=(1, 2))
        self.pods["priority_class"][1::3] = abi.PRIORITY_NONE
        self.pods["gpu_ring_bus_bandwidth"] = abi.ABSENT

    def ask(self, positions, **req):
        """Device requests of the pods at `positions`: gpu= / shared= / core= / mem= / ratio= / rdma=."""
        keys = dict(gpu=GPU, shared=SHARED, core=CORE, mem=MEM, ratio=RATIO, rdma=RDMA)
        for p in positions:
            self.pods["device_requests"][p] = 0
            for k, v in req.items():
                self.pods["device_requests"][p, keys[k]] = v
            self.pods["has_other_requests"][p] = 1

    def poison(self, *positions):
        for p in positions:
            self.pods["requests"][p, abi.RES_CPU] = self.pods["limits"][p, abi.RES_CPU] = POISON_CPU

    def load(self, h):
        synth.load_into(h, self.cl)
        synth.load_node_resources(h, self.tables)
        synth.load_devices(h, self.devs)
        if self.parts is not None:
            synth.load_partition_states(h, self.parts)

    load_ev = load

    def kw(self, a=0, b=None):
        return {}

    def oracle(self):
        o = Oracle(self.cfg, self.n)
        self.load(o)
        return o

    def members(self):
        m = np.zeros(self.P, bool)
        for r in self.runs:
            m[r[0]:r[0] + r[1]] = True
        return m


def probe_pods():
    """One pod of each member kind, small in CPU and memory: their DeviceShare Filter and Score read every device."""
    pods = plain_pods(len(KINDS), S + 99, cpu=(1,), mem=(1,))
    pods["gpu_ring_bus_bandwidth"] = abi.ABSENT
    for p, req in enumerate(KINDS.values()):
        for k, v in req.items():
            pods["device_requests"][p, dict(gpu=GPU, shared=SHARED, core=CORE, mem=MEM, ratio=RATIO, rdma=RDMA)[k]] = v
        pods["has_other_requests"][p] = 1
    return pods


def run_reference(o, pods, runs):
    """The queue on oracle `o`.  dict(chosen, score, status, tried, counts, minors, rollbacks): minors [P] uint64 as held
    at the end; rollbacks: (member, node, minors) in the order they were undone."""
    P = len(pods)
    score, minors = np.full(P, -1, np.int32), np.zeros(P, np.uint64)
    allocs, rollbacks = {}, []

    def place(p):
        c, s = o.schedule(pods[p:p + 1], T0)
        allocs[p] = o.last_allocations(1)[0].copy()
        score[p] = s[0]
        minors[p] = allocs[p]["device_minors"] if c[0] >= 0 else 0
        return int(c[0])

    def undo(p, node):
        o.release(pods[p], allocs[p], abi.RELEASE_UNRESERVE)
        rollbacks.append((p, node, int(minors[p])))
        score[p], minors[p] = -1, 0

    chosen, status, tried, counts = G.machine(P, runs, place, undo)
    return dict(chosen=chosen, score=score, status=status, tried=tried, counts=counts, minors=minors, rollbacks=rollbacks)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _mix(inp, seed, fraction=0.4):
    """A share of the non-members ask for devices too: whole GPUs, shared slices in both memory forms, RDMA."""
    rng = np.random.default_rng(S + seed)
    mem = inp.members()
    for p in np.nonzero(~mem & (rng.random(inp.P) < fraction))[0]:
        k = rng.integers(4)
        if k == 0:
            inp.ask([p], gpu=int(rng.choice([1, 2])))
        elif k == 1:
            inp.ask([p], shared=1, core=int(rng.choice([25, 50])), ratio=int(rng.choice([25, 50])))
        elif k == 2:
            inp.ask([p], shared=1, core=25, mem=int(rng.choice([16, 48])) * synth.GI)
        else:
            inp.ask([p], gpu=1, rdma=50)


def _layout(n, B):
    """gang_ref's run layout -- runs of 1, 2, B - 1 and B members at batch position 0, in mid-batch, forcing the cut rule
    and ending the call -- with whole-GPU members; 8 GPUs on every node (n = 300: on two nodes in three), half of them
    partly used; the run of B - 1 fails at its last member at the latest."""
    P = 256 if B == 64 else 64
    runs = G.layout_runs(B, P)
    devs = devices(n, used=(lambda i, m: (0, 50, 0, 25)[(i + m) % 4]) if n > 1 else None,
                   have=(lambda i: i % 3 != 2) if n == 300 else None)
    inp = Input(f"layout-{n}-{B}", n, P, B, runs, devs, G.LAYOUT_SLACK[n] if n != 64 else G.MEDIUM, seed=1000 * B + n)
    inp.ask(np.nonzero(inp.members())[0], gpu=1)
    _mix(inp, 1000 * B + n)
    inp.poison(runs[2][0] + runs[2][1] - 1)
    return inp


KINDS = {"whole-1": dict(gpu=1), "whole-2": dict(gpu=2), "whole-8": dict(gpu=8),
         "shared-ratio": dict(shared=1, core=50, ratio=50), "shared-bytes": dict(shared=1, core=50, mem=96 * synth.GI),
         "gpu-rdma": dict(gpu=1, rdma=100)}


def _kind(kind):
    """Three nodes of 8 free GPUs and 2 NICs.  A strict run of members of one kind that holds most of the devices fails
    at its last member and is rolled back; the pods behind it ask for what only the freed devices can give."""
    req = KINDS[kind]
    per = {"whole-1": 8, "whole-2": 4, "whole-8": 1, "shared-ratio": 16, "shared-bytes": 16, "gpu-rdma": 2}[kind]
    k = 3 * per - 1  # members that place: all devices but one member's worth
    inp = Input(f"kind-{kind}", 3, 2 + k + 1 + 3 * per + 1, 64, [(2, k + 1, k + 1)], devices(3), seed=20 + list(KINDS).index(kind))
    inp.ask(range(2, 2 + k + 1), **req)
    inp.poison(2 + k)
    inp.ask(range(2 + k + 1, inp.P - 1), **req)  # 3 * per pods: they fit only if every member's devices came back
    return inp


def _same_node():
    """One node of two GPUs, MostAllocated.  Pod 0 (a non-member) takes half of a GPU (core 50 + ratio 50); a strict run of
    four places three members -- the first on the other half of pod 0's minor -- and fails at its fourth: three inverses
    on one node, pod 0's half stays; then shared pods that need the room."""
    inp = Input("same-node", 1, 12, 64, [(1, 4, 4)], devices(1, gpus=2, rdmas=0), dict(slack_cpu=(64000,), slack_mem=(256,)),
                strategy=abi.STRATEGY_MOST_ALLOCATED, seed=12)
    inp.ask(range(12), shared=1, core=50, ratio=50)
    inp.poison(4)
    return inp


def _zero_keys():
    """Two nodes; GPU 0 of node 0 has its used keys present with value 0 before the run (an entry a release left at
    zero was deleted upstream, but a cache built from a device CRD status can carry zeros).  A member takes that GPU and
    is rolled back: the host path -- and the device -- delete the entry, so the keys are absent afterwards."""
    devs = devices(2, gpus=2, rdmas=0)
    devs[0][0]["has_used"][:] = 1
    devs[0][0]["used"][:] = 0
    inp = Input("zero-keys", 2, 10, 64, [(0, 5, 5)], devs, seed=13)
    inp.ask(range(10), gpu=1)
    inp.poison(4)
    return inp


def _thresholds():
    """gang_ref's threshold queue with DeviceShare members: min_member below the run length with the failure behind the
    threshold; assumed > 0; need = 0; a non-strict run; a run that ends waiting; a run whose first member fails; a run rolled back at its last member."""
    runs = [(0, 8, 4), (10, 6, 8, 5), (18, 4, 2, 2), (24, 6, 6, 0, G.NON_STRICT), (32, 4, 8), (38, 3, 3), (42, 4, 4)]
    inp = Input("thresholds", 64, 48, 64, runs, devices(64, used=lambda i, m: (0, 25, 50)[(i * 3 + m) % 3]), seed=14)
    inp.ask(np.nonzero(inp.members())[0][::2], gpu=1)
    inp.ask(np.nonzero(inp.members())[0][1::2], shared=1, core=25, ratio=25)
    _mix(inp, 14)
    inp.poison(6, 10 + 4, 18, 24 + 3, 38, 42 + 3)
    return inp


def _partition_topology():
    """Nodes with a partition table, an honor policy or a GPU topology (ds_reserve on one lane) beside default nodes
    (ds_reserve_wave); members with and without a required topology scope."""
    n = 24
    devs = devices(n, used=lambda i, m: 50 if (i + m) % 5 == 0 else 0)
    synth.add_gpu_topology(devs[:12], S + 15)
    inp = Input("partition-topology", n, 48, 64, [(2, 12, 12), (20, 10, 5), (34, 12, 12)], devs, seed=15)
    inp.parts = synth.make_partition_states(12, S + 16) + [(False, False, None)] * (n - 12)
    mem = np.nonzero(inp.members())[0]
    inp.ask(mem[::3], gpu=2)
    inp.ask(mem[1::3], gpu=1)
    inp.ask(mem[2::3], shared=1, core=50, ratio=50)
    inp.pods["gpu_required_topology_scope"][mem[::3]] = abi.SCOPE_NUMA
    _mix(inp, 15)
    inp.poison(2 + 10, 20 + 8, 34 + 11)
    return inp


def _cut_in_run(B=64):
    """MostAllocated DeviceShare scores on nodes of equal, partly used GPUs: every whole-GPU Reserve lifts its node above
    the snapshot's normalisation max, so the batch is cut behind nearly every pod.  The run of ten places
    seven members over several launches and fails at its eighth: the rollback reaches members earlier launches placed.
    Behind the run: pods that need the freed GPUs."""
    n = 6
    inp = Input(f"cut-in-run-{B}", n, 30, B, [(3, 10, 10)] if B == 64 else [(0, 7, 7), (8, 6, 6)],
                devices(n, gpus=4, rdmas=0, used=lambda i, m: 50 if m == 0 else 0), strategy=abi.STRATEGY_MOST_ALLOCATED,
                seed=17)
    inp.ask(range(30), gpu=1)
    inp.ask(range(20, 30, 3), shared=1, core=50, ratio=50)
    if B == 64:
        inp.poison(3 + 7)
    else:
        inp.poison(5, 8 + 4)
    return inp


def _short_list(n, L, cpu, seed):
    """_cut_in_run's devices with plain pods behind a run that fails at its last member, and node scores that rise with a
    node's load (NodeNUMAResource MostAllocated at weight 3): in the snapshot of the launch that begins at the failing
    member, the plain pod's best candidates are the nodes the run filled; the rollback adopts them and they fall behind
    an unchanged node.  Only a list longer than j + 1 entries still holds that node ("List length")."""
    first, tail = 3, 3
    P = first + L + tail + 4
    inp = Input(f"short-list-{n}-{L}", n, P, 64, [(first, L, L)], devices(n, gpus=4, rdmas=0, used=lambda i, m: 50 if m == 0 else 0),
                strategy=abi.STRATEGY_MOST_ALLOCATED, seed=seed)
    inp.cfg.numa.strategy = abi.STRATEGY_MOST_ALLOCATED
    inp.cfg.weight_numa = 3
    mem = list(range(first, first + L))
    inp.ask(list(range(first)) + mem, gpu=1)
    inp.ask(range(first + L + tail, P), gpu=1)
    inp.pods["requests"][mem, abi.RES_CPU] = inp.pods["limits"][mem, abi.RES_CPU] = cpu
    inp.poison(first + L - 1)
    return inp


def _mixed():
    """Five plain batches, a DeviceShare batch with a rolled-back run of GPU members, five more plain batches."""
    inp = Input("mixed", 300, 64 * 11, 64, [(64 * 5 + 8, 12, 12)], devices(300, used=lambda i, m: (0, 50)[(i + m) % 2]),
                seed=18)
    inp.ask(range(64 * 5 + 8, 64 * 5 + 20), gpu=1)
    inp.ask(range(64 * 5 + 30, 64 * 5 + 40), shared=1, core=50, ratio=50)
    inp.poison(64 * 5 + 8 + 9)
    return inp


def _slices():
    """Two slices of 40 pods for two submits in flight, each with its own runs of GPU members."""
    inp = Input("slices", 65, 80, 64, [(2, 8, 8), (20, 6, 3), (40 + 5, 10, 10), (40 + 30, 4, 8)],
                devices(65, used=lambda i, m: (0, 25)[(i + m) % 2]), seed=19)
    inp.ask(np.nonzero(inp.members())[0], gpu=1)
    _mix(inp, 19)
    inp.poison(2 + 5, 20 + 4, 45 + 7)
    return inp


BUILDERS = {f"layout-{n}-{B}": (lambda n=n, B=B: _layout(n, B)) for n in (1, 63, 64, 65, 300) for B in (7, 64)}
BUILDERS.update({f"kind-{k}": (lambda k=k: _kind(k)) for k in KINDS})
BUILDERS.update({"same-node": _same_node, "zero-keys": _zero_keys, "thresholds": _thresholds,
                 "partition-topology": _partition_topology, "cut-in-run-64": lambda: _cut_in_run(64),
                 "cut-in-run-7": lambda: _cut_in_run(7), "mixed": _mixed, "slices": _slices,
                 "short-list-16-7": lambda: _short_list(16, 7, 10000, 44),
                 "short-list-16-8": lambda: _short_list(16, 8, 10000, 44)})
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
            res = []
            for a, b in ((0, 40), (40, 80)):
                res.append(run_reference(o, inp.pods[a:b], [(r[0] - a,) + r[1:] for r in inp.runs if a <= r[0] < b]))
        else:
            res = run_reference(o, inp.pods, inp.runs)
        _REFS[name] = (inp, res, o)
    return _REFS[name]


def device_used(h, n):
    """Per node the device cache entry's (type, minor, has_used, used) rows, from node_state of an Evaluator or Oracle."""
    out = []
    for i in range(n):
        d = h.node_state(i)[3]
        out.append([(int(x["type"]), int(x["minor"]), x["has_used"].tolist(), x["used"].tolist()) for x in d])
    return out
