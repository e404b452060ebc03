"""Python handle over the C ABI (libkoordeval.so): the same calls a Go koord-scheduler makes via cgo.

`Evaluator` owns one ke_ctx (one GPU, one node shard).  State ingestion mirrors the informer events
the reference plugins consume; `eval` is the parity-mode Filter/Score matrix and `schedule` the
queue scheduler (findNodesThatFitPod + score + selectHost + Reserve per pod, exact speculative
batching on the device).  There is no CPU fallback: evaluation without the HIP device raises.
"""
import ctypes as C

import numpy as np

from . import abi


class KoordEvalError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"koord-eval error {code}: {msg}")
        self.code = code


def pack_node_sets(sets, n_nodes=None):
    """Node sets -> (n_sets, words_per_set, uint64 words) for ke_node_sets_load: `sets` is a bool [n_sets, N] matrix
    or a list of node index arrays (then N = n_nodes, default 1 + the highest index).  Bit i & 63 of word i >> 6 of a
    set's row = node i; the tail bits of the last word are zero."""
    if isinstance(sets, np.ndarray) and sets.ndim == 2:
        m = np.ascontiguousarray(sets, dtype=bool)
    else:
        idx = [np.asarray(x, np.int64).reshape(-1) for x in sets]
        if n_nodes is None:
            n_nodes = max([int(x.max()) + 1 for x in idx if len(x)], default=0)
        m = np.zeros((len(idx), n_nodes), bool)
        for r, x in enumerate(idx):
            if len(x) and (x.min() < 0 or x.max() >= n_nodes):
                raise ValueError("node index outside 0..n_nodes")
            m[r, x] = True
    n_sets, n = m.shape
    wps = (n + 63) // 64
    padded = np.zeros((n_sets, wps * 64), np.uint8)
    padded[:, :n] = m
    words = np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(n_sets, wps)
    return n_sets, wps, np.ascontiguousarray(words, np.uint64)


def unpack_node_sets(words, n_nodes):
    """The bool [n_sets, n_nodes] matrix of pack_node_sets' words."""
    w = np.ascontiguousarray(words, "<u8")
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")
    return bits[:, :n_nodes].astype(bool)


def reason_message(code, lib=None):
    """ke_reason_message: the plugin's message of a KE_REASON_* code ("" for an unknown one)."""
    return (lib or abi.load_library()).ke_reason_message(int(code)).decode()


def reason_plugin(code, lib=None):
    """ke_reason_plugin: the abi.PLUGIN_* bit of a KE_REASON_* code (0 for NONE / an unknown one)."""
    return int((lib or abi.load_library()).ke_reason_plugin(int(code)))


def as_pod_array(pods):
    """list[abi.Pod] | np.ndarray(POD_DTYPE) -> contiguous np.ndarray(POD_DTYPE)."""
    if isinstance(pods, np.ndarray):
        assert pods.dtype == abi.POD_DTYPE
        return np.ascontiguousarray(pods)
    arr = np.zeros(len(pods), dtype=abi.POD_DTYPE)
    if len(pods):
        buf = (abi.Pod * len(pods))(*pods)
        arr[:] = np.frombuffer(buf, dtype=abi.POD_DTYPE, count=len(pods))
    return arr


class Evaluator:
    def __init__(self, cfg, lib=None):
        self.lib = lib or abi.load_library()
        self.cfg = cfg
        h = C.c_void_p()
        self._check(self.lib.ke_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self._last_n, self._last_out = 0, {}
        self._inflight = {}  # ticket -> the submitted pod array (ke_schedule_submit reads it until the wait)

    # ---- plumbing --------------------------------------------------------------------------
    def _check(self, rc):
        if rc != abi.OK:
            raise KoordEvalError(rc, self.lib.ke_last_error().decode())
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.lib.ke_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def device(self):
        return bool(self.lib.ke_device_available())

    @property
    def num_nodes(self):
        return self.lib.ke_num_nodes(self.h)

    # ---- state ingestion --------------------------------------------------------------------
    def upsert_node(self, i, node):
        self._check(self.lib.ke_node_upsert(self.h, i, C.byref(node)))

    def nodes_load(self, nodes):
        nodes = np.ascontiguousarray(nodes, dtype=abi.NODE_DTYPE)
        self._check(self.lib.ke_nodes_load(self.h, len(nodes), abi.ptr(nodes)))

    def set_requested(self, i, milli_cpu, memory):
        self._check(self.lib.ke_node_set_requested(self.h, i, milli_cpu, memory))

    def set_cpuset_allocated(self, i, cpus):
        self._check(self.lib.ke_node_set_cpuset_allocated(self.h, i, cpus))

    def set_nodemetric(self, i, nm):
        """nm = model.make_node_metric(...) tuple."""
        hdr, pms, n_pm, aggs, n_agg = nm
        self._check(self.lib.ke_nodemetric_upsert(self.h, i, C.byref(hdr), n_pm, C.cast(pms, C.c_void_p), n_agg,
                                                   C.cast(aggs, C.c_void_p)))

    def nodemetrics_load(self, headers, pm_offsets, pod_metrics, agg_offsets, aggregated):
        headers = np.ascontiguousarray(headers, dtype=abi.NODE_METRIC_DTYPE)
        pm_offsets = np.ascontiguousarray(pm_offsets, dtype=np.int64)
        agg_offsets = np.ascontiguousarray(agg_offsets, dtype=np.int64)
        pod_metrics = np.ascontiguousarray(pod_metrics, dtype=abi.POD_METRIC_DTYPE)
        aggregated = np.ascontiguousarray(aggregated, dtype=abi.AGG_DTYPE)
        self._check(self.lib.ke_nodemetrics_load(self.h, len(headers), abi.ptr(headers), abi.ptr(pm_offsets),
                                                 abi.ptr(pod_metrics), abi.ptr(agg_offsets), abi.ptr(aggregated)))

    def delete_nodemetric(self, i):
        self._check(self.lib.ke_nodemetric_delete(self.h, i))

    def delete_node(self, i):
        """Node informer delete (ke_node_delete): out of the snapshot, other caches kept."""
        self._check(self.lib.ke_node_delete(self.h, i))

    def delete_topology(self, i):
        """NodeResourceTopology delete (ke_node_topology_delete)."""
        self._check(self.lib.ke_node_topology_delete(self.h, i))

    def assign(self, i, pod, timestamp_ns):
        self._check(self.lib.ke_pod_assign(self.h, i, C.byref(pod), int(timestamp_ns)))

    def assign_bulk(self, nodes, pods, timestamps_ns):
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        pods = as_pod_array(pods)
        ts = np.ascontiguousarray(timestamps_ns, dtype=np.int64)
        self._check(self.lib.ke_pods_assign(self.h, len(nodes), abi.ptr(nodes), abi.ptr(pods), abi.ptr(ts)))

    def unassign(self, i, uid):
        self._check(self.lib.ke_pod_unassign(self.h, i, uid))

    def set_devices(self, i, devices):
        """DeviceShare node device cache entry (model.make_devices(...))."""
        devices = np.ascontiguousarray(devices, dtype=abi.DEVICE_DTYPE)
        self._check(self.lib.ke_node_devices_set(self.h, i, len(devices), abi.ptr(devices)))

    def delete_devices(self, i):
        self._check(self.lib.ke_node_devices_delete(self.h, i))

    def set_pod_device_hints(self, hints):
        """ke_set_pod_device_hints: the DeviceAllocateHints / DeviceJointAllocate table (POD_DEVICE_HINTS_DTYPE)
        ke_pod.device_hint indexes (1 + index)."""
        h = abi.struct_array(hints, abi.PodDeviceHints)
        self._check(self.lib.ke_set_pod_device_hints(self.h, len(h), abi.ptr(h)))

    def gpu_templates_load(self, templates):
        """ke_gpu_templates_load: GPU shared resource templates (GPU_TEMPLATE_DTYPE)."""
        t = abi.struct_array(templates, abi.GpuTemplate)
        self._check(self.lib.ke_gpu_templates_load(self.h, len(t), abi.ptr(t)))

    def reservations_load(self, reservations, allocs=None, resources=None):
        """ke_reservations_load(_ex / _full): the reservation cache (RESERVATION_DTYPE array), optionally each one's
        NUMA / cpuset / device holdings (RESERVATION_ALLOC_DTYPE array, one per reservation) and its allocatable
        names beyond cpu / memory (`resources`: per reservation a RESERVATION_RESOURCE_DTYPE array or list)."""
        r = abi.struct_array(reservations, abi.Reservation)
        a = None
        if allocs is not None:
            a = abi.struct_array(allocs, abi.ReservationAlloc)
            assert len(a) == len(r)
        if resources is not None:
            off, res = abi.resource_csr(resources, len(r))
            self._check(self.lib.ke_reservations_load_full(self.h, len(r), abi.ptr(r), abi.ptr(a) if a is not None else None,
                                                           abi.ptr(off), abi.ptr(res)))
        elif a is None:
            self._check(self.lib.ke_reservations_load(self.h, len(r), abi.ptr(r)))
        else:
            self._check(self.lib.ke_reservations_load_ex(self.h, len(r), abi.ptr(r), abi.ptr(a)))
        self._n_resv = len(r)

    def reservation_resources_get(self, i):
        """ke_reservation_resources_get: reservation i's entries beyond cpu / memory as Reserve / release left them."""
        out = np.zeros(abi.MAX_XRES + 1, abi.RESERVATION_RESOURCE_DTYPE)
        n = C.c_int32()
        self._check(self.lib.ke_reservation_resources_get(self.h, int(i), len(out), abi.ptr(out), C.byref(n)))
        return out[:n.value]

    def reservation_allocs_get(self):
        """ke_reservation_allocs_get: the holdings with the owner parts as Reserve / release left them."""
        out = np.zeros(getattr(self, "_n_resv", 0), abi.RESERVATION_ALLOC_DTYPE)
        self._check(self.lib.ke_reservation_allocs_get(self.h, len(out), abi.ptr(out)))
        return out

    def reservations_get(self):
        """ke_reservations_get: the reservation cache as Reserve / Unreserve left it."""
        out = np.zeros(getattr(self, "_n_resv", 0), abi.RESERVATION_DTYPE)
        self._check(self.lib.ke_reservations_get(self.h, len(out), abi.ptr(out)))
        return out

    def pod_reservations(self, matches):
        """ke_pod_reservations: per pod of the next schedule() the reservation indices it matches."""
        off = np.zeros(len(matches) + 1, np.int32)
        off[1:] = np.cumsum([len(m) for m in matches])
        ids = np.ascontiguousarray(np.concatenate([np.asarray(m, np.int32) for m in matches]) if len(matches)
                                   else np.zeros(0, np.int32), np.int32)
        self._check(self.lib.ke_pod_reservations(self.h, len(matches), abi.ptr(off), abi.ptr(ids)))

    def node_sets_load(self, sets, n_nodes=None):
        """ke_node_sets_load: replace the node eligibility sets (pack_node_sets' inputs); set ids are 1 + the row.
        An empty list drops the table."""
        n_sets, wps, words = pack_node_sets(sets, n_nodes)
        self._check(self.lib.ke_node_sets_load(self.h, n_sets, wps, abi.ptr(words) if n_sets else None))

    def node_set_bits(self, node, member):
        """ke_node_set_bits: node `node`'s membership in every loaded set (member[s - 1] for set id s)."""
        m = np.ascontiguousarray(np.asarray(member).astype(bool), np.uint8)
        self._check(self.lib.ke_node_set_bits(self.h, int(node), len(m), abi.ptr(m)))

    def pod_node_sets(self, set_ids):
        """ke_pod_node_sets: the set id (0 = every node) per pod of the next eval / schedule / submit."""
        ids = np.ascontiguousarray(set_ids, np.int32)
        self._check(self.lib.ke_pod_node_sets(self.h, len(ids), abi.ptr(ids)))

    def node_scores_load(self, tables, n_nodes=None):
        """ke_node_scores_load: replace the node score offset tables -- `tables` a [n_tables, N] matrix (or a list of
        rows) of uint16 values, zero-padded to n_nodes when that is larger; table ids are 1 + the row.  An empty
        list drops the table."""
        t = np.asarray(tables)
        if t.size == 0:
            self._check(self.lib.ke_node_scores_load(self.h, 0, 0, None))
            return
        t = np.atleast_2d(t)
        if (t < 0).any() or (t > 0xFFFF).any():
            raise ValueError("node score outside 0..65535")
        n = t.shape[1] if n_nodes is None else int(n_nodes)
        if n < t.shape[1]:
            raise ValueError("n_nodes below the tables' width")
        v = np.zeros((t.shape[0], n), np.uint16)
        v[:, :t.shape[1]] = t
        self._check(self.lib.ke_node_scores_load(self.h, v.shape[0], n, abi.ptr(v)))

    def node_scores_set(self, node, column):
        """ke_node_scores_set: node `node`'s entry in every loaded table (column[t - 1] for table id t)."""
        c = np.asarray(column).reshape(-1)
        if (c < 0).any() or (c > 0xFFFF).any():
            raise ValueError("node score outside 0..65535")
        c = np.ascontiguousarray(c, np.uint16)
        self._check(self.lib.ke_node_scores_set(self.h, int(node), len(c), abi.ptr(c) if len(c) else None))

    def pod_node_scores(self, table_ids):
        """ke_pod_node_scores: the score table id (0 = no offset) per pod of the next eval / schedule / submit."""
        ids = np.ascontiguousarray(table_ids, np.int32)
        self._check(self.lib.ke_pod_node_scores(self.h, len(ids), abi.ptr(ids)))

    def spread_groups_load(self, counts, max_per_node, n_nodes=None):
        """ke_spread_groups_load: replace the spread groups -- `max_per_node` the cap (>= 1) per group, `counts` a
        [n_groups, N] matrix of the pods each group already has per node (None: all zero), zero-padded to n_nodes
        when that is larger; group ids are 1 + the row.  No caps drop the table."""
        caps = np.asarray(max_per_node).reshape(-1)
        if caps.size == 0:
            self._check(self.lib.ke_spread_groups_load(self.h, 0, 0, None, None))
            return
        if (caps < 0).any() or (caps > 0xFFFF).any():
            raise ValueError("spread group cap outside 0..65535")
        caps = np.ascontiguousarray(caps, np.uint16)
        if counts is None:
            n = self.num_nodes if n_nodes is None else int(n_nodes)
            self._check(self.lib.ke_spread_groups_load(self.h, len(caps), n, None, abi.ptr(caps)))
            return
        c = np.atleast_2d(np.asarray(counts))
        if c.shape[0] != len(caps):
            raise ValueError("one row of counts per cap")
        if (c < 0).any() or (c > 0xFFFF).any():
            raise ValueError("spread group count outside 0..65535")
        n = c.shape[1] if n_nodes is None else int(n_nodes)
        if n < c.shape[1]:
            raise ValueError("n_nodes below the counts' width")
        v = np.zeros((c.shape[0], n), np.uint16)
        v[:, :c.shape[1]] = c
        self._check(self.lib.ke_spread_groups_load(self.h, len(caps), n, abi.ptr(v), abi.ptr(caps)))

    def spread_group_add(self, group, node, delta):
        """ke_spread_group_add: count[group][node] += delta (an informer pod event, or -1 to undo a placement)."""
        self._check(self.lib.ke_spread_group_add(self.h, int(group), int(node), int(delta)))

    def spread_groups_get(self, group, n_nodes):
        """ke_spread_groups_get: group `group`'s current count per node, every Reserve included."""
        out = np.zeros(int(n_nodes), np.uint16)
        self._check(self.lib.ke_spread_groups_get(self.h, int(group), len(out), abi.ptr(out) if len(out) else None))
        return out

    def pod_spread_groups(self, ids):
        """ke_pod_spread_groups: the spread group id (0 = none) per pod of the next eval / diagnose / schedule / submit."""
        ids = np.ascontiguousarray(ids, np.int32)
        self._check(self.lib.ke_pod_spread_groups(self.h, len(ids), abi.ptr(ids)))

    def debug_spread_groups_check(self):
        """ke_debug_spread_groups_check: entries of the device's spread group table that differ from the host copy."""
        n = C.c_int64()
        self._check(self.lib.ke_debug_spread_groups_check(self.h, C.byref(n)))
        return n.value

    def spread_domains_load(self, node_domain, group_map, domains, max_skew, min_domains=None, counts=None, n_nodes=None):
        """ke_spread_domains_load: replace the spread domains -- `node_domain` a [n_maps, N] matrix of domain ids
        (0..63, abi.DOMAIN_NONE for a node without the topology key; padded with DOMAIN_NONE to n_nodes when that is
        larger); per group its map (1 + the row of node_domain), the uint64 bitmask `domains`, `max_skew` (>= 1),
        `min_domains` (None: 0) and `counts`, a [n_groups, 64] matrix of the pods it already has per domain (None:
        zero).  Group ids are 1 + the index.  No groups drop the table."""
        gm = np.ascontiguousarray(np.asarray(group_map).reshape(-1), np.int32)
        G = len(gm)
        if G == 0:
            self._check(self.lib.ke_spread_domains_load(self.h, 0, 0, None, 0, None, None, None, None, None))
            return
        m = np.atleast_2d(np.asarray(node_domain))
        if (m < 0).any() or (m > 0xFFFF).any():
            raise ValueError("domain id outside 0..65535")
        n = m.shape[1] if n_nodes is None else int(n_nodes)
        if n < m.shape[1]:
            raise ValueError("n_nodes below the maps' width")
        v = np.full((m.shape[0], n), abi.DOMAIN_NONE, np.uint16)
        v[:, :m.shape[1]] = m
        dom = np.ascontiguousarray([int(d) for d in np.asarray(domains, object).reshape(-1)], np.uint64)
        skew = np.ascontiguousarray(np.asarray(max_skew).reshape(-1), np.int32)
        mind = None if min_domains is None else np.ascontiguousarray(np.asarray(min_domains).reshape(-1), np.int32)
        if len(dom) != G or len(skew) != G or (mind is not None and len(mind) != G):
            raise ValueError("one map, domains mask, max_skew (and min_domains) per group")
        cnt = None
        if counts is not None:
            c = np.atleast_2d(np.asarray(counts))
            if c.shape != (G, abi.MAX_SPREAD_DOMAINS):
                raise ValueError("counts is [n_groups, 64]")
            if (c < 0).any() or (c > 0xFFFFFFFF).any():
                raise ValueError("spread domain count outside 0..2^32-1")
            cnt = np.ascontiguousarray(c, np.uint32)
        self._check(self.lib.ke_spread_domains_load(
            self.h, v.shape[0], n, abi.ptr(v) if v.size else None, G, abi.ptr(gm), abi.ptr(dom), abi.ptr(skew),
            None if mind is None else abi.ptr(mind), None if cnt is None else abi.ptr(cnt)))

    def spread_domain_add(self, group, domain, delta):
        """ke_spread_domain_add: count[group][domain] += delta (an informer pod event, or -1 to undo a placement)."""
        self._check(self.lib.ke_spread_domain_add(self.h, int(group), int(domain), int(delta)))

    def spread_domain_node_set(self, map_id, node, domain):
        """ke_spread_domain_node_set: the domain of `node` in map `map_id` (a node the informer adds or relabels)."""
        self._check(self.lib.ke_spread_domain_node_set(self.h, int(map_id), int(node), int(domain)))

    def spread_domains_get(self, group):
        """ke_spread_domains_get: group `group`'s current count per domain [64], every Reserve included."""
        out = np.zeros(abi.MAX_SPREAD_DOMAINS, np.uint32)
        self._check(self.lib.ke_spread_domains_get(self.h, int(group), abi.ptr(out)))
        return out

    def pod_spread_domains(self, ids):
        """ke_pod_spread_domains: the spread domain group id (0 = none) per pod of the next eval / diagnose / schedule /
        submit."""
        ids = np.ascontiguousarray(ids, np.int32)
        self._check(self.lib.ke_pod_spread_domains(self.h, len(ids), abi.ptr(ids)))

    def pod_spread_terms(self, terms, members):
        """ke_pod_spread_terms: per pod of the next eval / diagnose / schedule / submit a list of terms -- (group,
        kind, param) for abi.TERM_ANTI / TERM_AFFINITY, (group, kind, param, weight) for TERM_PREFER_FEWER /
        TERM_PREFER_MORE -- and a list of member groups, over the spread groups' counts; both lists of a plain pod are
        empty.  Packed here into the entry point's four CSR arrays."""
        self._check(self.lib.ke_pod_spread_terms(
            *self._term_lists(terms, members, (3, 4), "a term is (group, kind, param[, weight])")))

    def pod_spread_domain_terms(self, terms, members):
        """ke_pod_spread_domain_terms: pod_spread_terms' lists over the spread domain groups' counts -- zone-level
        affinity, anti-affinity and soft spread; besides its four kinds (group, abi.TERM_SKEW) is the group's maxSkew
        filter.  A placement increments every member's count of the node's domain in the member's map."""
        self._check(self.lib.ke_pod_spread_domain_terms(
            *self._term_lists(terms, members, (2, 3, 4), "a term is (group, kind[, param[, weight]])")))

    def _term_lists(self, terms, members, lengths, what):
        """The arguments of ke_pod_spread_terms / ke_pod_spread_domain_terms: per-pod lists packed into CSR arrays; a
        term of a length outside `lengths` is a ValueError (`what`)."""
        if len(terms) != len(members):
            raise ValueError("one term list and one member list per pod")
        t_off = np.zeros(len(terms) + 1, np.int32)
        m_off = np.zeros(len(members) + 1, np.int32)
        t_flat, m_flat = [], []
        for p, (tl, ml) in enumerate(zip(terms, members)):
            for t in tl:
                t = tuple(int(v) for v in t)
                if len(t) not in lengths:
                    raise ValueError(what)
                t_flat.append(t + (0,) * (4 - len(t)))
            m_flat.extend(int(m) for m in ml)
            t_off[p + 1], m_off[p + 1] = len(t_flat), len(m_flat)
        t_arr = np.ascontiguousarray(np.asarray(t_flat, np.int32).reshape(-1, 4))
        m_arr = np.ascontiguousarray(m_flat, np.int32)
        self._lists = (t_off, t_arr, m_off, m_arr)  # (alive through the call)
        return (self.h, len(terms), abi.ptr(t_off), abi.ptr(t_arr) if len(t_arr) else None, abi.ptr(m_off),
                abi.ptr(m_arr) if len(m_arr) else None)

    def debug_spread_domains_check(self):
        """ke_debug_spread_domains_check: counts and map entries of the device's spread domain tables that differ from
        the host copy."""
        n = C.c_int64()
        self._check(self.lib.ke_debug_spread_domains_check(self.h, C.byref(n)))
        return n.value

    def node_info_requested(self, i):
        """ke_node_info_requested: NodeInfo Requested / NonZeroRequested (MilliCPU, Memory) after the restore."""
        req, nz = (C.c_int64 * 2)(), (C.c_int64 * 2)()
        self._check(self.lib.ke_node_info_requested(self.h, i, req, nz))
        return list(req), list(nz)

    def set_device_flags(self, i, secondary_well_planned, gpu_model_key):
        """ke_node_device_flags: the Device's secondary-well-planned label and the node's GPU template key."""
        self._check(self.lib.ke_node_device_flags(self.h, i, int(secondary_well_planned), int(gpu_model_key)))

    def set_gpu_partitions(self, i, has_table, honor, partitions=None):
        """The node's GPU partition indexer + policy (model.gpu_partition_state(...))."""
        parts = np.ascontiguousarray(partitions if partitions is not None else np.zeros(0, abi.GPU_PARTITION_DTYPE),
                                     dtype=abi.GPU_PARTITION_DTYPE)
        self._check(self.lib.ke_node_gpu_partitions(self.h, i, int(bool(has_table)), int(bool(honor)), len(parts),
                                                    abi.ptr(parts)))

    def set_numa(self, i, zones):
        """NodeResourceTopology NUMA zones + their allocation (model.make_zones(...))."""
        zones = np.ascontiguousarray(zones, dtype=abi.NUMA_ZONE_DTYPE)
        self._check(self.lib.ke_node_numa_set(self.h, i, len(zones), abi.ptr(zones)))

    def set_resources(self, i, resources):
        """NodeResourcesFitPlus / ScarceResourceAvoidance table of node i (np.ndarray NODE_RESOURCE_DTYPE)."""
        res = np.ascontiguousarray(resources, dtype=abi.NODE_RESOURCE_DTYPE)
        self._check(self.lib.ke_node_resources_set(self.h, i, len(res), abi.ptr(res)))

    def get_resources(self, i):
        out = np.zeros(abi.MAX_XRES, abi.NODE_RESOURCE_DTYPE)
        n = abi.i32()
        self._check(self.lib.ke_node_resources_get(self.h, i, abi.MAX_XRES, abi.ptr(out), C.byref(n)))
        return out[:n.value]

    def set_cpus(self, i, cpus, max_ref_count=1):
        """CPU topology + cpuset allocation state (model.make_cpus(...)); an empty table clears it."""
        cpus = np.ascontiguousarray(cpus, dtype=abi.CPU_DTYPE)
        self._check(self.lib.ke_node_cpus_set(self.h, i, len(cpus), abi.ptr(cpus), max_ref_count))

    def estimate_pod(self, pod):
        est = np.zeros(2, np.int64)
        self._check(self.lib.ke_estimate_pod(self.h, C.byref(pod), abi.ptr(est)))
        return est

    # ---- node sharding (one process per GPU) ------------------------------------------------
    def shard_init(self, rank, world, unique_id=None):
        """Collective over `world` ranks with the same RCCL `unique_id` (bytes from comm_unique_id on
        rank 0); unique_id=None with world > 1 runs every shard in this context (loopback)."""
        buf = None
        if unique_id is not None:
            assert len(unique_id) == abi.COMM_ID_BYTES
            buf = C.create_string_buffer(bytes(unique_id), abi.COMM_ID_BYTES)
        self._check(self.lib.ke_shard_init(self.h, rank, world, buf))

    def shard_init_host(self, rank, world, collective):
        """ke_shard_init_host: the sharded path with its collectives carried on the host by
        collective(op, dtype, send: np.ndarray, world) -> np.ndarray (all-gather: world * len(send) elements
        rank-major; max / min: len(send) elements), e.g. koordinator_amd.shard.gloo_collective()."""
        dts = {abi.COLL_U32: np.uint32, abi.COLL_I32: np.int32, abi.COLL_I64: np.int64, abi.COLL_U64: np.uint64}

        def cb(user, op, dtype, send, recv, count):
            try:
                dt = np.dtype(dts[dtype])
                n = int(count)
                src = np.frombuffer((C.c_uint8 * (n * dt.itemsize)).from_address(send), dtype=dt).copy()
                out = np.ascontiguousarray(collective(int(op), dt, src, world), dtype=dt)
                m = n * (world if op == abi.COLL_ALL_GATHER else 1)
                assert out.size == m
                C.memmove(recv, out.ctypes.data, m * dt.itemsize)
                return 0
            except Exception:  # the library fails the call (KE_ERR_DEVICE)
                import traceback
                traceback.print_exc()
                return 1

        self._collective = abi.HOST_COLLECTIVE(cb)  # kept alive with the context
        self._check(self.lib.ke_shard_init_host(self.h, rank, world, self._collective, None))

    def shard_range(self):
        lo, hi = abi.i32(), abi.i32()
        self._check(self.lib.ke_shard_range(self.h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    # ---- evaluation -------------------------------------------------------------------------
    def _stage(self, node_sets, node_scores, spread_groups, spread_domains, spread_terms, spread_domain_terms=None):
        """The next call's per-pod attachments: each keyword that is not None goes through its pod_*() staging."""
        if node_sets is not None:
            self.pod_node_sets(node_sets)
        if node_scores is not None:
            self.pod_node_scores(node_scores)
        if spread_groups is not None:
            self.pod_spread_groups(spread_groups)
        if spread_domains is not None:
            self.pod_spread_domains(spread_domains)
        if spread_terms is not None:
            self.pod_spread_terms(*spread_terms)
        if spread_domain_terms is not None:
            self.pod_spread_domain_terms(*spread_domain_terms)

    def eval(self, pods, now_ns, node_sets=None, node_scores=None, spread_groups=None, spread_domains=None,
             spread_terms=None, spread_domain_terms=None):
        """ke_eval; `node_sets` (optional): the node set id per pod (0 = every node); `node_scores` (optional): the
        score table id per pod (0 = no offset); `spread_groups` (optional): the spread group id per pod (0 = none);
        `spread_domains` (optional): the spread domain group id per pod (0 = none); `spread_terms` (optional): the
        pair (terms, members) of pod_spread_terms(); `spread_domain_terms` (optional): that of
        pod_spread_domain_terms()."""
        pods = as_pod_array(pods)
        self._stage(node_sets, node_scores, spread_groups, spread_domains, spread_terms, spread_domain_terms)
        P, N = len(pods), self.num_nodes
        out = {
            "status": np.zeros((P, N), np.uint8),
            "reason": np.zeros((P, N), np.uint8),
            "la": np.zeros((P, N), np.int16),
            "numa": np.zeros((P, N), np.int16),
            "ds": np.zeros((P, N), np.int16),
            "total": np.zeros((P, N), np.int16),
            "best": np.zeros(P, np.int32),
        }
        self._check(self.lib.ke_eval(self.h, P, abi.ptr(pods), int(now_ns), abi.ptr(out["status"]),
                                     abi.ptr(out["reason"]), abi.ptr(out["la"]), abi.ptr(out["numa"]),
                                     abi.ptr(out["ds"]), abi.ptr(out["total"]), abi.ptr(out["best"])))
        return out

    def diagnose(self, pods, now_ns, node_sets=None, bitmaps=False, spread_groups=None, spread_domains=None,
                 spread_terms=None, spread_domain_terms=None):
        """ke_diagnose: per pod the reductions of eval()'s status / reason over every node, computed on the device
        with nothing per pair copied back -- int32 [P] arrays n_nodes, n_absent, n_feasible, n_unschedulable,
        n_unresolvable, n_error, uint32 [P] plugins (abi.PLUGIN_* bits), int32 [P, 128] reason_nodes; with
        `bitmaps` also the bool [P, N] matrices feasible, unschedulable, unresolvable.  `node_sets`, `spread_groups`,
        `spread_domains`, `spread_terms` and `spread_domain_terms` (their filter kinds) as for eval()."""
        pods = as_pod_array(pods)
        self._stage(node_sets, None, spread_groups, spread_domains, spread_terms, spread_domain_terms)
        P, N = len(pods), self.num_nodes
        rec = np.zeros(P, abi.POD_DIAGNOSIS_DTYPE)
        wpp = (N + 63) // 64
        names = ("feasible", "unschedulable", "unresolvable")
        words = {k: np.zeros((P, wpp), np.uint64) for k in names} if bitmaps else {}
        self._check(self.lib.ke_diagnose(self.h, P, abi.ptr(pods), int(now_ns), abi.ptr(rec), wpp,
                                         *[abi.ptr(words.get(k)) for k in names]))
        out = {k: np.ascontiguousarray(rec[k]) for k in rec.dtype.names if k != "reserved"}
        for k, w in words.items():
            out[k] = unpack_node_sets(w, N)
        return out

    # ---- dry-run preemption ---------------------------------------------------
    def resident_pods_load(self, per_node):
        """ke_resident_pods_load: `per_node` is, per node index from 0, an array / list of RESIDENT_POD_DTYPE records
        (any order; the library keeps each list in MoreImportantPod order).  Replaces the whole table."""
        parts = [np.ascontiguousarray(np.asarray(x, abi.RESIDENT_POD_DTYPE).reshape(-1)) for x in per_node]
        off = np.zeros(len(parts) + 1, np.int32)
        off[1:] = np.cumsum([len(x) for x in parts])
        recs = np.concatenate(parts) if off[-1] else np.zeros(1, abi.RESIDENT_POD_DTYPE)
        recs = np.ascontiguousarray(recs)
        self._check(self.lib.ke_resident_pods_load(self.h, len(parts), abi.ptr(off), abi.ptr(recs)))

    def resident_pod_add(self, node, pod):
        """ke_resident_pod_add: one RESIDENT_POD_DTYPE record onto `node`'s list."""
        rec = np.ascontiguousarray(np.asarray(pod, abi.RESIDENT_POD_DTYPE).reshape(1))
        self._check(self.lib.ke_resident_pod_add(self.h, int(node), abi.ptr(rec)))

    def resident_pod_remove(self, node, uid):
        self._check(self.lib.ke_resident_pod_remove(self.h, int(node), int(uid)))

    def resident_pods_get(self, node):
        """ke_resident_pods_get: the node's list in its kept order."""
        n = abi.i32()
        out = np.zeros(abi.MAX_RESIDENT_PODS, abi.RESIDENT_POD_DTYPE)
        self._check(self.lib.ke_resident_pods_get(self.h, int(node), len(out), abi.ptr(out), C.byref(n)))
        return out[:n.value].copy()

    def pdbs_load(self, disruptions_allowed):
        """ke_pdbs_load: Status.DisruptionsAllowed per PDB; a resident record's pdb id is 1 + its index here."""
        a = np.ascontiguousarray(disruptions_allowed, np.int32).reshape(-1)
        self._check(self.lib.ke_pdbs_load(self.h, len(a), abi.ptr(a) if len(a) else None))

    def preempt(self, pods, priorities, now_ns, args=None, victims_cap=abi.MAX_RESIDENT_PODS, candidates=False,
                node_sets=None, extra_words=0):
        """ke_preempt: per pod the dry-run victim selection over every node and the pick -- int32 [P] arrays node
        (-1 = no candidate), n_victims, n_pdb_violations, n_candidates, n_skipped, n_no_victims, n_unfit, n_error,
        `victims`: int64 [P, victims_cap] uids of the picked node's victims in the reference's order (0 beyond
        min(n_victims, victims_cap)); with `candidates` also the bool [P, N] candidate matrix.  `args`: abi.PreemptArgs
        or None; `node_sets` as for eval(); `extra_words`: bitmap words per pod beyond the minimum."""
        pods = as_pod_array(pods)
        self._stage(node_sets, None, None, None, None, None)
        P, N = len(pods), self.num_nodes
        pri = np.ascontiguousarray(priorities, np.int32).reshape(-1)
        assert len(pri) == P
        rec = np.zeros(P, abi.PREEMPTION_DTYPE)
        victims = np.zeros((P, victims_cap), np.int64)
        wpp = (N + 63) // 64 + extra_words
        words = np.zeros((P, wpp), np.uint64) if candidates else None
        self._check(self.lib.ke_preempt(self.h, P, abi.ptr(pods), abi.ptr(pri), int(now_ns),
                                        C.cast(C.pointer(args), C.c_void_p) if args is not None else None, abi.ptr(rec),
                                        int(victims_cap), abi.ptr(victims), wpp, abi.ptr(words)))
        out = {k: np.ascontiguousarray(rec[k]) for k in rec.dtype.names}
        out["victims"] = victims
        if candidates:
            out["candidates"] = unpack_node_sets(words[:, :(N + 63) // 64], N)
            out["candidate_words"] = words
        return out

    def pod_gangs(self, n_pods, runs):
        """ke_pod_gangs: the gang runs of the next schedule / submit of `n_pods` pods; `runs`: an abi.GANG_RUN_DTYPE
        array, or tuples (first, count, min_member[, assumed[, mode]]), ascending and disjoint."""
        n, a = abi.gang_runs(runs)
        self._check(self.lib.ke_pod_gangs(self.h, int(n_pods), n, abi.ptr(a) if n else None))

    def last_gang_status(self, n=None):
        """ke_last_gang_status of the last schedule() / wait(): (status, tried_node) per pod."""
        n = self._last_n if n is None else n
        status, tried = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._check(self.lib.ke_last_gang_status(self.h, n, abi.ptr(status), abi.ptr(tried)))
        return status, tried

    def debug_gangs(self):
        """ke_debug_gangs of the last call: runs, runs rolled back, inverse Reserves, batches the cut rule ended."""
        out = np.zeros(4, np.int64)
        self._check(self.lib.ke_debug_gangs(self.h, abi.ptr(out)))
        return {"runs": int(out[0]), "rolled_back": int(out[1]), "inverse_reserves": int(out[2]), "cuts": int(out[3])}

    def devices_check(self):
        """ke_debug_devices_check: nodes whose DeviceShare words on the device differ from the host's derivation."""
        n = abi.i64()
        self._check(self.lib.ke_debug_devices_check(self.h, C.byref(n)))
        return n.value

    def set_gang_devices(self, on):
        """ke_set_gang_devices: with `on`, a member of a gang run may be a DeviceShare pod (off by default)."""
        self._check(self.lib.ke_set_gang_devices(self.h, 1 if on else 0))

    def debug_gang_devices(self):
        """ke_debug_gang_devices of the last call: DeviceShare inverses, cuts inside an open run, slots adopted for
        members an earlier launch placed, launches that went on from a restored run state."""
        out = np.zeros(4, np.int64)
        self._check(self.lib.ke_debug_gang_devices(self.h, abi.ptr(out)))
        return {"device_inverses": int(out[0]), "cuts_in_run": int(out[1]), "adopted": int(out[2]), "restored": int(out[3])}

    def schedule(self, pods, now_ns, matches=None, node_sets=None, node_scores=None, spread_groups=None,
                 spread_domains=None, spread_terms=None, spread_domain_terms=None, gangs=None):
        """ke_schedule; `matches` (optional): per pod the reservation indices it matches (KE_RSV_MATCHED pods);
        `node_sets` (optional): the node set id per pod (0 = every node); `node_scores` (optional): the score table
        id per pod (0 = no offset); `spread_groups` (optional): the spread group id per pod (0 = none);
        `spread_domains` (optional): the spread domain group id per pod (0 = none); `spread_terms` (optional): the
        pair (terms, members) of pod_spread_terms(); `spread_domain_terms` (optional): that of
        pod_spread_domain_terms(); `gangs` (optional): the call's gang runs as for pod_gangs()."""
        pods = as_pod_array(pods)
        if matches is not None:
            self.pod_reservations(matches)
        self._stage(node_sets, node_scores, spread_groups, spread_domains, spread_terms, spread_domain_terms)
        if gangs is not None:
            self.pod_gangs(len(pods), gangs)
        chosen = np.zeros(len(pods), np.int32)
        score = np.zeros(len(pods), np.int32)
        self._check(self.lib.ke_schedule(self.h, len(pods), abi.ptr(pods), int(now_ns), abi.ptr(chosen), abi.ptr(score)))
        self._last_n, self._last_out = len(pods), {}  # the per-pod allocations are read on first access
        return chosen, score

    def submit(self, pods, now_ns, node_sets=None, node_scores=None, spread_groups=None, spread_domains=None,
               spread_terms=None, spread_domain_terms=None, gangs=None):
        """ke_schedule_submit: enqueue a queue slice behind the calls in flight; returns its ticket (wait() collects
        it).  The pod array is kept alive here until then.  `node_sets`, `node_scores`, `spread_groups`,
        `spread_domains`, `spread_terms`, `spread_domain_terms` and `gangs` as for schedule()."""
        pods = as_pod_array(pods)
        self._stage(node_sets, node_scores, spread_groups, spread_domains, spread_terms, spread_domain_terms)
        if gangs is not None:
            self.pod_gangs(len(pods), gangs)
        t = C.c_int64()
        self._check(self.lib.ke_schedule_submit(self.h, len(pods), abi.ptr(pods), int(now_ns), C.byref(t)))
        self._inflight[t.value] = pods
        return t.value

    def wait(self, ticket):
        """ke_schedule_wait: (chosen, score) of a submitted slice, as schedule() returns them."""
        pods = self._inflight[ticket]
        chosen = np.zeros(len(pods), np.int32)
        score = np.zeros(len(pods), np.int32)
        try:
            self._check(self.lib.ke_schedule_wait(self.h, int(ticket), abi.ptr(chosen), abi.ptr(score)))
        finally:
            del self._inflight[ticket]
        self._last_n, self._last_out = len(pods), {}
        return chosen, score

    def _last(self, name, shape, dtype, fn):
        if name not in self._last_out:
            a = np.zeros(shape, dtype)
            self._check(getattr(self.lib, fn)(self.h, self._last_n, abi.ptr(a)))
            self._last_out[name] = a
        return self._last_out[name]

    @property
    def last_device_allocations(self):
        """ke_last_device_allocations of the last schedule(): allocated minors per pod."""
        return self._last("dev", self._last_n, np.uint64, "ke_last_device_allocations")

    @property
    def last_numa_allocations(self):
        """ke_last_numa_allocations of the last schedule(): [pod][NUMA id * 2 + resource]."""
        return self._last("numa", (self._last_n, 16), np.int64, "ke_last_numa_allocations")

    @property
    def last_cpusets(self):
        """ke_last_cpusets of the last schedule(): 256-bit CPU-id set per pod."""
        return self._last("cpus", (self._last_n, 4), np.uint64, "ke_last_cpusets")

    def last_allocations(self, n=None):
        """Release records (np.ndarray POD_ALLOCATION_DTYPE) of the pods of the last schedule()."""
        n = self._last_n if n is None else n
        out = np.zeros(n, abi.POD_ALLOCATION_DTYPE)
        self._check(self.lib.ke_last_allocations(self.h, n, abi.ptr(out)))
        return out

    def release(self, pod, alloc, mode=abi.RELEASE_UNRESERVE):
        """ke_pod_release: Unreserve (or informer delete) of one placement; `pod` abi.Pod or a POD_DTYPE
        record, `alloc` a POD_ALLOCATION_DTYPE record."""
        p = as_pod_array([pod] if isinstance(pod, abi.Pod) else np.asarray(pod).reshape(1))
        a = np.ascontiguousarray(np.asarray(alloc, abi.POD_ALLOCATION_DTYPE).reshape(1))
        self._check(self.lib.ke_pod_release(self.h, abi.ptr(p), abi.ptr(a), int(mode)))

    def unreserve(self, pod, queue_pos):
        """ke_unreserve: Unreserve of the pod at `queue_pos` of the last schedule()."""
        p = as_pod_array([pod] if isinstance(pod, abi.Pod) else np.asarray(pod).reshape(1))
        self._check(self.lib.ke_unreserve(self.h, abi.ptr(p), int(queue_pos)))

    def quotas_load(self, args, quotas):
        """ElasticQuota tree (include/koord_eval.h ke_quotas_load): runtime computed on the host,
        admission and Reserve applied inside schedule()."""
        quotas = np.ascontiguousarray(quotas, abi.QUOTA_DTYPE)
        self._check(self.lib.ke_quotas_load(self.h, C.byref(args), abi.ptr(quotas), len(quotas)))

    def quota_state(self, q):
        limit, used, npu = np.zeros(2, np.int64), np.zeros(2, np.int64), np.zeros(2, np.int64)
        has = np.zeros(2, np.uint8)
        self._check(self.lib.ke_quota_state(self.h, int(q), abi.ptr(limit), abi.ptr(has), abi.ptr(used), abi.ptr(npu)))
        return {"limit": limit, "limit_has": has.astype(bool), "used": used, "np_used": npu}

    def stats(self):
        total = C.c_double()
        nb = abi.i32()
        self._check(self.lib.ke_last_schedule_stats(self.h, C.byref(total), C.byref(nb), None, 0))
        per = np.zeros(max(nb.value, 1), np.float64)
        self._check(self.lib.ke_last_schedule_stats(self.h, None, None, abi.ptr(per), len(per)))
        return total.value, per[: nb.value]

    def pod_latencies(self, n):
        """per-pod latency (ms, ke_last_pod_latencies) of the n pods of the last schedule()"""
        out = np.zeros(n, np.float64)
        self._check(self.lib.ke_last_pod_latencies(self.h, n, abi.ptr(out)))
        return out

    def set_profiling(self, sample_every):
        self._check(self.lib.ke_set_profiling(self.h, sample_every))

    def rsv_fused(self):
        """(fused, gated): matched pods of the last schedule placed behind their plain segment in its call, and those
        a plain pod of the segment broke (run again alone) -- ke_debug_rsv_fused."""
        out = (abi.i64 * 2)()
        self._check(self.lib.ke_debug_rsv_fused(self.h, out))
        return int(out[0]), int(out[1])

    def ds_cuts(self):
        """DeviceShare batches of the last schedule that stopped early (NormalizeScore max may have moved)."""
        n = abi.i32()
        self._check(self.lib.ke_debug_ds_cuts(self.h, C.byref(n)))
        return n.value

    def numa_deferred(self):
        """BestEffort pairs of the last eval / schedule that needed the compacted full NUMA merge."""
        n = abi.i64()
        self._check(self.lib.ke_debug_numa_deferred(self.h, C.byref(n)))
        return n.value

    def check_records(self, now_ns):
        """Nodes whose replay record differs from one derived from their device row (0 = consistent)."""
        n = abi.i64()
        self._check(self.lib.ke_debug_check_records(self.h, int(now_ns), C.byref(n)))
        return n.value

    def set_pipeline(self, on):
        """Pipelined schedule (default): batch b's eval + select overlap batch b-1's Reserve replay.
        on: False / True, or "fixup" (pipelined with exact lists from the fixup kernel, ke_set_pipeline 2)."""
        self._check(self.lib.ke_set_pipeline(self.h, 2 if on == "fixup" else (1 if on else 0)))

    HOST_PHASES = ("checks", "refresh", "upload", "setup", "enqueue", "wait", "stats", "mirror")

    def host_stats(self):
        """Host wall ms of the last schedule() by phase (ke_last_host_stats)."""
        ms = np.zeros(8, np.float64)
        self._check(self.lib.ke_last_host_stats(self.h, abi.ptr(ms)))
        return dict(zip(self.HOST_PHASES, ms.tolist()))

    def kernel_stats(self):
        ms4 = np.zeros(8, np.float64)
        n, npipe = abi.i32(), abi.i32()
        self._check(self.lib.ke_last_kernel_stats_ex(self.h, abi.ptr(ms4), C.byref(n), C.byref(npipe)))
        p, r = C.c_double(), C.c_double()
        self._check(self.lib.ke_last_resolve_split(self.h, C.byref(p), C.byref(r)))
        sf = C.c_double()
        self._check(self.lib.ke_debug_spec_failed(self.h, C.byref(sf)))
        ph = np.zeros(6, np.float64)
        self._check(self.lib.ke_debug_resolve_phases(self.h, abi.ptr(ph)))
        sub = np.zeros(5, np.float64)
        self._check(self.lib.ke_debug_resolve_subphases(self.h, abi.ptr(sub)))
        w1 = np.zeros(4, np.float64)
        self._check(self.lib.ke_debug_resolve_wave1(self.h, abi.ptr(w1)))
        return {"eval_ms": ms4[0], "select_ms": ms4[1], "fixup_ms": ms4[2], "resolve_ms": ms4[3], "samples": n.value,
                "pipelined_batches": npipe.value, "enqueue_ms": ms4[4], "handoff_ms": ms4[5],
                "rows_fetched": ms4[6], "rows_changed": ms4[7], "spec_failed_rounds": sf.value,
                "resolve_prologue_ms": p.value, "resolve_replay_ms": r.value,
                "resolve_phases_ms": dict(zip(["prologue", "spec_predict", "spec_reserve_eval", "spec_verify", "spec_later_rounds", "writeback",
                                               "sub_t_setup", "sub_predict_loop", "sub_t_rows_wave1", "sub_reserve_R",
                                               "t_helper_hit"],
                                              ph.tolist() + sub.tolist())),
                "resolve_wave1_ms": dict(zip(["wait", "reserve", "rows", "end"], w1.tolist()))}

    def call_boundary(self):
        """The last completed device call's boundary with the call before it (ke_debug_call_boundary)."""
        out = np.zeros(4, np.int64)
        self._check(self.lib.ke_debug_call_boundary(self.h, abi.ptr(out)))
        return dict(zip(("primed_batches", "reserve_stream_copies", "reserve_stream_fills", "boundary_ns"), out.tolist()))

    def bench_eval_kernel(self, pods, now_ns, iters):
        pods = as_pod_array(pods)
        ms = C.c_double()
        self._check(self.lib.ke_bench_eval_kernel(self.h, len(pods), abi.ptr(pods), int(now_ns), iters, C.byref(ms)))
        return ms.value

    def node_state(self, i):
        """Host object state of node i: (Node, cpus, zones, devices) (ke_debug_node_state)."""
        return abi.node_state(self.lib.ke_debug_node_state, self.h, i)

    def debug_rows(self, now_ns, device=True):
        n = self.num_nodes
        host = np.zeros(n, abi.ROW_DTYPE)
        dev = np.zeros(n, abi.ROW_DTYPE) if device else None
        self._check(self.lib.ke_debug_rows(self.h, n, int(now_ns), abi.ptr(dev), abi.ptr(host)))
        return dev, host


def comm_unique_id(lib=None):
    """RCCL unique id for ke_shard_init, created on rank 0 (needs the HIP device)."""
    lib = lib or abi.load_library()
    buf = C.create_string_buffer(abi.COMM_ID_BYTES)
    rc = lib.ke_comm_unique_id(buf, abi.COMM_ID_BYTES)
    if rc != abi.OK:
        raise KoordEvalError(rc, lib.ke_last_error().decode())
    return buf.raw
