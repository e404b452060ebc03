// The host half of ke_diagnose, free of HIP: the KE_REASON_* tables (the plugin's message and KE_PLUGIN_* bit of a
// reason), the layout of the raw per-pod tallies the kernels add into, and the fold of one pod's tallies into its
// ke_pod_diagnosis.  ke_kernels.hip and ke_capi.cpp include it; tests/diag/diag_check.cpp compiles it alone with g++.
#pragma once
#include <stdint.h>

#include "../../include/koord_eval.h"

namespace ke {

// ---- the raw tallies: DIAG_WORDS uint32 per pod, zeroed by the host before the launch -------------------------------
// [0, KE_DIAG_REASONS): nodes per reason of the pairs that reached a classification (a feasible or KE_CODE_ERROR
// pair counts under KE_REASON_NONE, as ke_eval's reason[] holds it); then one counter per class.  An empty node slot
// counts under DIAG_ABSENT alone.
constexpr int DIAG_ABSENT = KE_DIAG_REASONS;
constexpr int DIAG_FEASIBLE = KE_DIAG_REASONS + 1;
constexpr int DIAG_UNSCHEDULABLE = KE_DIAG_REASONS + 2;
constexpr int DIAG_UNRESOLVABLE = KE_DIAG_REASONS + 3;
constexpr int DIAG_ERROR = KE_DIAG_REASONS + 4;
constexpr int DIAG_WORDS = KE_DIAG_REASONS + 8;
// the three optional bitmaps, in ke_diagnose's argument order
constexpr int DIAG_BIT_FEASIBLE = 0, DIAG_BIT_UNSCHEDULABLE = 1, DIAG_BIT_UNRESOLVABLE = 2, DIAG_BITMAPS = 3;

// the largest KE_REASON_* define of each plugin's range (include/koord_eval.h) has a bin, so every reason has one
static_assert(KE_REASON_LA_AGG_USAGE_MEMORY < KE_DIAG_REASONS && KE_REASON_NUMA_INSUFFICIENT_CPUS < KE_DIAG_REASONS &&
                  KE_REASON_DS_NO_MATCHED_TEMPLATE < KE_DIAG_REASONS && KE_REASON_RSV_INSUFFICIENT_NUMA < KE_DIAG_REASONS &&
                  KE_REASON_FIT_INSUFFICIENT_SCALAR < KE_DIAG_REASONS && KE_REASON_NODE_SET < KE_DIAG_REASONS,
              "a KE_REASON_* at or above KE_DIAG_REASONS");
static_assert((KE_DIAG_REASONS & (KE_DIAG_REASONS - 1)) == 0, "the kernels mask a reason into its bin");

// ---- reason -> plugin (the header's ranges) -------------------------------------------------------------------------
inline uint32_t diag_reason_plugin(int32_t r) {
  if (r >= 1 && r <= 15) return KE_PLUGIN_LOADAWARE;
  if (r >= 16 && r <= 31) return KE_PLUGIN_NODENUMARESOURCE;
  if (r >= 32 && r <= 49) return KE_PLUGIN_DEVICESHARE;
  if (r >= 50 && r <= 63) return KE_PLUGIN_RESERVATION;
  if (r >= 64 && r <= 95) return KE_PLUGIN_NODERESOURCESFIT;
  if (r == KE_REASON_NODE_SET) return KE_PLUGIN_NODE_SET;
  return 0u;
}

// ---- reason -> the plugin's message (the strings include/koord_eval.h quotes beside each define) --------------------
inline const char* diag_reason_message(int32_t r) {
  switch (r) {
    case KE_REASON_LA_NODEMETRIC_EXPIRED: return "node(s) nodeMetric expired";
    case KE_REASON_LA_USAGE_CPU: return "node(s) cpu usage exceed threshold";
    case KE_REASON_LA_USAGE_MEMORY: return "node(s) memory usage exceed threshold";
    case KE_REASON_LA_AGG_USAGE_CPU: return "node(s) cpu aggregated usage exceed threshold";
    case KE_REASON_LA_AGG_USAGE_MEMORY: return "node(s) memory aggregated usage exceed threshold";
    case KE_REASON_NUMA_INSUFFICIENT_AMPLIFIED_CPU: return "Insufficient amplified cpu";
    case KE_REASON_NUMA_INVALID_AMPLIFICATION_RATIO: return "node(s) invalid CPU amplification ratio";
    case KE_REASON_NUMA_INVALID_CPU_TOPOLOGY: return "node(s) invalid CPU Topology";
    case KE_REASON_NUMA_POLICY_CONFLICT: return "node(s) NUMA Topology policy cannot match";
    case KE_REASON_NUMA_MISSING_RESOURCES: return "node(s) missing NUMA resources";
    case KE_REASON_NUMA_HINT_UNALIGNED: return "Unaligned NUMA Hint cannot be aligned";
    case KE_REASON_NUMA_INSUFFICIENT_RESOURCES: return "Insufficient NUMA <resource>";
    case KE_REASON_NUMA_INVALID_REQUESTED_CPUS: return "the requested CPUs must be integer";
    case KE_REASON_NUMA_CPU_BIND_POLICY_CONFLICT: return "node(s) cpu bind policy conflicts with pod's required cpu bind policy";
    case KE_REASON_NUMA_SMT_ALIGNMENT: return "node(s) requested cpus not multiple cpus per core";
    case KE_REASON_NUMA_INSUFFICIENT_CPUS: return "not enough cpus available to satisfy request";
    case KE_REASON_DS_INVALID_REQUEST: return "invalid resource device requests";
    case KE_REASON_DS_INSUFFICIENT_GPU: return "Insufficient gpu devices";
    case KE_REASON_DS_INSUFFICIENT_RDMA: return "Insufficient rdma devices";
    case KE_REASON_DS_INSUFFICIENT_FPGA: return "Insufficient fpga devices";
    case KE_REASON_DS_MISSING_PARTITION_TABLE: return "node(s) missing GPU Partition Table";
    case KE_REASON_DS_UNSUPPORTED_GPU_REQUESTS: return "node(s) Unsupported number of GPU requests";
    case KE_REASON_DS_INSUFFICIENT_PARTITIONED: return "Insufficient Partitioned GPU Devices";
    case KE_REASON_DS_MISSING_TOPOLOGY_TREE: return "node(s) missing GPU Device Topology Tree";
    case KE_REASON_DS_MULTI_SHARED_GPU: return "node(s) Unsupported Multi-Shared GPU";
    case KE_REASON_DS_INSUFFICIENT_TOPOLOGY_SCOPED: return "Insufficient Topology Scoped GPU Devices";
    case KE_REASON_DS_INSUFFICIENT_GPU_TOPOLOGY: return "Insufficient GPU Devices";
    case KE_REASON_DS_INSUFFICIENT_NUMA_SCOPED: return "Insufficient NUMA Scoped Devices";
    case KE_REASON_DS_INVALID_HINT: return "invalid Selector / VFSelector of DeviceHint";
    case KE_REASON_DS_INSUFFICIENT_RDMA_VF: return "Insufficient rdma VirtualFunctions";
    case KE_REASON_DS_INSUFFICIENT_FPGA_VF: return "Insufficient fpga VirtualFunctions";
    case KE_REASON_DS_INSUFFICIENT_PRIMARY: return "node(s) Insufficient primary device";
    case KE_REASON_DS_JOINT_VIOLATION: return "node(s) Device Joint-Allocate rules violation";
    case KE_REASON_DS_NO_MATCHED_TEMPLATE: return "no matched GPU shared resource template";
    case KE_REASON_RSV_INSUFFICIENT_CPUS: return "Reservation(s) not enough cpus available to satisfy request";
    case KE_REASON_RSV_INSUFFICIENT_DEVICES: return "Reservation(s) Insufficient <device type> devices";
    case KE_REASON_RSV_AFFINITY: return "node(s) no reservations match reservation affinity";
    case KE_REASON_RSV_INSUFFICIENT_NUMA: return "Reservation(s) Insufficient NUMA <resource>";
    case KE_REASON_FIT_TOO_MANY_PODS: return "Too many pods";
    case KE_REASON_FIT_INSUFFICIENT_CPU: return "Insufficient cpu";
    case KE_REASON_FIT_INSUFFICIENT_MEMORY: return "Insufficient memory";
    case KE_REASON_FIT_INSUFFICIENT_SCALAR: return "Insufficient <resource name>";
    case KE_REASON_NODE_SET: return "node(s) didn't match the pod's node set";
    default: return "";
  }
}

// ---- the fold -------------------------------------------------------------------------------------------------------
// One pod's raw tallies into its ke_pod_diagnosis; `n_slots` = ke_num_nodes.  False when the tallies break an
// invariant of the struct (a kernel fault: the caller fails the call, nothing is returned half-counted).
inline bool diag_fold(const uint32_t* raw, int32_t n_slots, ke_pod_diagnosis* out) {
  ke_pod_diagnosis d{};
  d.n_absent = (int32_t)raw[DIAG_ABSENT];
  d.n_feasible = (int32_t)raw[DIAG_FEASIBLE];
  d.n_unschedulable = (int32_t)raw[DIAG_UNSCHEDULABLE];
  d.n_unresolvable = (int32_t)raw[DIAG_UNRESOLVABLE];
  d.n_error = (int32_t)raw[DIAG_ERROR];
  d.n_nodes = d.n_feasible + d.n_unschedulable + d.n_unresolvable + d.n_error;
  int64_t failing = 0;
  for (int r = 0; r < KE_DIAG_REASONS; r++) {
    d.reason_nodes[r] = (int32_t)raw[r];
    if (r && raw[r]) {
      failing += raw[r];
      d.plugins |= diag_reason_plugin(r);
    }
  }
  *out = d;
  return d.n_nodes + d.n_absent == n_slots && failing == (int64_t)d.n_unschedulable + d.n_unresolvable &&
         d.reason_nodes[0] == d.n_feasible + d.n_error;
}

}  // namespace ke
