// ke_preempt.h alone (no HIP, no library): a line-driven driver for tests/test_preempt_host.py, built with
// -fsanitize=address,undefined and run as a program.  One command a line on stdin, one answer line each:
//   cap C                                      a fresh table of C node slots           -> "0"
//   add NODE <record>                          resident_add                            -> rc
//   rm NODE UID                                resident_remove                         -> rc
//   drop NODE                                  resident_drop                           -> "0"
//   get NODE CAP                               resident_get                            -> rc n uid...
//   load N off[0..N] K, then K <record> lines  resident_load                           -> rc
//   pack N NPDBS                               resident_pack -> rc total, then N+1 offsets, then a line per record
//   less <key a> <key b>                       preempt_key_less(a, b), preempt_key_less(b, a) -> "x y"
// <record> = uid priority start_ns cpu mem quota non_preemptible n_pdb pdb0 pdb1; <key> = violations hi_prio sum
// n_victims hi_start node.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../../koordinator_amd/csrc/ke_preempt.h"

using namespace ke;

static ke_resident_pod read_record(std::istream& in) {
  ke_resident_pod r{};
  long long uid, start, cpu, mem;
  int prio, quota, np, npdb, p0, p1;
  in >> uid >> prio >> start >> cpu >> mem >> quota >> np >> npdb >> p0 >> p1;
  r.uid = uid, r.priority = prio, r.start_ns = start, r.requests[KE_RES_CPU] = cpu, r.requests[KE_RES_MEMORY] = mem;
  r.quota = (int16_t)quota, r.non_preemptible = (uint8_t)np, r.n_pdb = (uint8_t)npdb;
  r.pdb[0] = (uint16_t)p0, r.pdb[1] = (uint16_t)p1;
  return r;
}
static PreemptKey read_key(std::istream& in) {
  long long viol, hi, cnt, start, node;
  unsigned long long sum;
  in >> viol >> hi >> sum >> cnt >> start >> node;
  return preempt_key((int32_t)viol, (int32_t)hi, sum, (int32_t)cnt, (int64_t)start, (int32_t)node);
}

int main() {
  ResidentTable t;
  std::string line;
  const char* why = "";
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "cap") {
      int c;
      in >> c;
      t = ResidentTable();
      t.nodes.resize((size_t)c);
      std::printf("0\n");
    } else if (cmd == "add") {
      int node;
      in >> node;
      const ke_resident_pod r = read_record(in);
      std::printf("%d\n", resident_add(t, node, &r, &why));
    } else if (cmd == "rm") {
      int node;
      long long uid;
      in >> node >> uid;
      std::printf("%d\n", resident_remove(t, node, uid, &why));
    } else if (cmd == "drop") {
      int node;
      in >> node;
      resident_drop(t, node);
      std::printf("0\n");
    } else if (cmd == "get") {
      int node, cap;
      in >> node >> cap;
      std::vector<ke_resident_pod> out((size_t)(cap > 0 ? cap : 1));
      int32_t n = -1;
      const int rc = resident_get(t, node, cap, cap > 0 ? out.data() : nullptr, &n, &why);
      std::printf("%d %d", rc, n);
      for (int j = 0; rc == 0 && j < n && j < cap; j++) std::printf(" %lld", (long long)out[(size_t)j].uid);
      std::printf("\n");
    } else if (cmd == "load") {
      int n, k;
      in >> n;
      std::vector<int32_t> off((size_t)(n > 0 ? n + 1 : 1));
      for (int i = 0; i <= n && n > 0; i++) in >> off[(size_t)i];
      in >> k;
      std::vector<ke_resident_pod> recs;
      for (int j = 0; j < k; j++) {
        std::getline(std::cin, line);
        std::istringstream rin(line);
        recs.push_back(read_record(rin));
      }
      std::printf("%d\n", resident_load(t, n, off.data(), recs.data(), &why));
    } else if (cmd == "pack") {
      int n, npdb;
      in >> n >> npdb;
      std::vector<int32_t> off;
      std::vector<DevResident> rec;
      std::vector<int64_t> uid;
      const int rc = resident_pack(t, n, npdb, off, rec, uid, &why);
      std::printf("%d %lld %d\n", rc, (long long)t.total, (int)t.dirty);
      if (rc) continue;
      for (int32_t o : off) std::printf("%d ", o);
      std::printf("\n");
      for (size_t j = 0; j < rec.size(); j++)
        std::printf("%lld %lld %lld %d %lld %u %u %d %d\n", (long long)uid[j], (long long)dr_cpu(rec[j]), (long long)rec[j].mem,
                    rec[j].priority, (long long)rec[j].start_ns, dr_pdb0(rec[j]), (unsigned)rec[j].pdb1, (int)rec[j].quota,
                    (int)rec[j].flags);
    } else if (cmd == "less") {
      const PreemptKey a = read_key(in), b = read_key(in);
      std::printf("%d %d\n", (int)preempt_key_less(a, b), (int)preempt_key_less(b, a));
    } else {
      std::printf("?\n");
      return 2;
    }
  }
  return 0;
}
