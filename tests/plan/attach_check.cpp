// A call's per-pod attachments (koordinator_amd/csrc/ke_attach.h) compiled alone for the host, for
// tests/test_attach_host.py.
//   attach_check modes   for each of the 24 legal combinations of kinds (sets x scores x domains x {none, group ids,
//                        term lists}) and n_pods in {0, 1, 5} one line: "sets scores domains gt n_pods | ns ns_filter
//                        batch_ns(false) batch_ns(true) | ids groups domains terms total | plan_groups plan_domains"
//                        (gt: 0 none, 1 group ids, 2 term lists; offsets in int32 words, -1 = no such section;
//                        plan_groups: 0 nullptr, 1 the group ids, 2 the term marks; plan_domains: 0 nullptr, 1 the ids)
//   attach_check apply   apply_placements over a stand-in context of 2 spread groups x 4 nodes and one domain group
//                        over one map (nodes 0..3 in domains 0, 1, none, 0).  Reads commands, prints the tables
//                        ("sg" the 8 counts, "sd" domains 0..1 and the sum of the other 62) after each:
//                          set g node v                 sg_cnt[g - 1][node] = v
//                          groups n  id.. chosen..      a call with spread group ids
//                          terms n  m1 m2 .. chosen..   a call with term records of two members each (0 = none)
//                          domains n  id.. chosen..     a call with spread domain group ids
//                          slot                         AttachSlot's stage / take sequence, prints its states
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../koordinator_amd/csrc/ke_attach.h"

using namespace ke;

struct Tables {
  int32_t sg_n = 2, sd_n = 1;
  int64_t sg_stride = 4, sd_stride = 4;
  std::vector<uint16_t> sg_cnt = std::vector<uint16_t>(8, 0);
  std::vector<uint16_t> sd_map = {0, 1, (uint16_t)KE_DOMAIN_NONE, 0};
  std::vector<int32_t> sd_gmap = {1};
  std::vector<uint32_t> sd_cnt = std::vector<uint32_t>(KE_MAX_SPREAD_DOMAINS, 0u);
};

static int modes() {
  const int32_t ids[5] = {1, 0, 2, 1, 0};
  const PodTerms recs[5] = {};
  for (int sets = 0; sets < 2; sets++)
    for (int scores = 0; scores < 2; scores++)
      for (int domains = 0; domains < 2; domains++)
        for (int gt = 0; gt < 3; gt++)
          for (int n : {0, 1, 5}) {
            CallAttach a;
            if (sets) a.sets = ids;
            if (scores) a.scores = ids;
            if (domains) a.domains = ids;
            if (gt == 1) a.groups = ids;
            if (gt == 2) {
              a.terms = recs;
              a.listed.assign(5, 1);
            }
            const AttachLayout l(a, n);
            const int32_t* pg = a.plan_groups();
            std::printf("%d %d %d %d %d | %d %d %d %d | %lld %lld %lld %lld %lld | %d %d\n", sets, scores, domains, gt, n, a.ns(),
                        a.ns_filter(), a.batch_ns(false), a.batch_ns(true), (long long)l.ids, (long long)l.groups,
                        (long long)l.domains, (long long)l.terms, (long long)l.total,
                        pg == nullptr ? 0 : pg == ids ? 1 : pg == a.listed.data() ? 2 : -1, a.plan_domains() == nullptr ? 0 : 1);
            // the completion's snapshot holds the kinds whose Reserves the host follows, n entries each
            const PlacedAttach s(a, n);
            if (s.groups.size() != (gt == 1 ? (size_t)n : 0) || s.domains.size() != (domains ? (size_t)n : 0) ||
                s.terms.size() != (gt == 2 ? (size_t)n : 0))
              return 1;
          }
  return 0;
}

static void print_tables(const Tables& t) {
  std::printf("sg");
  for (uint16_t v : t.sg_cnt) std::printf(" %u", (unsigned)v);
  uint64_t rest = 0;
  for (size_t d = 2; d < t.sd_cnt.size(); d++) rest += t.sd_cnt[d];
  std::printf(" sd %u %u %llu\n", t.sd_cnt[0], t.sd_cnt[1], (unsigned long long)rest);
}

static int apply() {
  Tables t;
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "set") {
      int g, node, v;
      std::cin >> g >> node >> v;
      t.sg_cnt[(size_t)((g - 1) * t.sg_stride + node)] = (uint16_t)v;
    } else if (cmd == "slot") {
      AttachSlot<int32_t> s;
      const int32_t v[3] = {7, 8, 9};
      const bool t0 = s.take();  // nothing staged
      s.stage(v, 3);
      const bool on = s.on;
      const bool t1 = s.take();  // the staging becomes the call's
      const size_t n1 = s.call.size(), st1 = s.staged.size();
      const bool t2 = s.take();  // and the next call has none
      std::printf("slot %d %d %d %zu %zu %d %zu %d\n", (int)t0, (int)on, (int)t1, n1, st1, (int)t2, s.call.size(), (int)s.on);
      continue;
    } else {
      int n;
      std::cin >> n;
      CallAttach a;
      std::vector<int32_t> ids((size_t)n), chosen((size_t)n);
      std::vector<PodTerms> recs((size_t)n, PodTerms{});
      if (cmd == "terms") {
        for (int p = 0; p < n; p++)
          for (int m = 0; m < 2; m++) {
            uint32_t g;
            std::cin >> g;
            recs[(size_t)p].mem[m >> 1] |= g << ((m & 1) * 16);
          }
        a.terms = recs.data();
      } else {
        for (int p = 0; p < n; p++) std::cin >> ids[(size_t)p];
        if (cmd == "groups") a.groups = ids.data();
        else if (cmd == "domains") a.domains = ids.data();
        else return 2;
      }
      for (int p = 0; p < n; p++) std::cin >> chosen[(size_t)p];
      apply_placements(t, PlacedAttach(a, n), chosen.data());
    }
    print_tables(t);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "modes")) return modes();
  if (argc == 2 && !std::strcmp(argv[1], "apply")) return apply();
  return 2;
}
