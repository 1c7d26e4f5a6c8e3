// Launch groups (include/tpgan.h tpg_group_begin / _member / _end).
// Between tpg_group_begin and tpg_group_end the halo conv, its split-K epilogue, the
// tap-flattened weight gradient and the vector activation backward are recorded instead of
// launched, tagged with the member (tpg_group_member) whose call issued them.  At the end,
// when every member issued the same sequence of kernel instances, position j of all members
// runs as ONE grouped launch (tpg_internal.h Grouped); otherwise, and for anything a member
// launches outside those four kernels (which first flushes the record: group_sync), the
// launches run one by one in their original order.  Members must be independent of each other.
//
// A groupable kernel is one record type: its argument block `a` and instance parameters, with
//   same(o)         the same kernel instance, up to what a grouped launch adapts per member
//   run()           launch alone
//   run_group(g, n) as the lead: one grid over the n >= 2 argument blocks g; -1: no grouped build
// plus its do_* below; the scheduler sees records only through these three.
#include "tpg_internal.h"
#include <algorithm>
#include <type_traits>
#include <variant>
#include <vector>

using namespace tpg;

namespace {

struct HaloRec {
  HaloArgs a;
  int dtype, cfg;
  hipStream_t s;
  bool mask;
  // (the halo capacity class may differ: the grouped launch takes the largest the members need)
  bool same(const HaloRec& o) const {
    if (s != o.s || dtype != o.dtype || mask != o.mask) return false;
    return (cfg >= 40) == (o.cfg >= 40) && (cfg >= 40 ? cfg == o.cfg : cfg % 8 == o.cfg % 8);
  }
  int run() const { return launch_halo(a, dtype, cfg, s, mask); }
  int run_group(const HaloArgs* g, int n) const { return launch_halo_group(g, n, dtype, cfg, s, mask); }
};

struct EpiRec {
  EpiArgs a;
  hipStream_t s;
  bool same(const EpiRec& o) const { return s == o.s && a.dtype == o.a.dtype; }
  int run() const { return launch_epilogue(a, s); }
  int run_group(const EpiArgs* g, int n) const { return launch_epilogue_group(g, n, s); }
};

struct Wgrad2Rec {
  Wgrad2Args a;
  int dtype, cfg, bm, bn;
  hipStream_t s;
  bool same(const Wgrad2Rec& o) const {
    return s == o.s && dtype == o.dtype && cfg == o.cfg && bm == o.bm && bn == o.bn;
  }
  int run() const { return launch_wgrad2(a, dtype, cfg, bm, bn, s); }
  int run_group(const Wgrad2Args* g, int n) const { return launch_wgrad2_group(g, n, dtype, cfg, bm, bn, s); }
};

struct ActVecRec {
  ActVecArgs a;
  int dtype;
  hipStream_t s;
  bool same(const ActVecRec& o) const { return s == o.s && dtype == o.dtype; }
  int run() const { return launch_act_vec(a, dtype, s); }
  int run_group(const ActVecArgs* g, int n) const { return launch_act_vec_group(g, n, dtype, s); }
};

using Rec = std::variant<HaloRec, EpiRec, Wgrad2Rec, ActVecRec>;

struct GLaunch {
  int member;
  Rec r;
};
struct GroupRec {
  bool active = false;
  int member = 0;
  std::vector<GLaunch> q;
};
thread_local GroupRec g_grp;

int run_one(const Rec& r) {
  return std::visit([](const auto& x) { return x.run(); }, r);
}

bool same_instance(const Rec& a, const Rec& b) {
  return a.index() == b.index() &&
         std::visit([&](const auto& x) { return x.same(std::get<std::decay_t<decltype(x)>>(b)); }, a);
}

// r[0..n) hold the record type of the lead r[0], whose instance parameters the launch takes
int run_grouped(const Rec* const* r, int n) {
  return std::visit(
      [&](const auto& lead) {
        using R = std::decay_t<decltype(lead)>;
        decltype(lead.a) a[TPG_GROUP_MAX];
        for (int k = 0; k < n; ++k) a[k] = std::get<R>(*r[k]).a;
        return lead.run_group(a, n);
      },
      *r[0]);
}

// run the recorded launches one by one, in order (the record stays active)
int group_flush() {
  if (!g_grp.active || g_grp.q.empty()) return 0;
  int rc = 0;
  for (const GLaunch& L : g_grp.q)
    if (!rc) rc = run_one(L.r);
  g_grp.q.clear();
  return rc;
}

// Members run their own launches in order; across members any interleaving is valid.  Each
// round takes the first unfinished member's next launch and groups it with every other
// member whose next launch is the same instance.
int group_run_merged() {
  std::vector<std::vector<const Rec*>> by(std::max(g_grp.member, 0) + 1);
  for (const GLaunch& L : g_grp.q) by[L.member].push_back(&L.r);
  by.erase(std::remove_if(by.begin(), by.end(), [](const std::vector<const Rec*>& v) { return v.empty(); }),
           by.end());
  const int nmem = (int)by.size();
  std::vector<size_t> head(nmem, 0);
  int rc = 0;
  for (;;) {
    int lead = -1;
    for (int m = 0; m < nmem && lead < 0; ++m)
      if (head[m] < by[m].size()) lead = m;
    if (lead < 0) break;
    const Rec& L0 = *by[lead][head[lead]];
    int mem[TPG_GROUP_MAX], n = 0;
    const Rec* rec[TPG_GROUP_MAX];
    for (int m = lead; m < nmem && n < TPG_GROUP_MAX; ++m)
      if (head[m] < by[m].size() && same_instance(*by[m][head[m]], L0)) {
        mem[n] = m;
        rec[n++] = by[m][head[m]];
      }
    int r = n >= 2 ? run_grouped(rec, n) : -1;
    if (r == -1) {  // a single member, or no grouped build of this instance: one by one
      r = 0;
      for (int k = 0; k < n && !r; ++k) r = run_one(*rec[k]);
    }
    if (r && !rc) rc = r;
    for (int k = 0; k < n; ++k) ++head[mem[k]];
  }
  g_grp.q.clear();
  return rc;
}

template <typename R>
int record(const R& r) {
  g_grp.q.push_back({std::max(g_grp.member, 0), r});
  return 0;
}

}  // namespace

int32_t tpg::group_sync() { return hip_check(group_flush(), "group flush"); }

// (the plan settled which of the two kernels takes h: plan_data clears h.pw where the pointwise
// kernel would refuse)
int tpg::do_halo(const HaloArgs& h, int dtype, int cfg, hipStream_t s, bool mask) {
  if (h.pw > 0) {  // (not a launch-group kernel: the recorded launches go first)
    const int rc = group_flush();
    return rc ? rc : launch_pw(h, dtype, s);
  }
  if (!g_grp.active) return launch_halo(h, dtype, cfg, s, mask);
  return record(HaloRec{h, dtype, cfg, s, mask});
}

int tpg::do_epilogue(const EpiArgs& e, hipStream_t s) {
  if (!g_grp.active) return launch_epilogue(e, s);
  return record(EpiRec{e, s});
}

int tpg::do_wgrad2(const Wgrad2Args& w, int dtype, int cfg, int bm, int bn, hipStream_t s) {
  if (!g_grp.active || !w.bflat) {
    const int rc = group_flush();
    return rc ? rc : launch_wgrad2(w, dtype, cfg, bm, bn, s);
  }
  return record(Wgrad2Rec{w, dtype, cfg, bm, bn, s});
}

int tpg::do_act_bwd(int n, int c, int h, int w, int act, float slope, const tpg_tensor& gy, const tpg_tensor& y,
                    const tpg_tensor& g, float* dbias, hipStream_t s) {
  if (g_grp.active) {
    ActVecArgs v;
    if (act_vec_args(n, c, h, w, act, slope, gy, y, g, dbias, &v) == 0) return record(ActVecRec{v, g.dtype, s});
    const int rc = group_flush();
    if (rc) return rc;
  }
  return launch_act_bwd(n, c, h, w, act, slope, gy, y, g, dbias, s);
}

extern "C" void tpg_group_begin(void) {
  group_flush();
  g_grp.active = true;
  g_grp.member = -1;
  g_grp.q.clear();
}

extern "C" void tpg_group_member(void) {
  if (g_grp.active) ++g_grp.member;
}

extern "C" int32_t tpg_group_end(void) {
  if (!g_grp.active) return 0;
  const int rc = g_grp.q.empty() ? 0 : group_run_merged();
  g_grp.active = false;
  g_grp.q.clear();
  return hip_check(rc, "grouped launch");
}
