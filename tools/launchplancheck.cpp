// TEST TOOL ONLY: a host compile of the launch plan's plain-C++ header (art_launch_plan.h: which kernels
// one propagate launch runs), for tools/launchplancheck.py and tests/test_launch_plan.py:
//     launchplancheck builds             the instantiation lists as data, one build per line:
//                                        "propagate INTEG GEOM SAVE DON WPS CYC" / "tail GEOM"
//     launchplancheck plan KEY=VALUE ... one plan: the record's decision half as "key=value" lines, then
//                                        "bulk_exists=0|1 cont_exists=0|1"; the keys are LaunchPlanIn's fields
//     launchplancheck streamed N GEOM BLOCKS   the streamed host call's plan, likewise
//     launchplancheck sweep              the full input grid: every plan must name builds of the lists (else
//                                        "FAIL ..." and exit status 1); prints each build some input reached
//                                        as "reached propagate ..." / "reached tail GEOM", and each listed
//                                        build nothing reached as "unreached ..."
// Without arguments: the sweep's check alone, then "launchplan OK" (exit status 1 on a failure).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "../adiabatic_raytracer_amd/csrc/art_launch_plan.h"

using namespace art;

static const char* geom_name(int g) { return g == LP_GEOM_FLAT ? "FLAT" : (g == LP_GEOM_GR ? "GR" : "ANY"); }
static const char* integ_name(int i) { return i == ART_RK4 ? "rk4" : "vern6"; }

static std::vector<LaunchBuild> listed() {
  std::vector<LaunchBuild> v;
#define ART_LP_ADD(I, G, S, D, W, C) v.push_back(LaunchBuild{I, G, S, D, W, C});
  ART_BUILDS_FLAT(ART_LP_ADD) ART_BUILDS_NL(ART_LP_ADD) ART_BUILDS_NL_CYC(ART_LP_ADD)
#undef ART_LP_ADD
  return v;
}
static std::vector<int> listed_tails() {
  std::vector<int> v;
#define ART_LP_ADD(G) v.push_back(G);
  ART_BUILDS_TAIL(ART_LP_ADD)
#undef ART_LP_ADD
  return v;
}
static bool tail_exists(int g) {
  for (int t : listed_tails())
    if (t == g) return true;
  return false;
}

using Key = std::tuple<int, int, int, int, int, int>;
static Key key(const LaunchBuild& b) { return Key{b.integrator, b.geom, (int)b.save, b.don, b.wps, (int)b.cyc}; }
static void print_build(const char* head, const LaunchBuild& b) {
  std::printf("%spropagate %s %s %d %d %d %d\n", head, integ_name(b.integrator), geom_name(b.geom), (int)b.save, b.don, b.wps,
              (int)b.cyc);
}

static void print_plan(const LaunchPlan& P, bool streamed) {
  const art_launch_path r = plan_record(P, streamed);
  std::printf("launches=%d\nstreamed=%d\nsmall_tail=%d\nbulk=%d\nintegrator=%s\ngeom=%s\nsave=%d\ndon=%d\nwps=%d\ncyc=%d\n", r.launches,
              r.streamed, r.small_tail, r.bulk, integ_name(r.integrator), geom_name(r.geom), r.save, r.don, r.wps, r.cyc);
  std::printf("bulk_grid=%d\ndonate=%d\ncont=%d\ncont_wps=%d\ncont_donate=%d\ntail=%d\ntail_geom=%s\ntail_grid=%d\n", r.bulk_grid, r.donate,
              r.cont, r.cont_wps, r.cont_donate, r.tail, geom_name(r.tail_geom), r.tail_grid);
  std::printf("hot=%d\nsorted=%d\ngraduate=%d\nhot_at=%d\n", r.hot, r.sorted, r.graduate, r.hot_at);
  // beside the record: the scratch the plan lays out, the continuation's build and grid, and whether the builds exist
  std::printf("ncont=%zu\nnhot=%zu\ngrad_records=%d\nhot_records=%d\ncont_grid=%d\ncont_geom=%s\ncont_don=%d\n", P.ncont, P.nhot,
              (int)P.grad_records, (int)P.hot_records, P.cont ? P.cont_grid : 0, geom_name(P.cont_build.geom),
              P.cont ? P.cont_build.don : 0);
  std::printf("bulk_exists=%d\ncont_exists=%d\ntail_exists=%d\n", (int)(!P.bulk || build_exists(P.bulk_build)),
              (int)(!P.cont || build_exists(P.cont_build)), (int)(!P.tail || tail_exists(P.tail_geom)));
}

static int geom_arg(const char* v) {
  if (!std::strcmp(v, "FLAT")) return LP_GEOM_FLAT;
  if (!std::strcmp(v, "GR")) return LP_GEOM_GR;
  return LP_GEOM_ANY;
}

static bool set_field(LaunchPlanIn* in, const std::string& k, const char* v) {
  const long long x = std::atoll(v);
  if (k == "n") in->n = x;
  else if (k == "integrator") in->integrator = !std::strcmp(v, "rk4") ? ART_RK4 : ART_VERN6;
  else if (k == "geom") in->geom = geom_arg(v);
  else if (k == "save") in->save = x != 0;
  else if (k == "cyc") in->cyc = x != 0;
  else if (k == "donate_caller") in->donate_caller = (int)x;
  else if (k == "donate_device") in->donate_device = (int)x;
  else if (k == "graduate_device") in->graduate_device = (int)x;
  else if (k == "graduate_env") in->graduate_env = (int)x;
  else if (k == "tail_rays") in->tail_rays = (int)x;
  else if (k == "tail_donate") in->tail_donate = (int)x;
  else if (k == "w1") in->w1 = x != 0;
  else if (k == "small_tail") {  // ART_SMALL_TAIL
    in->small_tail_set = true;
    in->small_tail_max = x;
  } else if (k == "nonblocking") in->nonblocking = x != 0;
  else if (k == "hot_at_env") in->hot_at_env = (int)x;
  else if (k == "hot_order") in->hot_order = x != 0;
  else if (k == "ncu") in->ncu = (int)x;
  else if (k == "blocks_per_cu") in->blocks_per_cu = (int)x;
  else return false;
  return true;
}

// The full input grid. Every plan must name builds that exist; reached: the builds some plan named.
static int sweep(std::set<Key>* reached, std::set<int>* reached_tails, long long* plans) {
  const int64_t ns[] = {1, 512, 1024, 1025, 2048, 65536, 65537, 1000000};
  const int donates[] = {-1, 0, 16};
  const int grads[] = {-1, 0, 64};
  const int tails[] = {0, 1, 100000};
  const int hot_ats[] = {0, 128};
  const int bpcs[] = {0, 1, 2};
  struct SmallTail { bool set; int64_t max; };
  const SmallTail sts[] = {{false, 0}, {true, 0}};
  for (int integ : {ART_VERN6, ART_RK4})
    for (int geom : {LP_GEOM_ANY, LP_GEOM_FLAT, LP_GEOM_GR})
      for (int mode = 0; mode < 3; ++mode)  // plain, saveat, cyclotron
        for (int64_t n : ns)
          for (int dc : donates)
            for (int dd : donates)
              for (int gd : grads)
                for (int tr : tails)
                  for (int w1 = 0; w1 < 2; ++w1)
                    for (const SmallTail& st : sts)
                      for (int nb = 0; nb < 2; ++nb)
                        for (int ha : hot_ats)
                          for (int bpc : bpcs) {
                            if (mode == 2 && integ == ART_RK4) continue;  // (the entry points refuse it)
                            LaunchPlanIn in;
                            in.n = n; in.integrator = integ; in.geom = geom; in.save = mode == 1; in.cyc = mode == 2;
                            in.donate_caller = dc; in.donate_device = dd; in.graduate_device = gd; in.tail_rays = tr;
                            in.w1 = w1 != 0; in.small_tail_set = st.set; in.small_tail_max = st.max;
                            in.nonblocking = nb != 0; in.hot_at_env = ha; in.ncu = 256; in.blocks_per_cu = bpc;
                            const LaunchPlan P = plan_launch(in);
                            ++*plans;
                            if ((P.bulk && !build_exists(P.bulk_build)) || (P.cont && !build_exists(P.cont_build)) ||
                                (P.tail && !tail_exists(P.tail_geom)) || (P.hot && !tail_exists(P.tail_geom)) ||
                                (!P.bulk && !P.tail)) {
                              std::printf("FAIL a plan names a build nobody instantiated: integrator=%s geom=%s mode=%d n=%lld "
                                          "donate=%d/%d graduate=%d tail=%d w1=%d small_tail=%d nonblocking=%d\n",
                                          integ_name(integ), geom_name(geom), mode, (long long)n, dc, dd, gd, tr, w1, (int)st.set, nb);
                              return 1;
                            }
                            if (P.bulk) reached->insert(key(P.bulk_build));
                            if (P.cont) reached->insert(key(P.cont_build));
                            if (P.tail || P.hot) reached_tails->insert(P.tail_geom);
                          }
  // the streamed host call's integrator: Vern6 in every geometry
  for (int geom : {LP_GEOM_ANY, LP_GEOM_FLAT, LP_GEOM_GR}) {
    const LaunchPlan P = plan_streamed(1000000, geom, 496);
    ++*plans;
    if (!build_exists(P.bulk_build)) {
      std::printf("FAIL the streamed plan names a build nobody instantiated: geom=%s\n", geom_name(geom));
      return 1;
    }
    reached->insert(key(P.bulk_build));
  }
  return 0;
}

int main(int argc, char** argv) {
  const std::string what = argc > 1 ? argv[1] : "";
  if (what == "builds") {
    for (const LaunchBuild& b : listed()) print_build("", b);
    for (int g : listed_tails()) std::printf("tail %s\n", geom_name(g));
    return 0;
  }
  if (what == "plan") {
    LaunchPlanIn in;
    for (int i = 2; i < argc; ++i) {
      const char* eq = std::strchr(argv[i], '=');
      if (!eq || !set_field(&in, std::string(argv[i], eq - argv[i]), eq + 1)) {
        std::printf("FAIL unknown argument %s\n", argv[i]);
        return 2;
      }
    }
    print_plan(plan_launch(in), false);
    return 0;
  }
  if (what == "streamed" && argc == 5) {
    print_plan(plan_streamed(std::atoll(argv[2]), geom_arg(argv[3]), std::atoi(argv[4])), true);
    return 0;
  }
  if (what == "sweep" || argc == 1) {
    std::set<Key> reached;
    std::set<int> tails;
    long long plans = 0;
    if (sweep(&reached, &tails, &plans)) return 1;
    if (argc == 1) {
      std::printf("launchplan OK\n");
      return 0;
    }
    std::printf("plans %lld\n", plans);
    for (const LaunchBuild& b : listed()) print_build(reached.count(key(b)) ? "reached " : "unreached ", b);
    for (int g : listed_tails()) std::printf("%stail %s\n", tails.count(g) ? "reached " : "unreached ", geom_name(g));
    return 0;
  }
  return 2;
}
