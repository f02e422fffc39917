// Stand-alone host program of tests/test_pool_layout_cpu.py: runs every layout list of optas_amd/csrc/oh_carve.h on a fake base (never
// dereferenced, no GPU call) and prints each pointer's byte offset and the total as JSON.  It fails (exit status 1) when the measuring pass and
// the carving pass disagree on the size, when two takes overlap, or when two pointers of a struct come from the same take.
#include <cstdio>
#include <string>
#include <vector>

#include "oh_carve.h"

static char* const BASE = (char*)(size_t)0x40000000;
static int g_bad = 0;
static bool g_first_case = true;

struct Dump {
  struct Entry { std::string name; const void* p; bool derived; };
  std::vector<Entry> e;
  void add(const std::string& name, const void* p, const bool derived = false) { e.push_back({name, p, derived}); }
  void pair(const std::string& name, double* const (&p)[2]) { add(name + "0", p[0]); add(name + "1", p[1]); }
};

// layout(Carver&, Dump&): one layout list, and the pointers it filled by name
template <class Layout>
static void run_case(const std::string& label, const Carver::Mode mode, Layout&& layout) {
  Carver m(nullptr, mode);
  Dump dm;
  layout(m, dm);
  Carver c(BASE, mode);
  std::vector<std::pair<size_t, size_t>> log;
  c.log = &log;
  Dump d;
  layout(c, d);
  auto bad = [&](const std::string& why) { fprintf(stderr, "%s: %s\n", label.c_str(), why.c_str()); g_bad = 1; };
  if (m.bytes() != c.bytes()) bad("the measuring pass and the carving pass disagree on bytes()");
  for (const Dump::Entry& x : dm.e)
    if (x.p) bad("the measuring pass returned a pointer for " + x.name);
  size_t end = 0;
  for (const auto& t : log) {
    if (t.first < end) bad("two takes overlap");
    end = t.first + t.second;
  }
  if (end > c.bytes()) bad("a take ends beyond bytes()");
  std::vector<int> owner(log.size(), 0);
  for (const Dump::Entry& x : d.e) {
    if (!x.p || x.derived) continue;
    const size_t off = (size_t)((const char*)x.p - BASE);
    size_t k = 0;  // (an empty array and the array behind it start at the same offset: each pointer still needs a take of its own)
    while (k < log.size() && (log[k].first != off || owner[k])) ++k;
    if (k == log.size()) bad(x.name + " does not start a take of its own");
    else owner[k] = 1;
  }
  printf("%s\n  \"%s\": {\"total\": %zu", g_first_case ? "" : ",", label.c_str(), c.bytes());
  g_first_case = false;
  for (const Dump::Entry& x : d.e) printf(", \"%s\": %lld", x.name.c_str(), x.p ? (long long)((const char*)x.p - BASE) : -1LL);
  printf("}");
}

static void dump_fig(Dump& d, const FigBuffers& D) {
  d.pair("q", D.q); d.pair("q_spare", D.q_spare); d.pair("Z", D.Z); d.pair("Dr", D.Dr); d.pair("g", D.g); d.pair("phi", D.phi); d.pair("cv", D.cv);
  d.pair("Gfull", D.Gfull); d.add("G_spare", D.G_spare); d.pair("mdl", D.mdl); d.pair("E", D.E); d.pair("gt", D.gt); d.pair("merit", D.merit);
  d.add("zstep", D.zstep); d.add("Kmat", D.Kmat); d.add("kvec", D.kvec); d.add("ref", D.ref); d.add("fconst", D.fconst); d.add("f_cur", D.f_cur);
  d.add("pred", D.pred); d.add("mu", D.mu); d.add("nun", D.nun); d.add("stat", D.stat); d.add("feas", D.feas); d.add("lam_h", D.lam_h); d.add("lead", D.lead);
  d.add("cur", D.cur); d.add("first", D.first); d.add("skip", D.skip); d.add("polish", D.polish); d.add("stale", D.stale); d.add("status", D.status);
  d.add("iters", D.iters); d.add("orig", D.orig); d.add("newidx", D.newidx); d.add("n_running", D.n_running); d.add("n_new", D.n_new); d.add("work", D.work);
  d.add("n_defer", D.n_defer, true); d.add("scan_blk", D.scan_blk); d.add("defer_list", D.defer_list);
}
static void dump_guards(Dump& d, const GuardBuffers& GB, const double* fpsi) {
  d.add("lam", GB.lam); d.add("par", GB.par); d.pair("psi", GB.psi); d.add("rho", GB.rho); d.add("rho_next", GB.rho_next); d.add("omega", GB.omega);
  d.add("meas_prev", GB.meas_prev); d.add("fpsi", fpsi); d.pair("mcv", GB.mcv); d.add("meas", GB.meas); d.add("lamv", GB.lamv); d.add("lam_out", GB.lam_out);
  d.add("lamv_out", GB.lamv_out); d.add("scr", GB.scr); d.add("ls_gd", GB.ls_gd); d.add("ls_q", GB.ls_q); d.add("outer", GB.outer); d.add("n_outer", GB.n_outer);
  d.add("ls_count", GB.ls_count);
}
static void dump_tq(Dump& d, const TqBuffers& D) {
  d.add("xs", D.xs); d.add("st", D.st); d.add("lam", D.lam); d.add("gains", D.gains); d.add("goal", D.goal); d.add("f_cur", D.f_cur); d.add("f_true", D.f_true);
  d.add("bsum", D.bsum); d.add("mu", D.mu); d.add("nun", D.nun); d.add("mub", D.mub); d.add("stat", D.stat); d.add("alpha", D.alpha); d.add("qk", D.qk);
  d.add("ndx", D.ndx); d.add("viol", D.viol); d.add("cur", D.cur); d.add("first", D.first); d.add("curv", D.curv); d.add("status", D.status); d.add("iters", D.iters);
  d.add("rejected", D.rejected); d.add("n_barrier", D.n_barrier); d.add("nrel", D.nrel); d.add("n_back", D.n_back); d.add("stall", D.stall);
  d.add("curv_age", D.curv_age); d.add("list", D.list); d.add("n_running", D.n_running); d.add("n_list", D.n_list);
}
static void dump_pm(Dump& d, const PmBuffers& D) {
  d.add("a", D.a); d.add("X", D.X); d.add("s", D.s); d.add("lam", D.lam); d.add("K", D.K); d.add("kk", D.kk); d.add("dX", D.dX); d.add("da", D.da);
}
static void dump_stage(Dump& d, const StageLayout& L) {
  d.add("x0", L.x0); d.add("p", L.p); d.add("x", L.x); d.add("f", L.f); d.add("kkt", L.kkt); d.add("iters", L.iters); d.add("status", L.status);
}

int main() {
  printf("{");
  const int traj[5][4] = {{7, 1, 50, 64}, {7, 1, 50, 262144 + 13 * 64}, {4, 1, 3, 64}, {2, 0, 3, 128}, {8, 0, 128, 192}};  // ndof, lock, T, Bp
  for (const auto& t : traj)
    run_case("traj ndof=" + std::to_string(t[0]) + " lock=" + std::to_string(t[1]) + " T=" + std::to_string(t[2]) + " Bp=" + std::to_string(t[3]), Carver::Packed,
             [&](Carver& c, Dump& d) {
               FigBuffers D{};
               layout_fig(c, D, t[0], t[1], t[2], t[3]);
               dump_fig(d, D);
             });
  // guard pool, 7 joints, 5 knots: limits only; 2 sphere links x 3 obstacles with velocity rows; velocity rows only
  const int N = 7, T = 5;
  const int guards[3][4] = {{1, 0, 0, 0}, {0, 2, 3, 1}, {0, 0, 0, 1}};  // limits, n_links, n_obs, vel
  for (const auto& g : guards)
    for (const int Bp : {64, 192})
      run_case("guards limits=" + std::to_string(g[0]) + " links=" + std::to_string(g[1]) + " obs=" + std::to_string(g[2]) + " vel=" + std::to_string(g[3]) +
                   " Bp=" + std::to_string(Bp),
               Carver::Packed, [&](Carver& c, Dump& d) {
                 GuardParams GP{};
                 GP.limits = g[0]; GP.n_links = g[1]; GP.n_obs = g[2]; GP.vel = g[3];
                 GP.NC = (g[0] ? 2 * N : 0) + g[1] * g[2];
                 GuardBuffers GB{};
                 double* fpsi = nullptr;
                 layout_guards(c, GB, fpsi, GP, N, T, Bp);
                 dump_guards(d, GB, fpsi);
               });
  const int tq[2][3] = {{2, 2, 1}, {7, 30, 100}};  // N, T, B
  for (const auto& t : tq)
    run_case("tq N=" + std::to_string(t[0]) + " T=" + std::to_string(t[1]) + " B=" + std::to_string(t[2]), Carver::Packed, [&](Carver& c, Dump& d) {
      TqBuffers D{};
      layout_tq(c, D, t[2], t[1]);
      dump_tq(d, D);
    });
  for (const int Tp : {2, 20})
    run_case("pm T=" + std::to_string(Tp) + " Bp=64", Carver::Packed, [&](Carver& c, Dump& d) {
      PmBuffers D{};
      layout_pm(c, D, Tp, 64);
      dump_pm(d, D);
    });
  // staging of oh_solve, a shape of every problem kind (nx, npar, mult as shape_of gives them)
  const struct { const char* kind; Shape sh; } kinds[] = {
      {"figure_eight", {7 * 5 + 7 * 4, 7, 4 * 5}},  // 7 joints, 5 knots, orientation-locked
      {"point_mass", {4 * 4, 4 + 4 * 4, 0}},        // T = 4
      {"ik", {7, 7 + 3, 3 + 2 * 7}},
      {"qp", {4, 16 + 4 + 2 * 4 + 2 + 1 * 4 + 1, 3}},  // n = 4, m = 2, me = 1
      {"tape", {3, 1, 2}},
      {"torque", {4 * 2 * 4, 2 * 2 + 3 * 4, 4 * 2 * 2}},  // 2 joints, T = 4
  };
  for (const auto& k : kinds)
    for (const size_t B : {(size_t)1, (size_t)33})
      run_case(std::string("stage ") + k.kind + " B=" + std::to_string(B), Carver::Slots, [&](Carver& c, Dump& d) {
        StageLayout L{};
        layout_stage(c, L, k.sh, B);
        dump_stage(d, L);
      });
  printf("\n}\n");
  return g_bad;
}
