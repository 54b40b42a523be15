// Does a walker.h issue the same calls as another one?  A stand-alone host program (no GPU, nothing of the library
// linked): Walker<LogOps>, where LogOps writes one line per call the walker makes of its Ops and of its transport, with
// every argument -- pointers as offsets from a made-up base, counters as offsets into the counter array, a PanelRef as
// its P, bases and firsts -- and after run() the return code, info, upd_launches, upd_flops (%.17g), flow_waves and
// regimes[].  The pure accessors (tile, winv, stream, sem, flow_event, the capability queries) are not logged.
//
// Build it once per checkout, against that checkout's walker.h (OTHER is typically the parent commit:
// git worktree add ../parent HEAD~1), and compare the outputs:
//   hipcc --offload-arch=gfx950 --offload-host-only -x hip -O1 -DWALKER_H='"THIS/dense_linear_app_amd/csrc/walker.h"' \
//         scripts/walker_calls.cpp -o walker_calls_this        (and the same with OTHER/... -o walker_calls_other)
//   ./walker_calls_this sweep > this.txt; ./walker_calls_other sweep > other.txt; cmp this.txt other.txt
// `sweep` prints one line per case -- the case, the number of lines of its log and a digest of them -- for the sweeps
// of tests/test_schedule_check.py (every switch set of SWITCHES on one GPU and of GRID_SWITCHES on every rank of its
// eight grids, with every capability on), and under the default switches the one-GPU sweep without counters and both
// sweeps with every capability off (CbOps in dist.hip); its last line is the number of cases.  Without an argument
// the cases come from stdin, one per line, and their whole logs are printed (the switches: the environment's):
//   nt mb p q rank t_tile t_panel profiling counters pipe_ok can_split_trsm flow_ok
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <string>

#ifndef WALKER_H
#define WALKER_H "../dense_linear_app_amd/csrc/walker.h"
#endif
#include WALKER_H

extern "C" int chol_internal_fail(int code, const char *msg) {
  printf("chol_internal_fail %d %s\n", code, msg);
  return code;
}
bool cholmi::flow_applies(int nbm) { return nbm >= 3 && nbm <= 4; }  // (the library's default)

using namespace cholmi;

struct Case {
  int nt, mb, p, q, rank;
  double t_tile, t_panel;
  int profiling, counters, pipe_ok, split, flow_ok;
};

struct Log {
  bool print;
  long lines = 0;
  uint64_t digest = 1469598103934665603ull;  // FNV-1a over the lines
  void operator()(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
    char b[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof b, fmt, ap);
    va_end(ap);
    ++lines;
    if (print) puts(b);
    for (const char *c = b; *c; ++c) digest = (digest ^ (unsigned char)*c) * 1099511628211ull;
    digest = (digest ^ '\n') * 1099511628211ull;
  }
};

struct LogOps {
  const WaveGeo &g;
  const Case &c;
  Log &log;
  char *const base = reinterpret_cast<char *>(uintptr_t(1) << 40);
  size_t next;  // (the local tiles, the two block-inverse workspaces, then whatever the walker allocates)
  std::vector<int> sems;
  LogOps(const WaveGeo &geo, const Case &cs, Log &l) : g(geo), c(cs), log(l) { next = ((size_t)g.lmt * std::max(1, g.lnt) + 2) * g.tile_bytes; }
  long off(const void *p) const { return p ? (long)((const char *)p - base) : -1; }
  long ctr(const int *p) const { return p ? (long)(p - sems.data()) : -1; }
  std::string ref(const PanelRef *p) const {
    if (!p) return "none";
    std::string s = "P" + std::to_string(p->P);
    for (int i = 0; i < p->P; ++i) s += " " + std::to_string(off(p->base[i])) + "/" + std::to_string(p->first[i]);
    return s;
  }
  bool profiling() const { return c.profiling; }
  bool counters() const { return c.counters; }
  bool pipe_ok() const { return c.pipe_ok; }
  bool can_split_trsm() const { return c.split; }
  bool flow_ok() const { return c.flow_ok; }
  void *flow_event() { return base - 64; }
  void *stream(int st) { return reinterpret_cast<void *>(uintptr_t(st + 1)); }
  char *tile(int il, int jl) { return base + ((size_t)il + (size_t)jl * g.lmt) * g.tile_bytes; }
  void *winv(int par) { return base + ((size_t)g.lmt * std::max(1, g.lnt) + par) * g.tile_bytes; }
  int *sem(int k, int which, int per_wave) { return sems.data() + ((size_t)per_wave * k + which) * 32; }
  void *alloc(size_t bytes) {
    void *p = base + next;
    next += bytes;
    log("alloc %zu -> %ld", bytes, off(p));
    return p;
  }
  int begin(int nevents, int nt, int sem_per_wave) {
    sems.assign((size_t)nt * sem_per_wave * 32 + 32, 0);
    log("begin %d %d %d", nevents, nt, sem_per_wave);
    return 0;
  }
  int rec(int ev, int st) { return log("rec %d %d", ev, st), 0; }
  int wt(int st, int ev) { return log("wt %d %d", st, ev), 0; }
  int panel(int k, char *lkk, void *wv, char *tiles, int ntiles, int ev_steps, int ev_head, const SyrkPipe *sy, const int *wait_sem, int wait_target) {
    char s[256] = "none";
    if (sy)
      snprintf(s, sizeof s, "c %ld su %ld sem %ld fc %ld sflow %ld ev_flow %ld join %d", off(sy->c), (long)(uintptr_t)sy->su, ctr(sy->sem), ctr(sy->fc),
               (long)(uintptr_t)sy->sflow, off(sy->ev_flow), (int)sy->join_flow);
    log("panel %d %ld %ld %ld %d %d %d sy %s wait %ld %d", k, off(lkk), off(wv), off(tiles), ntiles, ev_steps, ev_head, s, ctr(wait_sem), wait_target);
    return 0;
  }
  int trsm(int k, char *tiles, int ntiles, const char *lkk, const char *wv, int st) {
    return log("trsm %d %ld %d %ld %ld %d", k, off(tiles), ntiles, off(lkk), off(wv), st), 0;
  }
  int diag_syrk(int k, int j, char *C, const char *A, int st) { return log("diag_syrk %d %d %ld %ld %d", k, j, off(C), off(A), st), 0; }
  int update(int k1, int k2, int jlo, int jhi, int what, const PanelRef &p1, const PanelRef *p2, bool yield, int st) {
    return log("update %d %d %d %d %d [%s] [%s] %d %d", k1, k2, jlo, jhi, what, ref(&p1).c_str(), ref(p2).c_str(), (int)yield, st), 0;
  }
  int update_col_small(int k, int st) { return log("update_col_small %d %d", k, st), 0; }
  int finish(int ev_start, int ev_stop, const std::vector<std::pair<int, int>> &brackets, int *info) {
    std::string s;
    for (auto &b : brackets) s += " " + std::to_string(b.first) + ":" + std::to_string(b.second);
    log("finish %d %d%s", ev_start, ev_stop, s.c_str());
    *info = 0;
    return 0;
  }
  // the transport: ctx is a channel of this engine
  struct Chan {
    LogOps *o;
    int id;
  } chan[2] = {{this, 0}, {this, 1}};
  static int t_begin(void *x) { return ((Chan *)x)->o->log("group_begin ch%d", ((Chan *)x)->id), 0; }
  static int t_end(void *x) { return ((Chan *)x)->o->log("group_end ch%d", ((Chan *)x)->id), 0; }
  static int t_send(void *x, const void *buf, size_t bytes, int peer, void *stream) {
    Chan *c = (Chan *)x;
    return c->o->log("send ch%d %ld %zu %d %ld", c->id, c->o->off(buf), bytes, peer, (long)(uintptr_t)stream), 0;
  }
  static int t_recv(void *x, void *buf, size_t bytes, int peer, void *stream) {
    Chan *c = (Chan *)x;
    return c->o->log("recv ch%d %ld %zu %d %ld", c->id, c->o->off(buf), bytes, peer, (long)(uintptr_t)stream), 0;
  }
  static int t_allreduce(void *x, long long *v) { return ((Chan *)x)->o->log("allreduce_max ch%d %lld", ((Chan *)x)->id, *v), 0; }
};

static void run_case(const Case &c, bool print) {
  WaveGeo g;
  g.init(c.nt, c.mb, c.p, c.q, c.rank, 8);
  Log log{print};
  LogOps ops(g, c, log);
  WaveComm cm;
  for (int ch = 0; ch < 2; ++ch) {
    cm.ch[ch].ctx = &ops.chan[ch];
    cm.ch[ch].group_begin = LogOps::t_begin;
    cm.ch[ch].send = LogOps::t_send;
    cm.ch[ch].recv = LogOps::t_recv;
    cm.ch[ch].group_end = LogOps::t_end;
    cm.ch[ch].allreduce_max = LogOps::t_allreduce;
  }
  WaveCalib cal;
  cal.t_tile = c.t_tile, cal.t_panel = c.t_panel;
  Walker<LogOps> w(ops, g, c.p * c.q > 1 ? &cm : nullptr, cal);
  long long info = -1;
  int rc = w.setup();
  if (!rc) rc = w.run(&info);
  std::string r;
  for (int x : w.regimes) r += " " + std::to_string(x);
  log("rc %d info %lld upd_launches %d upd_flops %.17g flow_waves %d regimes%s", rc, info, w.upd_launches, w.upd_flops, w.flow_waves, r.c_str());
  if (!print)
    printf("%d %d %d %d %d %.17g %.17g %d %d %d %d %d: %ld lines, digest %016" PRIx64 "\n", c.nt, c.mb, c.p, c.q, c.rank, c.t_tile, c.t_panel,
           c.profiling, c.counters, c.pipe_ok, c.split, c.flow_ok, log.lines, log.digest);
}

// ---- the sweeps of tests/test_schedule_check.py
static const char *const NAMES[] = {"PAIR_FACTOR", "YIELD_FACTOR", "PIPE_FACTOR", "FLOW_FACTOR", "FLOW_RUN_FACTOR", "HALVES_MAX_ROUNDS", "NEAR_FACTOR", "U1_SMALL"};
#define PAIR "PAIR_FACTOR="
#define PIPE "PIPE_FACTOR="
#define YIELD "YIELD_FACTOR="
#define NEAR "NEAR_FACTOR="
#define FLOW "FLOW_FACTOR="
#define FLOW_RUN "FLOW_RUN_FACTOR="
#define HALVES "HALVES_MAX_ROUNDS="
#define U1 "U1_SMALL="
static const char *const SWITCHES[] = {
    "", PAIR "0", PAIR "1000", PAIR "0 " HALVES "1000 " PIPE "0", PIPE "100 " PAIR "1000", PIPE "0.02", PIPE "0",
    PIPE "0 " HALVES "1000 " PAIR "1000", HALVES "0 " PIPE "0", YIELD "0", YIELD "1000", NEAR "0", U1 "0", NEAR "0 " U1 "0",
    PIPE "100 " PAIR "1000 " NEAR "100 " U1 "64", PIPE "0.3 " NEAR "100 " HALVES "1000 " PAIR "1000", NEAR "0.3",
    FLOW "100 " PIPE "100 " PAIR "1000", FLOW "0.05", FLOW_RUN "0", FLOW_RUN "100", PAIR "0 " FLOW "0.1", PAIR "0 " FLOW "100 " PIPE "100"};
static const char *const GRID_SWITCHES[] = {"", PAIR "0", PAIR "1000", PIPE "100 " PAIR "1000", PIPE "0", PAIR "0 " HALVES "1000 " PIPE "0", YIELD "1000"};
// "PAIR_FACTOR=0 PIPE_FACTOR=100": CHOLMI_PAIR_FACTOR=0 CHOLMI_PIPE_FACTOR=100, every other switch unset
static void set_switches(const char *s) {
  for (const char *n : NAMES) unsetenv((std::string("CHOLMI_") + n).c_str());
  printf("switches: %s\n", *s ? s : "default");
  for (std::string rest = s; !rest.empty();) {
    const size_t sp = std::min(rest.find(' '), rest.size()), eq = rest.find('=');
    setenv(("CHOLMI_" + rest.substr(0, eq)).c_str(), rest.substr(eq + 1, sp - eq - 1).c_str(), 1);
    rest = rest.substr(std::min(sp + 1, rest.size()));
  }
}
struct Speeds {
  int mb;
  double t_tile, t_panel;
};
static const Speeds TRIPLES[] = {{512, 3.8e-6, 700e-6}, {384, 1.6e-6, 570e-6}, {256, 0.5e-6, 350e-6}, {1024, 30e-6, 1400e-6}, {128, 0.06e-6, 180e-6}};
static const double SCALES[] = {1.0, 0.05, 20.0};

static long sweep_one_gpu(int counters, int others) {
  long n = 0;
  for (const Speeds &s : TRIPLES)
    for (int nt : {1, 2, 3, 4, 5, 7, 8, 12, 16, 17, 24, 33, 48})
      for (double scale : SCALES)
        for (int prof = 0; prof <= others; ++prof, ++n)
          run_case(Case{nt, s.mb, 1, 1, 0, s.t_tile, s.t_panel * scale, prof, counters, others, others, others}, false);
  return n;
}
static long sweep_grids(int caps) {
  const int grids[8][2] = {{2, 1}, {1, 2}, {2, 2}, {4, 2}, {2, 4}, {3, 2}, {4, 1}, {3, 3}};
  long n = 0;
  for (auto &gr : grids)
    for (int nt : {1, 2, 3, 5, 8, 13, 24, 40})
      for (int t : {0, 3, 4})
        for (double scale : SCALES)
          for (int rank = 0; rank < gr[0] * gr[1]; ++rank, ++n)
            run_case(Case{nt, TRIPLES[t].mb, gr[0], gr[1], rank, TRIPLES[t].t_tile, TRIPLES[t].t_panel * scale, caps ? rank & 1 : 0, caps, caps, caps, caps},
                     false);
  return n;
}

int main(int argc, char **argv) {
  if (argc > 1 && std::string(argv[1]) == "sweep") {
    long n = 0;
    for (const char *s : SWITCHES) set_switches(s), n += sweep_one_gpu(1, 1);
    for (const char *s : GRID_SWITCHES) set_switches(s), n += sweep_grids(1);
    set_switches("");
    n += sweep_one_gpu(0, 1);  // HipOps without a counter array
    n += sweep_one_gpu(0, 0);  // CbOps: every capability off (profiling among them: one case where the tests have two)
    n += sweep_grids(0);
    printf("%ld cases\n", n);
    return 0;
  }
  Case c;
  while (scanf("%d %d %d %d %d %lf %lf %d %d %d %d %d", &c.nt, &c.mb, &c.p, &c.q, &c.rank, &c.t_tile, &c.t_panel, &c.profiling, &c.counters, &c.pipe_ok,
               &c.split, &c.flow_ok) == 12) {
    printf("case %d %d %d %d %d %g %g %d %d %d %d %d\n", c.nt, c.mb, c.p, c.q, c.rank, c.t_tile, c.t_panel, c.profiling, c.counters, c.pipe_ok, c.split,
           c.flow_ok);
    run_case(c, true);
  }
  return 0;
}
