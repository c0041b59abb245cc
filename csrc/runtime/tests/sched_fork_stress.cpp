// Sanitizer stress test of the families of the continuous-batching core
// (csrc/runtime/sched_core.h add_fork), run by tests/test_fork.py under
// AddressSanitizer + UBSan.
//
// Random workloads as in sched_core_stress.cpp -- several replicas and groups,
// slot pools smaller than the demand, chunked prefill under a token budget,
// readouts 0-3 steps late -- in which about half the requests ask for 2 to
// min(cap, slots, 6) samples (want = 1 parents among them), and every few runs
// end in a reset() with families in flight.  A naive model keeps who owns which
// slot and checks at every step:
//   * a fork's chunk is (L - 1, 1, final), in the step after its parent's
//     final chunk, in the parent's (replica, group), ahead of the group's other
//     chunks, and forks() lists exactly these chunks with the parent's slot;
//   * no slot has two owners, and the source slot is still its parent's;
//   * a parent's RELEASE comes with the read-back of an item planned at or
//     after its forks' step;
//   * every sequence is released once, no slot leaks, no pending readouts.
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <map>
#include <random>
#include <tuple>
#include <vector>

#include "../sched_core.h"

using namespace lsd_rt;

static int fail(const char* what, long long v) {
  std::fprintf(stderr, "FAIL: %s (%lld)\n", what, v);
  return 1;
}

struct Track {
  int64_t parent = -1;
  int L = 0;
  int rep = -1, slot = -1;          // from the first chunk on
  int64_t final_step = -1, fork_step = -1;  // its final chunk; (parents) the step of its forks' chunks
  int final_rep = -1, final_g = -1;
  bool released = false;
};

static long g_forked = 0;  // fork chunks planned, over every seed

static int run(unsigned seed) {
  std::mt19937 rnd(seed);
  auto pick = [&](std::vector<int> v) { return v[rnd() % v.size()]; };
  const int R = pick({1, 2}), M = pick({1, 2, 3}), cap = pick({2, 3, 8});
  const int slots = pick({cap, cap + 1, cap * M});
  const int budget = pick({0, 5, 64}), chunk = pick({0, 3, 9});
  const bool collect = seed % 2 == 1, reset_early = seed % 5 == 4;
  const int eos = 3;
  std::vector<SlotAllocator> pools;
  for (int r = 0; r < R; ++r) pools.emplace_back(slots);
  std::vector<SlotAllocator*> pp;
  for (auto& p : pools) pp.push_back(&p);
  SchedCore core(R, M, cap, budget, chunk, 4096, pp);
  if (seed % 3 == 0) core.set_join_policy(3, 2);
  std::map<int64_t, Track> seqs;
  std::map<std::pair<int, int>, int64_t> owner;  // (rep, slot) -> sid
  std::deque<std::tuple<int64_t, int, int, int>> pending;  // step, rep, g, n
  int64_t sid = 0;
  long forked = 0;
  auto on_release = [&](int64_t s, int64_t st) -> int {
    Track& t = seqs.at(s);
    if (t.released) return fail("released twice", s);
    t.released = true;
    // the read-back of step st returns the item planned at st - 1
    if (t.fork_step >= 0 && st - 1 < t.fork_step) return fail("a parent's slot came back before its forks' item", s);
    if (t.slot >= 0) {
      auto it = owner.find({t.rep, t.slot});
      if (it == owner.end() || it->second != s) return fail("released a slot it does not own", s);
      owner.erase(it);
    }
    return 0;
  };
  auto readout = [&](int64_t st, int rep, int g, int n, bool random_tokens) -> int {
    std::vector<int> toks(n);
    for (int& t : toks) t = random_tokens ? pick({eos, 11, 12, 13}) : 11;
    std::vector<Event> ev;
    if (collect) {
      std::vector<int32_t> t32(toks.begin(), toks.end());
      ev = core.assign_collect(rep, st, g, t32.data(), n, eos).first;
    } else {
      ev = core.assign(rep, st, g, toks, eos);
    }
    for (const auto& e : ev)
      if (std::get<2>(e) & EV_RELEASE)
        if (int rc = on_release(std::get<0>(e), st)) return rc;
    return 0;
  };
  for (int64_t step = 0; step < 20000; ++step) {
    if (step < 120 && rnd() % 10 < 3) {
      const int reqs = 1 + rnd() % 3;
      for (int q = 0; q < reqs; ++q) {
        const int top = std::min({cap, slots, 6});
        const int n = (rnd() % 2 && top >= 2) ? 2 + (int)(rnd() % (top - 1)) : 1;
        const int L = 1 + rnd() % 40;
        const bool stop = rnd() % 2;
        const int64_t par = sid++;
        core.add(par, L, pick({1, 1, 3, 20}), stop);
        seqs[par].L = L;
        for (int i = 1; i < n; ++i) {
          const int64_t f = sid++;
          core.add_fork(f, par, pick({1, 2, 9}), stop);
          seqs[f].L = L;
          seqs[f].parent = L > 1 ? par : -1;  // a one-token prompt: a plain sequence
        }
      }
    }
    if (!core.has_work()) {
      if (step >= 120) break;
      continue;
    }
    if (reset_early && step == 60) {
      core.reset();
      for (auto& p : pools)
        if (p.available() != slots) return fail("reset leaked a slot", p.available());
      if (core.has_work() || core.n_expect() != 0) return fail("work left after reset", step);
      return 0;
    }
    std::vector<int64_t> admitted;
    auto plans = core.plan(step, &admitted);
    std::vector<std::pair<int64_t, int>> in_plan;
    for (int rep = 0; rep < R; ++rep)
      for (const auto& go : plans[rep]) {
        const int g = std::get<0>(go), ret = std::get<1>(go);
        const auto& chunks = std::get<6>(go);
        bool past_forks = false;
        for (const auto& c : chunks) {
          const int64_t s = std::get<0>(c);
          const int slot = std::get<1>(c), start = std::get<2>(c), len = std::get<3>(c);
          const bool final = std::get<4>(c);
          Track& t = seqs.at(s);
          const bool is_fork = t.parent >= 0 && t.slot < 0;
          if (t.slot < 0) {
            if (owner.count({rep, slot})) return fail("a slot has two owners", slot);
            owner[{rep, slot}] = s;
            t.rep = rep;
            t.slot = slot;
          } else if (t.rep != rep || t.slot != slot) {
            return fail("a sequence changed its slot", s);
          }
          if (is_fork) {
            if (past_forks) return fail("a fork chunk behind another chunk", s);
            Track& p = seqs.at(t.parent);
            if (start != t.L - 1 || len != 1 || !final) return fail("a fork's chunk is not (L - 1, 1, final)", s);
            if (p.final_step != step - 1 || p.final_rep != rep || p.final_g != g)
              return fail("a fork chunk not one step after its parent's final chunk, in its group", s);
            if (p.released || owner[{p.rep, p.slot}] != t.parent) return fail("the source slot is not the parent's", s);
            p.fork_step = step;
            in_plan.emplace_back(s, p.slot);
            ++forked;
          } else {
            past_forks = true;
          }
          if (final) {
            t.final_step = step;
            t.final_rep = rep;
            t.final_g = g;
          }
        }
        if (ret) pending.emplace_back(step, rep, g, ret);
      }
    if (in_plan != core.forks()) return fail("forks() does not list the plan's fork chunks", step);
    const int lag = rnd() % 4;
    while (!pending.empty() && std::get<0>(pending.front()) <= step - lag) {
      auto [st, rep, g, n] = pending.front();
      pending.pop_front();
      if (int rc = readout(st, rep, g, n, true)) return rc;
    }
    if (step == 19999) return fail("the workload did not drain", step);
  }
  while (!pending.empty()) {
    auto [st, rep, g, n] = pending.front();
    pending.pop_front();
    if (int rc = readout(st, rep, g, n, false)) return rc;
  }
  if (core.n_expect() != 0) return fail("pending readouts", core.n_expect());
  for (auto& kv : seqs)
    if (!kv.second.released) return fail("a sequence was never released", kv.first);
  if (!owner.empty()) return fail("owned slots left", (long long)owner.size());
  for (auto& p : pools)
    if (p.available() != slots) return fail("slot leak", p.available());
  g_forked += forked;
  return 0;
}

int main(int argc, char** argv) {
  const int runs = argc > 1 ? std::atoi(argv[1]) : 16;
  for (int s = 0; s < runs; ++s)
    if (int rc = run(1234u + (unsigned)s)) {
      std::fprintf(stderr, "seed %d failed\n", s);
      return rc;
    }
  if (g_forked <= 0) return fail("no fork chunk was ever planned", g_forked);
  std::printf("ok %d (%ld fork chunks)\n", runs, g_forked);
  return 0;
}
