// Sanitizer stress test of the stop sequences of the continuous-batching core
// (csrc/runtime/sched_core.h set_stops), run by tests/test_stop.py under
// AddressSanitizer + UBSan.
//
// Random workloads as in sched_core_stress.cpp -- several replicas and groups,
// slot pools smaller than the demand, chunked prefill, readouts 0-3 steps late
// -- in which about two sequences in three carry random stop lists (up to 8
// sequences of 1 to 32 tokens, often longer than the output), a random
// min_tokens, and tokens from an alphabet of four, so stop material comes up
// often.  Every run goes through assign or through assign_collect.  A naive
// model keeps each sequence's whole output and decides, token by token, what
// the core must report:
//   * EOS first (stop_at_eos), then the first stop sequence equal to the
//     output's last tokens, counted only past min_tokens;
//   * FINISH exactly at that token or at the want-th, STOP exactly with a
//     counting match that is not an EOS stop;
//   * assign_collect's finished token lists equal the model's outputs;
//   * each sequence is released once, no slot leaks, no pending readouts.
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
  int want = 0, min_tokens = 0;
  bool stop_at_eos = false;
  std::vector<std::vector<int>> stops;
  std::vector<int> out;
  bool finished = false, released = false, collected = false;
};

// the rule, on the whole output
static bool naive_match(const Track& t) {
  const int n = (int)t.out.size();
  if (n <= t.min_tokens) return false;
  for (const auto& w : t.stops) {
    const int m = (int)w.size();
    if (m > n) continue;
    bool eq = true;
    for (int i = 0; i < m; ++i) eq = eq && t.out[n - m + i] == w[i];
    if (eq) return true;
  }
  return false;
}

static int run(unsigned seed) {
  std::mt19937 rnd(seed);
  auto pick = [&](std::vector<int> v) { return v[rnd() % v.size()]; };
  const int R = pick({1, 2, 3}), M = pick({1, 2, 4}), cap = pick({1, 3, 8, 16});
  const int slots = pick({1, 5, cap * M * R});
  const int budget = pick({0, 7, 64}), chunk = pick({0, 4, 9});
  const bool collect = seed % 2 == 1;
  const int eos = 3;
  std::vector<SlotAllocator> pools;
  for (int r = 0; r < R; ++r) pools.emplace_back(slots);
  std::vector<SlotAllocator*> pp;
  for (auto& p : pools) pp.push_back(&p);
  SchedCore core(R, M, cap, budget, chunk, 4096, pp);
  std::map<int64_t, Track> seqs;
  std::deque<std::tuple<int64_t, int, int, int>> pending;  // step, rep, g, n
  int64_t sid = 0;
  // one token event of sequence s against the model
  auto token = [&](int64_t s, int tok, int fl) -> int {
    auto it = seqs.find(s);
    if (it == seqs.end()) return fail("event for an unknown sequence", s);
    Track& t = it->second;
    if (t.finished) return fail("token after finish", s);
    if ((fl & EV_FIRST) != (t.out.empty() ? EV_FIRST : 0)) return fail("first-token flag", s);
    t.out.push_back(tok);
    const bool eos_stop = t.stop_at_eos && tok == eos;
    const bool stop = !eos_stop && naive_match(t);
    const bool done = (int)t.out.size() >= t.want || eos_stop || stop;
    if (done != bool(fl & EV_FINISH)) return fail("finish flag", s);
    if (stop != bool(fl & EV_STOP)) return fail("stop flag", s);
    if (done) t.finished = true;
    return 0;
  };
  auto drain = [&](int64_t upto) -> int {
    while (!pending.empty() && std::get<0>(pending.front()) <= upto) {
      const auto [st, rep, g, n] = pending.front();
      pending.pop_front();
      std::vector<int> toks(n);
      for (int& t : toks) t = rnd() % 4;
      std::vector<Event> ev;
      SchedCore::Finished done;
      if (collect) {
        std::vector<int32_t> t32(toks.begin(), toks.end());
        auto r = core.assign_collect(rep, st, g, t32.data(), n, eos);
        ev = std::move(r.first);
        done = std::move(r.second);
      } else {
        ev = core.assign(rep, st, g, toks, eos);
      }
      for (const auto& e : ev) {
        const int64_t s = std::get<0>(e);
        const int tok = std::get<1>(e), fl = std::get<2>(e);
        auto it = seqs.find(s);
        if (it == seqs.end()) return fail("event for an unknown sequence", s);
        Track& t = it->second;
        if (fl & EV_RELEASE) {
          if (t.released) return fail("released twice", s);
          t.released = true;
          if (fl & EV_FINISH) t.finished = true;
          continue;
        }
        if (collect) continue;  // checked from the finished lists below
        if (int rc = token(s, tok, fl)) return rc;
      }
      for (const auto& d : done) {
        auto it = seqs.find(d.first);
        if (it == seqs.end()) return fail("finished list of an unknown sequence", d.first);
        Track& t = it->second;
        if (t.collected) return fail("finished twice", d.first);
        t.collected = true;
        // replay the list through the model: it must end exactly where the model ends
        for (size_t i = 0; i < d.second.size(); ++i) {
          if (t.finished) return fail("tokens past the model's end", d.first);
          t.out.push_back(d.second[i]);
          const bool eos_stop = t.stop_at_eos && d.second[i] == eos;
          if ((int)t.out.size() >= t.want || eos_stop || naive_match(t)) t.finished = true;
        }
        if (!t.finished && !d.second.empty()) return fail("finished list ends early", d.first);
      }
      if (collect)
        for (const auto& e : ev) {  // the STOP bit of a collected finish
          const int fl = std::get<2>(e);
          if ((fl & EV_RELEASE) || !(fl & EV_FINISH)) continue;
          const Track& t = seqs.at(std::get<0>(e));
          const bool eos_stop = t.stop_at_eos && !t.out.empty() && t.out.back() == eos;
          if ((!eos_stop && naive_match(t)) != bool(fl & EV_STOP)) return fail("stop flag", std::get<0>(e));
        }
    }
    return 0;
  };
  for (int64_t step = 0; step < 2000000; ++step) {
    if (step < 300 && rnd() % 3 == 0)
      for (int k = rnd() % 5; k >= 0; --k) {
        Track t;
        t.want = 1 + rnd() % 60;
        t.stop_at_eos = rnd() % 2 == 0;
        const int64_t id = sid++;
        core.add(id, 1 + rnd() % 60, t.want, t.stop_at_eos);
        if (rnd() % 3 != 0) {
          t.min_tokens = pick({0, 0, 1, 3, (int)(rnd() % 40)});
          std::vector<int> flat, lens;
          for (int e = 1 + rnd() % 8; e > 0; --e) {
            const int m = pick({1, 1, 2, 2, 3, 5, 32, (int)(1 + rnd() % 32)});
            std::vector<int> w(m);
            for (int& x : w) x = rnd() % 4;
            flat.insert(flat.end(), w.begin(), w.end());
            lens.push_back(m);
            t.stops.push_back(std::move(w));
          }
          core.set_stops(id, flat, lens, t.min_tokens);
        }
        seqs[id] = std::move(t);
      }
    if (!core.has_work()) {
      if (step >= 300) break;
      continue;
    }
    std::vector<int64_t> adm;
    const auto plans = core.plan(step, &adm);
    for (size_t rep = 0; rep < plans.size(); ++rep)
      for (const auto& go : plans[rep]) {
        if (std::get<3>(go) > cap) return fail("bucket above capacity", std::get<3>(go));
        if (std::get<1>(go)) pending.emplace_back(step, (int)rep, std::get<0>(go), std::get<1>(go));
      }
    if (int rc = drain(step - (int64_t)(rnd() % 4))) return rc;
  }
  if (int rc = drain(1LL << 60)) return rc;
  if (core.has_work()) return fail("work left", core.n_seqs());
  if (core.n_expect() != 0) return fail("readouts left", core.n_expect());
  for (auto& p : pools)
    if (p.available() != slots) return fail("slots leaked", slots - p.available());
  for (const auto& kv : seqs) {
    const Track& t = kv.second;
    if (!t.released || !t.finished) return fail("sequence never completed", kv.first);
    if ((int)t.out.size() > t.want) return fail("token count", kv.first);
    if (collect && !t.collected) return fail("no finished list", kv.first);
  }
  // set_stops refuses what it cannot hold
  int refused = 0;
  core.add(sid, 3, 4, false);
  for (auto bad : {std::make_pair(std::vector<int>{1, 2}, std::vector<int>{1}),
                   std::make_pair(std::vector<int>{}, std::vector<int>{0}),
                   std::make_pair(std::vector<int>(33, 1), std::vector<int>{33})})
    try {
      core.set_stops(sid, bad.first, bad.second, 0);
    } catch (const std::invalid_argument&) {
      ++refused;
    }
  try {
    core.set_stops(sid + 1, {1}, {1}, 0);
  } catch (const std::invalid_argument&) {
    ++refused;
  }
  if (refused != 4) return fail("set_stops accepted a bad list", refused);
  core.reset();
  return 0;
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 50;
  for (int s = 0; s < n; ++s)
    if (int rc = run((unsigned)s)) {
      std::fprintf(stderr, "seed %d\n", s);
      return rc;
    }
  std::printf("ok %d workloads\n", n);
  return 0;
}
