// Sanitizer stress test of the prefix cache of the continuous-batching core
// (csrc/runtime/sched_core.h set_prefix_cache), run by
// tests/test_prefix_cache.py under AddressSanitizer + UBSan.
//
// Random workloads as in sched_fork_stress.cpp -- several replicas and groups,
// slot pools smaller than the demand, chunked prefill under a token budget,
// readouts 0-3 steps late, families -- whose prompts are one of three stems of
// 20-40 tokens plus a tail of 0-12, so that they share prefixes and repeat;
// some sequences opt out (no set_prompt), some insert without looking up.
// Small pools and small max_entries make hits, evictions and dropped matches
// frequent; every few runs end in a reset() or a clear_prefix_cache() with
// hits in flight.  A naive model keeps who owns which slot and checks at
// every step:
//   * free slots + entries + slots held by admitted sequences = capacity;
//   * no slot is both an entry and a sequence's; at most max_entries entries;
//   * a hit's source is an entry, pinned from the plan with its first chunk
//     until the read-back that brings the sequence's first token;
//   * m <= L - 1, m >= min_tokens, m is what the source's key gives, and m is
//     the brute-force best over the replica's entries (a miss: that best is 0)
//     in every plan that evicted nothing;
//   * a sequence that opted out of the lookup never hits;
//   * insert: no entry's key starts with the new entry's, and an entry whose
//     key the new one starts with is pinned;
//   * every sequence is released once, and reset() / clear_prefix_cache() give
//     every slot back.
// A last scenario: a pool of exactly 1 + k slots, all cached, still admits a
// family of 1 + k.
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <map>
#include <random>
#include <set>
#include <tuple>
#include <vector>

#include "../sched_core.h"

using namespace lsd_rt;

static int fail(const char* what, long long v) {
  std::fprintf(stderr, "FAIL: %s (%lld)\n", what, v);
  return 1;
}

struct Track {
  std::vector<int> prompt;
  bool opted = false, lookup = false;  // set_prompt was called; with lookup
  int64_t parent = -1;
  int rep = -1, slot = -1;  // from the first chunk on
  int src = -1;             // the entry it hit, until its first token is back
  bool admitted = false, first = false, released = false;
};

using Entries = std::vector<std::tuple<int, int, std::vector<int>>>;  // (slot, pins, key)

static int lcp(const std::vector<int>& a, const std::vector<int>& b) {
  size_t n = 0;
  while (n < a.size() && n < b.size() && a[n] == b[n]) ++n;
  return (int)n;
}

// the best m over `es` for `prompt`, 0 below min_tokens
static int brute(const Entries& es, const std::vector<int>& prompt, int min_tokens) {
  int best = 0;
  for (const auto& e : es) best = std::max(best, std::min(lcp(std::get<2>(e), prompt), (int)prompt.size() - 1));
  return best >= min_tokens ? best : 0;
}

static long g_hits = 0, g_evictions = 0, g_dropped = 0;

static int run(unsigned seed) {
  std::mt19937 rnd(seed);
  auto pick = [&](std::vector<int> v) { return v[rnd() % v.size()]; };
  const int R = pick({1, 2}), M = pick({1, 2, 3}), cap = pick({2, 3, 8});
  const int slots = pick({cap, cap + 1, cap * M});
  const int budget = pick({0, 5, 64}), chunk = pick({0, 3, 9});
  const int min_tokens = pick({1, 4, 16}), max_entries = pick({1, 2, slots});
  const bool collect = seed % 2 == 1;
  const int ending = seed % 7;  // 5: reset() at step 60, 6: clear_prefix_cache() at step 60, then on
  const int eos = 3;
  std::vector<SlotAllocator> pools;
  for (int r = 0; r < R; ++r) pools.emplace_back(slots);
  std::vector<SlotAllocator*> pp;
  for (auto& p : pools) pp.push_back(&p);
  SchedCore core(R, M, cap, budget, chunk, 4096, pp);
  core.set_prefix_cache(max_entries, min_tokens);
  if (seed % 3 == 0) core.set_join_policy(3, 2);
  std::vector<std::vector<int>> stems(3);
  for (auto& st : stems) {
    st.resize(20 + rnd() % 21);
    for (int& t : st) t = 20 + (int)(rnd() % 4);  // few distinct tokens: stems share heads now and then
  }
  std::map<int64_t, Track> seqs;
  std::map<std::pair<int, int>, int64_t> owner;  // (rep, slot) -> sid
  std::deque<std::tuple<int64_t, int, int, int>> pending;  // step, rep, g, n
  std::vector<std::vector<int>> recent;
  int64_t sid = 0;
  long held = 0;  // admitted, not released
  auto check_slots = [&]() -> int {
    long free_ = 0, cached = 0;
    for (int rep = 0; rep < R; ++rep) {
      const Entries es = core.prefix_entries(rep);
      if ((int)es.size() > max_entries) return fail("more than max_entries entries", (long long)es.size());
      free_ += pools[rep].available();
      cached += (long)es.size();
      for (const auto& e : es)
        if (owner.count({rep, std::get<0>(e)})) return fail("a slot is an entry and a sequence's", std::get<0>(e));
    }
    if (free_ + cached + held != (long)R * slots) return fail("free + cached + held != capacity", free_ + cached + held);
    if (std::get<0>(core.prefix_cache_stats()) != cached) return fail("the entries counter is off", cached);
    return 0;
  };
  auto readout = [&](int64_t st, int rep, int g, int n, bool random_tokens) -> int {
    std::vector<int> toks(n);
    for (int& t : toks) t = random_tokens ? pick({eos, 11, 12, 13}) : 11;
    std::vector<std::set<int>> before(R);
    for (int r = 0; r < R; ++r)
      for (const auto& e : core.prefix_entries(r)) before[r].insert(std::get<0>(e));
    std::vector<Event> ev;
    if (collect) {
      std::vector<int32_t> t32(toks.begin(), toks.end());
      ev = core.assign_collect(rep, st, g, t32.data(), n, eos).first;
    } else {
      ev = core.assign(rep, st, g, toks, eos);
    }
    for (const auto& e : ev) {
      Track& t = seqs.at(std::get<0>(e));
      if (std::get<2>(e) & EV_FIRST) {
        t.first = true;
        t.src = -1;  // the pin is back
      }
      if (std::get<2>(e) & EV_RELEASE) {
        if (t.released) return fail("released twice", std::get<0>(e));
        t.released = true;
        --held;
        if (t.slot >= 0) {
          auto it = owner.find({t.rep, t.slot});
          if (it == owner.end() || it->second != std::get<0>(e)) return fail("released a slot it does not own", t.slot);
          owner.erase(it);
        }
      }
    }
    // the entries this read-back inserted, against the dedup rules
    for (int r = 0; r < R; ++r) {
      const Entries es = core.prefix_entries(r);
      for (const auto& e : es) {
        if (before[r].count(std::get<0>(e))) continue;
        const auto& key = std::get<2>(e);
        if ((int)key.size() < min_tokens) return fail("an entry shorter than min_tokens", (long long)key.size());
        for (const auto& o : es) {
          if (std::get<0>(o) == std::get<0>(e)) continue;
          const auto& ok = std::get<2>(o);
          const int c = lcp(key, ok);
          if (c == (int)key.size()) return fail("an entry's key starts with the new entry's", std::get<0>(o));
          if (c == (int)ok.size() && std::get<1>(o) == 0)
            return fail("the new entry's key starts with an unpinned entry's", std::get<0>(o));
        }
      }
    }
    return check_slots();
  };
  for (int64_t step = 0; step < 20000; ++step) {
    if (step < 160 && rnd() % 10 < 3) {
      const int reqs = 1 + rnd() % 3;
      for (int q = 0; q < reqs; ++q) {
        const int top = std::min({cap, slots, 4});
        const int n = (rnd() % 4 == 0 && top >= 2) ? 2 + (int)(rnd() % (top - 1)) : 1;
        std::vector<int> prompt;
        if (!recent.empty() && rnd() % 4 == 0) {
          prompt = recent[rnd() % recent.size()];  // a duplicate
        } else if (rnd() % 12 == 0) {
          prompt.assign(1, 25);  // a one-token prompt
        } else {
          prompt = stems[rnd() % 3];
          if (rnd() % 5 == 0) prompt.resize(1 + rnd() % prompt.size());
          for (int k = rnd() % 13; k > 0; --k) prompt.push_back(30 + (int)(rnd() % 3));
        }
        recent.push_back(prompt);
        const bool stop = rnd() % 2;
        const int64_t par = sid++;
        core.add(par, (int)prompt.size(), pick({1, 1, 3, 20}), stop);
        Track& tp = seqs[par];
        tp.prompt = prompt;
        const int mode = rnd() % 6;  // 0: opted out, 1: inserts only, else both
        std::vector<int64_t> fam;
        for (int i = 1; i < n; ++i) {
          const int64_t f = sid++;
          if (i % 2) core.add_fork(f, par, pick({1, 2, 9}), stop);  // ahead of set_prompt, and behind it
          else fam.push_back(f);
          seqs[f].prompt = prompt;
          seqs[f].parent = prompt.size() > 1 ? par : -1;
        }
        if (mode) {
          core.set_prompt(par, prompt, mode != 1);
          seqs[par].opted = true;
          seqs[par].lookup = mode != 1;
        }
        for (int64_t f : fam) core.add_fork(f, par, pick({1, 2, 9}), stop);
      }
    }
    if (!core.has_work()) {
      if (step >= 160) break;
      continue;
    }
    if (step == 60 && ending == 5) {
      core.reset();
      for (auto& p : pools)
        if (p.available() != slots) return fail("reset leaked a slot", p.available());
      if (core.has_work() || core.n_expect() != 0) return fail("work left after reset", step);
      if (std::get<0>(core.prefix_cache_stats()) != 0) return fail("entries left after reset", step);
      return 0;
    }
    if (step == 60 && ending == 6) {
      core.clear_prefix_cache();
      for (int r = 0; r < R; ++r)
        for (const auto& e : core.prefix_entries(r))
          if (std::get<1>(e) == 0) return fail("an unpinned entry survived clear_prefix_cache", std::get<0>(e));
      if (int rc = check_slots()) return rc;
    }
    std::vector<Entries> snap(R);
    for (int r = 0; r < R; ++r) snap[r] = core.prefix_entries(r);
    const auto stats0 = core.prefix_cache_stats();
    std::vector<int64_t> admitted;
    auto plans = core.plan(step, &admitted);
    const auto stats1 = core.prefix_cache_stats();
    const bool evicted = std::get<4>(stats1) != std::get<4>(stats0);
    g_evictions += (long)(std::get<4>(stats1) - std::get<4>(stats0));
    std::set<int64_t> now(admitted.begin(), admitted.end());
    for (int64_t s : admitted) {
      if (seqs.at(s).admitted) return fail("admitted twice", s);
      seqs.at(s).admitted = true;
      ++held;
    }
    std::map<int64_t, int> hit_m;
    for (const auto& h : core.hits()) hit_m[h.first] = h.second;
    std::map<int64_t, int> fork_src;
    for (const auto& f : core.forks()) fork_src[f.first] = f.second;
    size_t hits_seen = 0;
    for (int rep = 0; rep < R; ++rep)
      for (const auto& go : plans[rep]) {
        const int g = std::get<0>(go), ret = std::get<1>(go);
        for (const auto& c : std::get<6>(go)) {
          const int64_t s = std::get<0>(c);
          const int slot = std::get<1>(c), start = std::get<2>(c);
          Track& t = seqs.at(s);
          const bool opens = t.slot < 0;
          if (opens) {
            if (owner.count({rep, slot})) return fail("a slot has two owners", slot);
            owner[{rep, slot}] = s;
            t.rep = rep;
            t.slot = slot;
          } else if (t.rep != rep || t.slot != slot) {
            return fail("a sequence changed its slot", s);
          }
          if (!opens) continue;
          const int L = (int)t.prompt.size();
          if (t.parent >= 0) {
            if (hit_m.count(s)) return fail("a family fork among the hits", s);
            continue;
          }
          const bool hit = hit_m.count(s) != 0;
          if (!hit && start != 0) return fail("a first chunk past 0 that is no hit", s);
          if (hit) {
            ++hits_seen;
            ++g_hits;
            const int m = hit_m[s];
            if (!t.opted || !t.lookup) return fail("a sequence that does not look up hit", s);
            if (m != start || m > L - 1 || m < min_tokens) return fail("m outside [min_tokens, L - 1] or not the start", m);
            if (!fork_src.count(s)) return fail("a hit that forks() does not list", s);
            t.src = fork_src[s];
            bool found = false;
            for (const auto& e : core.prefix_entries(rep))
              if (std::get<0>(e) == t.src) {
                found = true;
                if (std::get<1>(e) <= 0) return fail("a hit's source is not pinned", t.src);
                if (std::min(lcp(std::get<2>(e), t.prompt), L - 1) != hit_m[s])
                  return fail("m is not what the source's key gives", hit_m[s]);
              }
            if (!found) return fail("a hit's source is no entry", t.src);
            if (owner.count({rep, t.src})) return fail("a hit's source is a sequence's slot", t.src);
          }
          // the lookup ran in this plan and nothing was evicted in it: the snapshot is what it saw
          if (now.count(s) && !evicted) {
            const int want = t.opted && t.lookup ? brute(snap[rep], t.prompt, min_tokens) : 0;
            if ((hit ? hit_m[s] : 0) != want) return fail("m is not the brute-force best", want);
          } else if (now.count(s) && !hit && t.opted && t.lookup && brute(snap[rep], t.prompt, min_tokens) > 0) {
            ++g_dropped;  // a match that evictions took away, or that was dropped for the family to fit
          }
        }
        if (ret) pending.emplace_back(step, rep, g, ret);
      }
    if (hits_seen != core.hits().size()) return fail("hits() lists a chunk the plan does not hold", step);
    // every hit whose first token is not back yet still pins its entry
    for (const auto& kv : seqs) {
      const Track& t = kv.second;
      if (t.src < 0 || t.released) continue;
      bool pinned = false;
      for (const auto& e : core.prefix_entries(t.rep))
        if (std::get<0>(e) == t.src && std::get<1>(e) > 0) pinned = true;
      if (!pinned) return fail("an entry lost its pin before the hit's first token", kv.first);
    }
    if (int rc = check_slots()) return rc;
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
  for (int r = 0; r < R; ++r)
    for (const auto& e : core.prefix_entries(r))
      if (std::get<1>(e) != 0) return fail("a pin outlived every sequence", std::get<0>(e));
  if (seed % 2) core.clear_prefix_cache();
  else core.reset();
  for (auto& p : pools)
    if (p.available() != slots) return fail("slot leak", p.available());
  return 0;
}

// k + 1 slots, every one an entry: a family of 1 + k whose prompt matches one
// of them is still admitted (the match is dropped, every entry evicted).
static int all_cached(int k) {
  SlotAllocator pool(1 + k);
  SchedCore core(1, 1, 1 + k, 0, 0, 4096, {&pool});
  core.set_prefix_cache(1 + k, 4);
  int64_t step = 0;
  auto drain = [&]() {
    while (core.has_work() || core.n_expect()) {
      auto plans = core.plan(step, nullptr);
      for (const auto& go : plans[0])
        if (std::get<1>(go)) core.assign(0, step, std::get<0>(go), std::vector<int>(std::get<1>(go), 11), 3);
      ++step;
    }
  };
  for (int i = 0; i <= k; ++i) {
    std::vector<int> p(8, 40 + i);
    core.add(i, 8, 1, false);
    core.set_prompt(i, p);
  }
  drain();
  if (pool.available() != 0 || std::get<0>(core.prefix_cache_stats()) != 1 + k) return fail("not every slot is cached", pool.available());
  std::vector<int> p(8, 40);
  p.push_back(9);
  core.add(100, 9, 1, false);
  for (int i = 1; i <= k; ++i) core.add_fork(100 + i, 100, 1, false);
  core.set_prompt(100, p);
  std::vector<int64_t> admitted;
  core.plan(step++, &admitted);
  if ((int)admitted.size() != 1 + k) return fail("the family was not admitted", (long long)admitted.size());
  if (k > 0 && !core.hits().empty()) return fail("a match that left no room was kept", k);
  drain();
  core.clear_prefix_cache();
  if (pool.available() != 1 + k) return fail("slot leak", pool.available());
  return 0;
}

int main(int argc, char** argv) {
  const int runs = argc > 1 ? std::atoi(argv[1]) : 16;
  for (int s = 0; s < runs; ++s)
    if (int rc = run(4321u + (unsigned)s)) {
      std::fprintf(stderr, "seed %d failed\n", s);
      return rc;
    }
  for (int k : {0, 1, 3})
    if (int rc = all_cached(k)) return rc;
  if (g_hits <= 0 || g_evictions <= 0) return fail("no hit or no eviction was ever seen", g_hits);
  std::printf("ok %d (%ld hits, %ld evictions, %ld dropped matches)\n", runs, g_hits, g_evictions, g_dropped);
  return 0;
}
