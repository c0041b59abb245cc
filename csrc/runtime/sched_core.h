// Iteration-level (continuous-batching) scheduler core, pure C++17.
//
// The state machine behind runtime/scheduler.py. The Python `Scheduler`
// keeps the request futures, the sampling parameters and the GPU readout
// events; this core owns everything that changes at every decode step:
//   * sequences: slot, prefill progress, issued tokens, decode position,
//     sampler counter;
//   * per microbatch group: its decode rows, the sequences still
//     prefilling, and the composition of its last token-producing item;
//   * admission: a FIFO into free slots of the replica's SlotAllocator,
//     capped by the group capacity;
//   * planning: one step's group plans, i.e. leaves, joins, prefill chunks
//     under the token budget, decode rows, power-of-two row bucket and
//     256-position context bucket;
//   * readout assignment: sampled ids -> per-sequence events, EOS stop,
//     per-request stop sequences, and slot release at a sequence's last item;
//   * families (add_fork): further samples of one prompt, admitted with their
//     parent and started from a copy of its KV instead of a prefill;
//   * the prefix cache (set_prefix_cache): slots that finished requests left,
//     keyed by their prompts, which later prompts start their prefill behind.
// The reference has no scheduler at all. Its coordinator runs one request's
// token loop per HTTP call (`server.py:154-206`); see SURVEY.md §5.2.
//
// Semantics are identical to the Python twin (`_PyCore` in
// runtime/scheduler.py); tests/test_sched_core.py drives both with the same
// random workloads and compares every plan and event.
#pragma once

#include <algorithm>
#include <cstdint>
#include <deque>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

namespace lsd_rt {

// The free list the core allocates KV slots from (runtime.cpp binds the same
// class to Python as SlotAllocator).
class SlotAllocator {
 public:
  explicit SlotAllocator(int n) : cap_(n), used_(n, false) {
    for (int i = n - 1; i >= 0; --i) free_.push_back(i);
  }
  std::vector<int> alloc(int k) {
    if (k > (int)free_.size())
      throw std::runtime_error("out of KV slots: want " + std::to_string(k) + ", have " +
                               std::to_string(free_.size()));
    std::vector<int> out;
    out.reserve(k);
    for (int i = 0; i < k; ++i) {
      const int s = free_.back();
      free_.pop_back();
      used_[s] = true;
      out.push_back(s);
    }
    return out;
  }
  void free(const std::vector<int>& slots) {
    for (int s : slots) {
      if (s < 0 || s >= cap_ || !used_[s])
        throw std::runtime_error("double free / bad slot " + std::to_string(s));
      used_[s] = false;
      free_.push_back(s);
    }
  }
  int available() const { return (int)free_.size(); }
  int capacity() const { return cap_; }

 private:
  int cap_;
  std::vector<bool> used_;
  std::vector<int> free_;
};

// (sid, slot, start, len, final)
using ChunkOut = std::tuple<int64_t, int, int, int, bool>;
// (sid, slot, pos, sstep, src): src = index of the row's last token in the
// previous token-return vector of this group
using RowOut = std::tuple<int64_t, int, int, int, int>;
// (g, ret, n, b, ctxb, rows_changed, chunks, rows)
using GroupOut = std::tuple<int, int, int, int, int, bool, std::vector<ChunkOut>, std::vector<RowOut>>;
// (sid, token, flags): FIRST = first token of the sequence, FINISH = the
// request is complete now, RELEASE = its slot went back to the pool (token -1),
// STOP (beside FINISH) = the token completed one of the request's stop sequences
using Event = std::tuple<int64_t, int, int>;
constexpr int EV_FIRST = 1, EV_FINISH = 2, EV_RELEASE = 4, EV_STOP = 8;
constexpr int MAX_STOP_LEN = 32;  // tokens of the longest stop sequence, and of the tail kept for matching

class SchedCore {
 public:
  SchedCore(int replicas, int groups, int cap, int64_t prefill_budget, int chunk, int max_seq,
            std::vector<SlotAllocator*> pools)
      : R_(replicas), M_(groups), cap_(cap), budget_(prefill_budget), chunk_(chunk),
        max_seq_(max_seq), pools_(std::move(pools)),
        groups_(replicas, std::vector<Group>(groups)), caches_(replicas) {
    if ((int)pools_.size() != R_) throw std::invalid_argument("one slot pool per replica");
  }

  void add(int64_t sid, int prompt_len, int want, bool stop_at_eos) {
    if (prompt_len <= 0) throw std::invalid_argument("empty prompt");
    Seq s;
    s.prompt_len = prompt_len;
    s.want = want;
    s.stop_at_eos = stop_at_eos;
    seqs_[sid] = s;
    waiting_.push_back(sid);
  }

  // add() of a whole batch (one call from the scheduler's bulk admission)
  void add_many(const std::vector<int64_t>& sids, const std::vector<int>& prompt_lens,
                const std::vector<int>& wants, const std::vector<bool>& stops) {
    const size_t n = sids.size();
    if (prompt_lens.size() != n || wants.size() != n || stops.size() != n)
      throw std::invalid_argument("add_many: length mismatch");
    for (size_t i = 0; i < n; ++i)
      if (prompt_lens[i] <= 0) throw std::invalid_argument("empty prompt");
    for (size_t i = 0; i < n; ++i) add(sids[i], prompt_lens[i], wants[i], stops[i]);
  }

  // A further sample of `parent`'s prompt (SamplingParams.n): a *fork*.  The
  // parent must be known and still waiting.  The fork takes its prompt length
  // and joins its family:
  //   1. a family is admitted as a unit -- the head of the waiting queue with
  //      k forks is taken only by a group with room for 1 + k sequences while
  //      the pool has 1 + k free slots; otherwise admission stops there.  The
  //      forks sit in the group's prefilling list from then on;
  //   2. in the step after the one that planned the parent's final chunk every
  //      fork gets its one chunk (sid, slot, L - 1, 1, final) in the parent's
  //      group, ahead of the group's other chunks; it counts against the
  //      prefill budget and is never stopped by it.  forks() names the slot to
  //      copy positions [0, L - 1) from: the parent's;
  //   3. the parent keeps its slot past that step: a sequence's slot goes back
  //      with the read-back of the last item that held its decode row, and
  //      the parent's first decode row is in the forks' item at the earliest
  //      (a want = 1 parent included: its first row is issued and discarded).
  // A prompt of one token has nothing to copy: the fork is a plain add().
  void add_fork(int64_t sid, int64_t parent, int want, bool stop_at_eos) {
    auto it = seqs_.find(parent);
    if (it == seqs_.end()) throw std::invalid_argument("add_fork: unknown parent");
    if (it->second.slot >= 0 || it->second.g >= 0 || it->second.parent >= 0)
      throw std::invalid_argument("add_fork: the parent is admitted already, or is a fork itself");
    if (seqs_.count(sid)) throw std::invalid_argument("add_fork: the sequence exists already");
    const int L = it->second.prompt_len;
    if (L == 1) {
      add(sid, 1, want, stop_at_eos);
      seqs_.at(sid).prompt = seqs_.at(parent).prompt;
      return;
    }
    Seq s;
    s.prompt_len = L;
    s.want = want;
    s.stop_at_eos = stop_at_eos;
    s.parent = parent;
    s.prompt = it->second.prompt;
    seqs_[sid] = s;
    seqs_.at(parent).forks.push_back(sid);
  }

  // (sid, source slot) of the chunks of the last plan() that start behind a
  // copy of another slot's KV, in plan order: the families' fork chunks, and
  // the first chunk of every sequence that hit the prefix cache
  const std::vector<std::pair<int64_t, int>>& forks() const { return forks_; }

  // The prefix cache.  An *entry* is a KV slot that a finished sequence left,
  // valid for positions [0, L) of that sequence's prompt -- its key; the slot
  // stays taken from the pool.  Off (max_entries 0) nothing below happens.
  //   insert: when a sequence with a prompt (set_prompt) gives its slot back
  //     (release) the slot becomes an entry instead, at no copy.  A prompt
  //     shorter than min_tokens can never be matched: its slot is freed.  If an
  //     entry's key starts with the new key the new slot is freed (and the
  //     entry counts as used now); every unpinned entry whose key the new key
  //     starts with is freed.  At most max_entries per replica: the least
  //     recently used unpinned entry goes first (with every entry pinned the
  //     new slot is freed instead);
  //   lookup: at admission, for a sequence whose set_prompt asked for it, over
  //     the entries of the admitting replica that share the prompt's first
  //     min_tokens tokens (one hash lookup finds them).  c = the longest
  //     common prefix with an entry's key, m = min(c, L - 1) -- one token is
  //     always forwarded, to take draw 0 -- the largest m wins, ties go to the
  //     most recently used entry, and m >= min_tokens is a hit;
  //   hit: the sequence starts with prefilled = m; its first chunk
  //     (sid, slot, m, len, final?) is reported by forks() with the entry's
  //     slot, and by hits() with m; chunk length and budget apply to the tail;
  //   pin: the entry is pinned from the admission until the hitting
  //     sequence's first token has been read back (EV_FIRST): the item that
  //     drew it ran behind the copy on the same lane.  A pinned entry is never
  //     evicted and never handed out;
  //   evict: an admission that needs 1 + k slots while the pool is short gives
  //     least recently used unpinned entries back to the pool, never the one
  //     just matched -- unless the family cannot fit beside it: then the match
  //     is dropped (a miss) and that entry may go too.  Nothing is evicted for
  //     a family that would not fit even so.
  // free slots + entries + slots held by sequences = the pool's capacity.
  void set_prefix_cache(int max_entries, int min_tokens) {
    if (max_entries < 0 || min_tokens < 1) throw std::invalid_argument("set_prefix_cache: max_entries >= 0, min_tokens >= 1");
    clear_prefix_cache();
    for (const auto& c : caches_)
      if (!c.entries.empty()) throw std::runtime_error("set_prefix_cache: entries are pinned by sequences in flight");
    pc_max_ = max_entries;
    pc_min_ = min_tokens;
  }

  // The prompt of a sequence that was added and is not admitted yet (its forks
  // share it): the sequence leaves an entry behind, and with `lookup` it may
  // start from one.  The core holds no token ids otherwise.
  void set_prompt(int64_t sid, const std::vector<int>& tokens, bool lookup = true) {
    auto it = seqs_.find(sid);
    if (it == seqs_.end()) throw std::invalid_argument("set_prompt: unknown sequence");
    Seq& s = it->second;
    if (s.slot >= 0 || s.g >= 0) throw std::invalid_argument("set_prompt: the sequence is admitted already");
    if ((int)tokens.size() != s.prompt_len) throw std::invalid_argument("set_prompt: not prompt_len tokens");
    s.prompt = std::make_shared<const std::vector<int>>(tokens);
    s.lookup = lookup;
    for (int64_t fid : s.forks) seqs_.at(fid).prompt = s.prompt;
  }

  // (sid, m) of the prefix-cache hits among forks(), in plan order
  const std::vector<std::pair<int64_t, int>>& hits() const { return hits_; }

  // (entries, hits, misses, tokens reused, evictions)
  std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t> prefix_cache_stats() const {
    int64_t n = 0;
    for (const auto& c : caches_) n += (int64_t)c.entries.size();
    return {n, pc_hits_, pc_misses_, pc_tokens_, pc_evictions_};
  }

  // (slot, pins, key) of replica rep's entries, by slot (tests, debugging)
  std::vector<std::tuple<int, int, std::vector<int>>> prefix_entries(int rep) const {
    std::vector<std::tuple<int, int, std::vector<int>>> out;
    for (const auto& kv : caches_.at(rep).entries) out.emplace_back(kv.first, kv.second.pins, kv.second.toks);
    return out;
  }

  // Free the unpinned entries.
  void clear_prefix_cache() {
    for (int rep = 0; rep < R_; ++rep) {
      std::vector<int> go;
      for (const auto& kv : caches_[rep].entries)
        if (kv.second.pins == 0) go.push_back(kv.first);
      for (int slot : go) drop_entry(rep, slot);
    }
  }

  // Stop sequences of a sequence that was added and has no token yet:
  // lengths[e] tokens of flat_tokens each, tried in this order.  After its
  // j-th generated token is read back (the prefill draw is token 1) a stop
  // sequence matches when it equals the last len generated tokens -- the
  // prompt never takes part -- and the match counts when j > min_tokens; the
  // first counting match ends the sequence as a read-back EOS does.
  void set_stops(int64_t sid, const std::vector<int>& flat_tokens, const std::vector<int>& lengths,
                 int min_tokens) {
    auto it = seqs_.find(sid);
    if (it == seqs_.end()) throw std::invalid_argument("set_stops: unknown sequence");
    if (it->second.ntok > 0) throw std::invalid_argument("set_stops: the sequence has tokens already");
    size_t total = 0;
    for (int n : lengths) {
      if (n < 1 || n > MAX_STOP_LEN) throw std::invalid_argument("set_stops: a stop sequence holds 1 to 32 tokens");
      total += (size_t)n;
    }
    if (total != flat_tokens.size()) throw std::invalid_argument("set_stops: lengths do not add up to the tokens");
    if (lengths.empty()) {
      it->second.stops.reset();
      return;
    }
    auto st = std::make_shared<Stops>();
    st->toks = flat_tokens;
    st->lens = lengths;
    st->min_tokens = min_tokens;
    it->second.stops = std::move(st);
  }

  bool has_work() const {
    if (!waiting_.empty()) return true;
    for (const auto& rep : groups_)
      for (const auto& g : rep)
        if (!g.rows.empty() || !g.prefilling.empty() || g.prev >= 0) return true;
    return false;
  }

  // Group plans of step `step` for every replica (groups with nothing to do
  // and nothing to read back are omitted); `admitted` gets the sequences
  // that joined at this step.
  std::vector<std::vector<GroupOut>> plan(int64_t step, std::vector<int64_t>* admitted) {
    std::vector<std::vector<GroupOut>> out(R_);
    forks_.clear();
    hits_.clear();
    for (int rep = 0; rep < R_; ++rep)
      for (int g = 0; g < M_; ++g) {
        GroupOut go;
        if (group_plan(rep, g, step, &go, admitted)) out[rep].push_back(std::move(go));
      }
    ++steps_;
    return out;
  }

  // Token readout of the item (rep, step, g): tokens = [decode rows | finals].
  std::vector<Event> assign(int rep, int64_t step, int g, const std::vector<int>& tokens, int eos) {
    auto it = expect_.find(key(rep, step, g));
    if (it == expect_.end()) throw std::runtime_error("no item awaiting this readout");
    const Produced prod = std::move(it->second);
    expect_.erase(it);
    std::vector<Event> ev;
    for (size_t i = 0; i < prod.rows.size(); ++i) give(prod.rows[i], tokens.at(i), eos, &ev);
    for (size_t j = 0; j < prod.finals.size(); ++j)
      give(prod.finals[j], tokens.at(prod.b + j), eos, &ev);
    for (int64_t sid : prod.release) release(sid, &ev);
    return ev;
  }

  // assign() for the serving hot path: each sequence's tokens are kept here,
  // and only FIRST / FINISH / RELEASE events come back (a plain token of a
  // running sequence costs the caller nothing), plus the whole token list of
  // every sequence that finished in this readout.  tokens points at n int32
  // ids (the pinned host copy of the token-return vector).
  using Finished = std::vector<std::pair<int64_t, std::vector<int>>>;
  std::pair<std::vector<Event>, Finished> assign_collect(int rep, int64_t step, int g,
                                                         const int32_t* tokens, int n, int eos) {
    auto it = expect_.find(key(rep, step, g));
    if (it == expect_.end()) throw std::runtime_error("no item awaiting this readout");
    const Produced prod = std::move(it->second);
    expect_.erase(it);
    auto tok_at = [&](size_t i) {
      if ((int)i >= n) throw std::out_of_range("token-return vector shorter than the item's rows");
      return (int)tokens[i];
    };
    std::vector<Event> ev;
    Finished done;
    for (size_t i = 0; i < prod.rows.size(); ++i) give_collect(prod.rows[i], tok_at(i), eos, &ev, &done);
    for (size_t j = 0; j < prod.finals.size(); ++j)
      give_collect(prod.finals[j], tok_at(prod.b + j), eos, &ev, &done);
    for (int64_t sid : prod.release) {
      auto f = seqs_.find(sid);
      if (f != seqs_.end() && !f->second.finished) done.emplace_back(sid, f->second.toks);
      release(sid, &ev);
    }
    return {std::move(ev), std::move(done)};
  }

  // Drop every sequence and give their slots back (failure path).
  void reset() {
    for (auto& kv : seqs_)
      if (kv.second.slot >= 0) pools_[kv.second.rep]->free({kv.second.slot});
    for (int rep = 0; rep < R_; ++rep) {  // every entry, the pinned ones too: their sequences are gone
      for (const auto& kv : caches_[rep].entries) pools_[rep]->free({kv.first});
      caches_[rep] = Cache();
    }
    seqs_.clear();
    waiting_.clear();
    expect_.clear();
    produced_.clear();
    forks_.clear();
    hits_.clear();
    groups_.assign(R_, std::vector<Group>(M_));
  }

  // Join policy: a group admits waiting requests only when it has room for
  // all of them or for `join_min` of them, when it is idle, or after it has
  // deferred `max_wait` steps in a row -- so a running batch takes its
  // joiners in larger prefill items, fewer weight passes per generated token
  // (join_min 1: admit whatever fits at every step).
  void set_join_policy(int join_min, int max_wait) {
    if (join_min < 1 || max_wait < 0) throw std::invalid_argument("join_min >= 1, max_wait >= 0");
    join_min_ = join_min;
    max_wait_ = max_wait;
  }
  int64_t deferred() const { return deferred_; }

  int64_t joins() const { return joins_; }
  int64_t leaves() const { return leaves_; }
  int max_rows() const { return max_rows_; }
  int64_t steps() const { return steps_; }
  int n_waiting() const { return (int)waiting_.size(); }
  int n_seqs() const { return (int)seqs_.size(); }
  int n_expect() const { return (int)expect_.size(); }

 private:
  // stop sequences of a request that gave some, and the last generated tokens
  // they are matched against (sequences without stops keep neither)
  struct Stops {
    std::vector<int> toks, lens;
    int min_tokens = 0;
    int tail[MAX_STOP_LEN];  // the last min(ntok, 32) generated tokens, oldest first
    int ntail = 0;
  };
  struct Seq {
    int rep = 0, g = -1, slot = -1;
    int prompt_len = 0, prefilled = 0, issued = 0, pos = 0, sstep = 1;
    int want = 0, ntok = 0;
    bool stop_at_eos = false, stop = false, finished = false;
    std::vector<int> toks;  // assign_collect only
    std::shared_ptr<Stops> stops;  // null without stop sequences
    // families: a fork's parent (-1: none) and the slot its KV is copied from;
    // ready once the parent's final chunk has been planned.  forks: the fork ids
    // of a parent whose final chunk is not planned yet, cleared when it is
    int64_t parent = -1;
    int src_slot = -1;
    bool ready = false;
    std::vector<int64_t> forks;
    // prefix cache: the prompt's ids (null: the sequence opted out), whether it
    // looks an entry up at admission, and of a hit the entry's slot (pinned
    // until this sequence's first token) and whether its first chunk is still
    // to be planned
    std::shared_ptr<const std::vector<int>> prompt;
    bool lookup = false, hit_new = false;
    int hit_slot = -1;
  };
  struct Entry {
    std::vector<int> toks;
    int pins = 0;
    int64_t used = 0;  // tick of the insert or of the last hit
  };
  // one replica's entries by slot, and the slots by the hash of their keys'
  // first min_tokens tokens
  struct Cache {
    std::map<int, Entry> entries;
    std::unordered_map<uint64_t, std::vector<int>> index;
  };
  struct Produced {
    int b = 0;
    std::vector<int64_t> rows, finals, release;
  };
  struct Group {
    std::vector<int64_t> rows, prefilling;
    // rows' Seq entries (node-based map: stable until a sequence is erased,
    // which happens only after it left its group), so the steady-state step
    // touches each row through a pointer instead of three hash lookups
    std::vector<Seq*> rowp;
    int64_t prev = -1;  // produced_ id of the last token-producing item
    int waited = 0;     // consecutive steps this group deferred its joins
  };

  static std::tuple<int, int64_t, int> key(int rep, int64_t step, int g) { return {rep, step, g}; }

  static int bucket(int n, int cap) {
    if (n <= 0) return 0;
    int b = 1;
    while (b < n) b <<= 1;
    return std::min(b, cap);
  }

  bool join_ok(Group& gh, int room, bool idle) {
    if (waiting_.empty() || room <= 0) {
      gh.waited = 0;
      return false;
    }
    if (idle || room >= std::min<int64_t>(join_min_, (int64_t)waiting_.size()) || gh.waited >= max_wait_) {
      gh.waited = 0;
      return true;
    }
    ++gh.waited;
    ++deferred_;
    return false;
  }

  std::vector<int64_t> admit(int rep, int g, int room, std::vector<int64_t>* admitted) {
    SlotAllocator* pool = pools_[rep];
    std::vector<int64_t> out;
    while (!waiting_.empty() && room > 0 && pool->available() + (int)caches_[rep].entries.size() > 0) {
      const int64_t sid = waiting_.front();
      Seq& s = seqs_.at(sid);
      const int k = (int)s.forks.size();
      if (room < 1 + k) break;  // a family is admitted as a unit
      int src = -1, m = 0;
      if (pc_max_ > 0) {
        if (s.lookup && s.prompt) m = lookup(rep, *s.prompt, &src);
        if (pool->available() < 1 + k) {
          // the slots that evictions could add: every unpinned entry but the match
          int spare = 0;
          for (const auto& kv : caches_[rep].entries) spare += kv.second.pins == 0 && kv.first != src;
          if (src >= 0 && pool->available() + spare < 1 + k && caches_[rep].entries.at(src).pins == 0) {
            src = -1;  // the family does not fit beside the entry it matched: a miss
            m = 0;
            spare += 1;
          }
          if (pool->available() + spare < 1 + k) break;
          while (pool->available() < 1 + k) evict_lru(rep, src);
        }
        if (s.lookup && s.prompt) {
          if (src >= 0) {
            Entry& e = caches_[rep].entries.at(src);
            e.pins += 1;
            e.used = ++pc_tick_;
            s.hit_slot = src;
            s.hit_new = true;
            s.prefilled = m;
            pc_hits_ += 1;
            pc_tokens_ += m;
          } else {
            pc_misses_ += 1;
          }
        }
      } else if (pool->available() < 1 + k) {
        break;
      }
      waiting_.pop_front();
      s.rep = rep;
      s.g = g;
      s.slot = pool->alloc(1)[0];
      out.push_back(sid);
      if (admitted) admitted->push_back(sid);
      for (int64_t fid : s.forks) {
        Seq& f = seqs_.at(fid);
        f.rep = rep;
        f.g = g;
        f.slot = pool->alloc(1)[0];
        f.src_slot = s.slot;
        f.prefilled = f.prompt_len - 1;
        out.push_back(fid);
        if (admitted) admitted->push_back(fid);
      }
      room -= 1 + k;
      joins_ += 1 + k;
    }
    return out;
  }

  // FNV-1a over the first pc_min_ tokens (the caller made sure they exist)
  uint64_t head_hash(const std::vector<int>& toks) const {
    uint64_t h = 1469598103934665603ull;
    for (int i = 0; i < pc_min_; ++i) {
      h ^= (uint64_t)(uint32_t)toks[i];
      h *= 1099511628211ull;
    }
    return h;
  }

  // The best entry of replica rep for `toks`: -> m (0: none), *src its slot.
  int lookup(int rep, const std::vector<int>& toks, int* src) const {
    const int L = (int)toks.size();
    *src = -1;
    if (L - 1 < pc_min_) return 0;
    const Cache& c = caches_[rep];
    const auto b = c.index.find(head_hash(toks));
    if (b == c.index.end()) return 0;
    int best = 0;
    int64_t best_used = -1;
    for (int slot : b->second) {
      const Entry& e = c.entries.at(slot);
      const int n = std::min(L, (int)e.toks.size());
      int cp = 0;
      while (cp < n && e.toks[cp] == toks[cp]) ++cp;
      const int m = std::min(cp, L - 1);
      if (m < pc_min_) continue;
      if (m > best || (m == best && e.used > best_used)) {
        best = m;
        best_used = e.used;
        *src = slot;
      }
    }
    return best;
  }

  void drop_entry(int rep, int slot) {
    Cache& c = caches_[rep];
    const auto it = c.entries.find(slot);
    const uint64_t h = head_hash(it->second.toks);
    auto& b = c.index.at(h);
    b.erase(std::find(b.begin(), b.end(), slot));
    if (b.empty()) c.index.erase(h);
    c.entries.erase(it);
    pools_[rep]->free({slot});
  }

  // Give the least recently used unpinned entry other than `keep` back to the
  // pool (the caller made sure there is one).
  void evict_lru(int rep, int keep) {
    int slot = -1;
    int64_t used = 0;
    for (const auto& kv : caches_[rep].entries)
      if (kv.second.pins == 0 && kv.first != keep && (slot < 0 || kv.second.used < used)) {
        slot = kv.first;
        used = kv.second.used;
      }
    if (slot < 0) throw std::logic_error("prefix cache: no entry to evict");
    drop_entry(rep, slot);
    pc_evictions_ += 1;
  }

  // A released slot whose sequence had a prompt: an entry, or back to the pool.
  void insert_entry(int rep, int slot, const std::vector<int>& toks) {
    Cache& c = caches_[rep];
    const int L = (int)toks.size();
    if (L < pc_min_) {
      pools_[rep]->free({slot});
      return;
    }
    const uint64_t h = head_hash(toks);
    const auto b = c.index.find(h);
    if (b != c.index.end()) {
      std::vector<int> covered;
      for (int other : b->second) {
        Entry& e = c.entries.at(other);
        const int n = (int)e.toks.size();
        if (n >= L && std::equal(toks.begin(), toks.end(), e.toks.begin())) {
          e.used = ++pc_tick_;  // the entry covers the new key
          pools_[rep]->free({slot});
          return;
        }
        if (n < L && e.pins == 0 && std::equal(e.toks.begin(), e.toks.end(), toks.begin())) covered.push_back(other);
      }
      for (int other : covered) drop_entry(rep, other);
    }
    if ((int)c.entries.size() >= pc_max_) {
      bool any = false;
      for (const auto& kv : c.entries) any = any || kv.second.pins == 0;
      if (!any) {
        pools_[rep]->free({slot});
        return;
      }
      evict_lru(rep, -1);
    }
    Entry e;
    e.toks = toks;
    e.used = ++pc_tick_;
    c.entries.emplace(slot, std::move(e));
    c.index[h].push_back(slot);
  }

  // The sequence's first token is back: the copy from the entry it hit is done.
  void unpin(Seq& s) {
    if (s.hit_slot < 0) return;
    const auto it = caches_[s.rep].entries.find(s.hit_slot);
    if (it != caches_[s.rep].entries.end() && it->second.pins > 0) it->second.pins -= 1;
    s.hit_slot = -1;
  }

  bool group_plan(int rep, int g, int64_t step, GroupOut* go, std::vector<int64_t>* admitted) {
    Group& gh = groups_[rep][g];
    int ret = 0, n = 0, b = 0, ctxb = 0;
    bool changed = false;
    std::vector<ChunkOut> chunks;
    std::vector<RowOut> rows;
    Produced* prev = nullptr;
    const int64_t prev_id = gh.prev;
    gh.prev = -1;
    if (prev_id >= 0) {
      prev = &produced_.at(prev_id);
      ret = prev->b + (int)prev->finals.size();
    }
    // leaves: every token scheduled, or EOS read back
    bool any_leave = false;
    for (const Seq* s : gh.rowp)
      if (s->issued >= s->want || s->stop) {
        any_leave = true;
        break;
      }
    // steady state (no leave, no newly sampled prefill): the rows stay put
    const bool same = !any_leave && !(prev && !prev->finals.empty());
    std::vector<int64_t> new_rows;
    std::vector<Seq*> new_p;
    if (same) {
      new_rows = gh.rows;
    } else {
      for (size_t i = 0; i < gh.rows.size(); ++i) {
        const int64_t sid = gh.rows[i];
        Seq* s = gh.rowp[i];
        if (s->issued >= s->want || s->stop) {
          ++leaves_;
          if (prev) prev->release.push_back(sid);
        } else {
          new_rows.push_back(sid);
          new_p.push_back(s);
        }
      }
      if (prev)
        for (int64_t sid : prev->finals) {
          new_rows.push_back(sid);
          new_p.push_back(&seqs_.at(sid));
        }
    }
    changed = !same && new_rows != gh.rows;
    // joins (capacity counts rows + sequences still prefilling)
    const int room = cap_ - (int)new_rows.size() - (int)gh.prefilling.size();
    if (join_ok(gh, room, new_rows.empty() && gh.prefilling.empty()))
      for (int64_t sid : admit(rep, g, room, admitted)) gh.prefilling.push_back(sid);
    // prefill chunks (FIFO, one chunk per sequence per step, token budget)
    int64_t budget = budget_ > 0 ? budget_ : (int64_t(1) << 62);
    std::vector<int64_t> finals;
    const std::vector<int64_t> pf = gh.prefilling;
    // forks whose parent's final chunk was planned in the previous step: one
    // token each, ahead of every other chunk, whatever the budget has left
    for (int64_t sid : pf) {
      Seq& s = seqs_.at(sid);
      if (s.parent < 0 || !s.ready) continue;
      const int L = s.prompt_len;
      budget -= 1;
      chunks.emplace_back(sid, s.slot, L - 1, 1, true);
      forks_.emplace_back(sid, s.src_slot);
      s.prefilled = L;
      gh.prefilling.erase(std::find(gh.prefilling.begin(), gh.prefilling.end(), sid));
      finals.push_back(sid);
      s.issued = 1;
      s.pos = L;
      s.sstep = 1;
    }
    for (int64_t sid : pf) {
      Seq& s = seqs_.at(sid);
      if (s.parent >= 0) continue;  // a fork: planned above, or waiting for its parent's final chunk
      const int L = s.prompt_len;
      const int take = chunk_ <= 0 ? L - s.prefilled : std::min(chunk_, L - s.prefilled);
      if (!chunks.empty() && take > budget) break;
      budget -= take;
      const int a = s.prefilled;
      const bool final = a + take == L;
      chunks.emplace_back(sid, s.slot, a, take, final);
      if (s.hit_new) {  // the first chunk of a prefix-cache hit: behind a copy of [0, a)
        forks_.emplace_back(sid, s.hit_slot);
        hits_.emplace_back(sid, a);
        s.hit_new = false;
      }
      s.prefilled += take;
      if (final) {
        gh.prefilling.erase(std::find(gh.prefilling.begin(), gh.prefilling.end(), sid));
        finals.push_back(sid);
        s.issued = 1;
        s.pos = L;
        s.sstep = 1;
        for (int64_t fid : s.forks) seqs_.at(fid).ready = true;  // their chunks: the next step
        s.forks.clear();
      }
    }
    // decode rows
    n = (int)new_rows.size();
    b = bucket(n, cap_);
    const std::vector<Seq*>& rp = same ? gh.rowp : new_p;
    if (changed) {
      std::unordered_map<int64_t, int> old_index;
      for (size_t i = 0; i < gh.rows.size(); ++i) old_index[gh.rows[i]] = (int)i;
      for (size_t k = 0; k < new_rows.size(); ++k) {
        const int64_t sid = new_rows[k];
        const Seq& s = *rp[k];
        int src;
        auto f = old_index.find(sid);
        if (f != old_index.end()) {
          src = f->second;
        } else {
          const auto p = std::find(prev->finals.begin(), prev->finals.end(), sid);
          src = prev->b + (int)(p - prev->finals.begin());
        }
        rows.emplace_back(sid, s.slot, s.pos, s.sstep, src);
      }
    }
    if (n) {
      int top = 0;
      for (const Seq* s : rp) top = std::max(top, s->pos);
      top += 1;
      ctxb = std::min((top + 255) / 256 * 256, max_seq_);
      for (Seq* s : rp) {  // one token per decode row this step
        s->issued += 1;
        s->pos += 1;
        s->sstep += 1;
      }
    }
    if (!same) {
      gh.rows = new_rows;
      gh.rowp = std::move(new_p);
    }
    max_rows_ = std::max(max_rows_, n);
    if (b || !finals.empty()) {
      Produced np;
      np.b = b;
      np.rows = new_rows;
      np.finals = finals;
      gh.prev = next_id_;
      produced_[next_id_++] = std::move(np);
    }
    if (prev) {  // its readout comes back in this step's token-return vector
      expect_[key(rep, step, g)] = std::move(*prev);
      produced_.erase(prev_id);
    }
    const bool has_work = b > 0 || !chunks.empty();
    if (!(ret || has_work)) return false;
    *go = GroupOut(g, ret, n, b, ctxb, changed, std::move(chunks), std::move(rows));
    return true;
  }

  // The token `tok`, the ntok-th of the sequence (already counted), goes
  // into the tail; true when it completes a stop sequence and ntok >
  // min_tokens.
  static bool stop_match(Stops& st, int tok, int ntok) {
    if (st.ntail == MAX_STOP_LEN) {
      std::copy(st.tail + 1, st.tail + MAX_STOP_LEN, st.tail);
      --st.ntail;
    }
    st.tail[st.ntail++] = tok;
    if (ntok <= st.min_tokens) return false;
    size_t at = 0;
    for (int n : st.lens) {
      if (n <= st.ntail && std::equal(st.toks.begin() + at, st.toks.begin() + at + n, st.tail + st.ntail - n))
        return true;
      at += (size_t)n;
    }
    return false;
  }

  void give(int64_t sid, int tok, int eos, std::vector<Event>* ev) {
    auto it = seqs_.find(sid);
    if (it == seqs_.end()) return;
    Seq& s = it->second;
    if (s.finished || s.ntok >= s.want) return;
    int flags = s.ntok == 0 ? EV_FIRST : 0;
    if (flags) unpin(s);
    s.ntok += 1;
    const bool hit = s.stops && stop_match(*s.stops, tok, s.ntok);
    if (s.stop_at_eos && tok == eos) {
      s.stop = true;
    } else if (hit) {
      s.stop = true;
      flags |= EV_STOP;
    }
    if (s.ntok >= s.want || s.stop) {
      s.finished = true;
      flags |= EV_FINISH;
    }
    ev->emplace_back(sid, tok, flags);
  }

  void give_collect(int64_t sid, int tok, int eos, std::vector<Event>* ev, Finished* done) {
    auto it = seqs_.find(sid);
    if (it == seqs_.end()) return;
    Seq& s = it->second;
    if (s.finished || s.ntok >= s.want) return;
    int flags = s.ntok == 0 ? EV_FIRST : 0;
    if (flags) unpin(s);
    s.ntok += 1;
    s.toks.push_back(tok);
    const bool hit = s.stops && stop_match(*s.stops, tok, s.ntok);
    if (s.stop_at_eos && tok == eos) {
      s.stop = true;
    } else if (hit) {
      s.stop = true;
      flags |= EV_STOP;
    }
    if (s.ntok >= s.want || s.stop) {
      s.finished = true;
      flags |= EV_FINISH;
      done->emplace_back(sid, s.toks);
    }
    if (flags) ev->emplace_back(sid, tok, flags);
  }

  void release(int64_t sid, std::vector<Event>* ev) {
    auto it = seqs_.find(sid);
    if (it == seqs_.end()) return;
    Seq s = it->second;
    seqs_.erase(it);
    unpin(s);
    if (s.slot >= 0) {
      if (pc_max_ > 0 && s.prompt)
        insert_entry(s.rep, s.slot, *s.prompt);
      else
        pools_[s.rep]->free({s.slot});
    }
    ev->emplace_back(sid, -1, EV_RELEASE | (s.finished ? 0 : EV_FINISH));
  }

  int R_, M_, cap_;
  int64_t budget_;
  int chunk_, max_seq_;
  std::vector<SlotAllocator*> pools_;
  std::vector<std::vector<Group>> groups_;
  std::unordered_map<int64_t, Seq> seqs_;
  std::deque<int64_t> waiting_;
  std::map<std::tuple<int, int64_t, int>, Produced> expect_;
  std::unordered_map<int64_t, Produced> produced_;
  int64_t next_id_ = 0, joins_ = 0, leaves_ = 0, steps_ = 0, deferred_ = 0;
  int join_min_ = 1, max_wait_ = 0;
  int max_rows_ = 0;
  std::vector<std::pair<int64_t, int>> forks_, hits_;
  std::vector<Cache> caches_;
  int pc_max_ = 0, pc_min_ = 8;
  int64_t pc_tick_ = 0, pc_hits_ = 0, pc_misses_ = 0, pc_tokens_ = 0, pc_evictions_ = 0;
};

}  // namespace lsd_rt
