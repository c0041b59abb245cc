// Stand-alone driver of plan_gemm() (csrc/kernels/gemm_plan.h) for
// tests/test_gemm_plan.py: built with g++ -fsanitize=address,undefined, no HIP.
//
// Commands on stdin, one per line:
//   reset                      tuning back to the defaults
//   knob <name> <value>        one knob, through its setter's clamping
//   show                       the 15 knobs, in GemmTuning's order
//   M|N|K|S <values...>        the sweep's lists
//   sweep                      a plan line per (M, N, K, S, epi 0..6, kind 0..3), in that nesting
//   plan M N K S epi kind      one plan line
// A plan line is "0" for an invalid plan, else
//   1 <tag> <grid x> <y> <z> <block> <combine_tiles> <tile_floats>
#include <cstdio>
#include <sstream>
#include <string>
#include <vector>

#include "../gemm_plan.h"

using lsd::GemmPlan;
using lsd::GemmTuning;

static bool set_knob(GemmTuning& t, const std::string& name, int v) {
  if (name == "big_min_blocks") t.big_min_blocks = v;
  else if (name == "big_group") t.set_big_group(v);
  else if (name == "big_kind") t.set_big_kind(v);
  else if (name == "tiled3_max_blocks") t.tiled3_max_blocks = v;
  else if (name == "ring_slots") t.set_ring_slots(v);
  else if (name == "ring_tn") t.set_ring_tn(v);
  else if (name == "ring_fill") t.ring_fill = v;
  else if (name == "ring_m96") t.ring_m96 = v;
  else if (name == "ring8") t.set_ring8(v);
  else if (name == "ring8_flags") t.set_ring8_flags(v);
  else if (name == "ring8_pack") t.set_ring8_pack(v);
  else if (name == "d256_slots") t.set_d256_slots(v);
  else if (name == "sk_rows") t.set_sk_rows(v);
  else if (name == "rb_fill") t.rb_fill = v;
  else if (name == "nw2_rows") t.nw2_rows = v;
  else return false;
  return true;
}

static void print_plan(std::string& out, const GemmPlan& p) {
  if (!p.valid) {
    out += "0\n";
    return;
  }
  char line[160];
  std::snprintf(line, sizeof line, "1 %s %u %u %u %u %ld %ld\n", p.tag, p.grid[0], p.grid[1], p.grid[2], p.block,
                p.combine_tiles, p.tile_floats);
  out += line;
}

int main() {
  GemmTuning t;
  std::vector<int> Ms, Ns, Ks, Ss;
  std::string out, line, cmd;
  char buf[1 << 16];
  while (std::fgets(buf, sizeof buf, stdin)) {
    std::istringstream in(buf);
    if (!(in >> cmd)) continue;
    if (cmd == "reset") {
      t = GemmTuning();
    } else if (cmd == "knob") {
      std::string name;
      int v;
      if (!(in >> name >> v) || !set_knob(t, name, v)) {
        std::fprintf(stderr, "bad knob line: %s", buf);
        return 2;
      }
    } else if (cmd == "show") {
      char s[256];
      std::snprintf(s, sizeof s, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", t.big_min_blocks, t.big_group,
                    t.big_kind, t.tiled3_max_blocks, t.ring_slots, t.ring_tn, t.ring_fill, t.ring_m96, t.ring8,
                    t.ring8_flags, t.ring8_pack, t.d256_slots, t.sk_rows, t.rb_fill, t.nw2_rows);
      out += s;
    } else if (cmd == "M" ||cmd == "N" || cmd == "K" || cmd == "S") {
      std::vector<int>& list = cmd == "M" ? Ms : cmd == "N" ? Ns : cmd == "K" ? Ks : Ss;
      list.clear();
      for (int v; in >> v;) list.push_back(v);
    } else if (cmd == "sweep") {
      for (int M : Ms)
        for (int N : Ns)
          for (int K : Ks)
            for (int S : Ss)
              for (int epi = 0; epi < 7; ++epi)
                for (int kind = 0; kind < 4; ++kind) print_plan(out, lsd::plan_gemm(M, N, K, S, epi, kind, t));
      std::fwrite(out.data(), 1, out.size(), stdout);
      out.clear();
    } else if (cmd == "plan") {
      int M, N, K, S, epi, kind;
      if (!(in >> M >> N >> K >> S >> epi >> kind)) return 2;
      print_plan(out, lsd::plan_gemm(M, N, K, S, epi, kind, t));
    } else {
      std::fprintf(stderr, "unknown command: %s", buf);
      return 2;
    }
  }
  std::fwrite(out.data(), 1, out.size(), stdout);
  return 0;
}
