// Stand-alone driver over liodom_amd/csrc/map_register.h (the plain-C++ half of liodom_map_register_poses) and the convergence
// verdict of liodom_math.h: tests/test_map_register_host.py builds it plain and under host sanitizers and feeds it lines.
//   default                                   -> "default <the ten fields>"
//   check name=value ...                      -> "ok <local_cap>" | "refused <reason>"     (fields not named keep their defaults)
//   table <n>                                 -> "table <slots>"
//   layout <rows> <local_cap> <edge_cap>      -> "layout <table> <pose> <T> <count> <pts> <order> <slot> <key> <first> <fill> <corr> <out> <bytes>" | "nofit"
//   verdict <7 old> <7 new> <stop_t> <stop_r> -> "verdict <0|1> <move_t> <move_r>"
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "map_register.h"
#include "liodom_math.h"

using namespace liodom_dev;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "default") {
      liodom_map_register_t o;
      std::memset(&o, 0xff, sizeof(o));
      map_register_default(&o);
      std::printf("default %d %d %d %d %d %d %.17g %.17g %.17g %.17g\n", o.cells_xy, o.cells_z, o.max_passes, o.min_matches, o.local_capacity,
                  o.reserved, o.stop_translation, o.stop_rotation, o.min_range, o.max_range);
    } else if (cmd == "check") {
      liodom_map_register_t o;
      map_register_default(&o);
      std::string kv;
      bool bad = false;
      while (in >> kv) {
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) { bad = true; break; }
        const std::string k = kv.substr(0, eq), v = kv.substr(eq + 1);
        if (k == "cells_xy") o.cells_xy = std::atoi(v.c_str());
        else if (k == "cells_z") o.cells_z = std::atoi(v.c_str());
        else if (k == "max_passes") o.max_passes = std::atoi(v.c_str());
        else if (k == "min_matches") o.min_matches = std::atoi(v.c_str());
        else if (k == "local_capacity") o.local_capacity = std::atoi(v.c_str());
        else if (k == "reserved") o.reserved = std::atoi(v.c_str());
        else if (k == "stop_translation") o.stop_translation = std::strtod(v.c_str(), nullptr);
        else if (k == "stop_rotation") o.stop_rotation = std::strtod(v.c_str(), nullptr);
        else if (k == "min_range") o.min_range = std::strtod(v.c_str(), nullptr);
        else if (k == "max_range") o.max_range = std::strtod(v.c_str(), nullptr);
        else bad = true;
      }
      if (bad) { std::printf("error unknown field\n"); continue; }
      const char* why = map_register_check(&o);
      if (why) std::printf("refused %s\n", why);
      else std::printf("ok %d\n", map_register_local_cap(&o));
    } else if (cmd == "table") {
      long long n = 0;
      in >> n;
      std::printf("table %lld\n", (long long)map_register_table_size(n));
    } else if (cmd == "layout") {
      int rows = 0, cap = 0, edge_cap = 0;
      in >> rows >> cap >> edge_cap;
      RegisterLayout L;
      if (!map_register_layout(rows, cap, edge_cap, &L)) { std::printf("nofit\n"); continue; }
      std::printf("layout %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)L.table, (long long)L.pose, (long long)L.T,
                  (long long)L.count, (long long)L.pts, (long long)L.order, (long long)L.slot, (long long)L.key, (long long)L.first,
                  (long long)L.fill, (long long)L.corr, (long long)L.out, (long long)L.bytes);
    } else if (cmd == "verdict") {
      double a[7], b[7], st = 0, sr = 0, mt = 0, mr = 0;
      auto next = [&in]() { std::string w; in >> w; return std::strtod(w.c_str(), nullptr); };      // (strtod reads nan / inf)
      for (double& x : a) x = next();
      for (double& x : b) x = next();
      st = next(); sr = next();
      const bool ok = register_pass_converged(a, a + 4, b, b + 4, st, sr, &mt, &mr);
      std::printf("verdict %d %.17g %.17g\n", ok ? 1 : 0, mt, mr);
    } else if (!cmd.empty()) {
      std::printf("error unknown command\n");
    }
  }
  return 0;
}
