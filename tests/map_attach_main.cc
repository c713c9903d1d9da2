// Driver of tests/test_map_attach.py: which map is attached to which stream, as what (liodom_amd/csrc/map_attach.h), without a
// device.  Standard input is a sequence of lines:
//   new          handle A with two streams, handle B with one, maps 0 and 1, nothing attached
//   <operation>  one of tests/map_attach_cases.py
// The driver models only what the entry points of liodom_hip.hip add around StreamMaps: which function they call in which order,
// and the device words reader_sel[s] / lag_on[s] as carry_out writes them.  Output: one line per operation,
// "<verdict> <effects> | <state>" (Model.op and Model.state of map_attach_cases.py).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "map_attach.h"

using namespace liodom_dev;

struct Map { MapLink link; };
struct Options { int cells_xy, cells_z, lag; };
using Maps = StreamMaps<Map, Options>;

struct Handle {
  Maps maps;
  std::vector<int> sel, lag_on;      // the device words: sel is [S][3]
  explicit Handle(int S) : sel(3 * (size_t)S, 0), lag_on((size_t)S, 0) { maps.bind(this, S); }
};

struct World {
  Map map[2];
  std::unique_ptr<Handle> h[2] = {std::make_unique<Handle>(2), std::make_unique<Handle>(1)};
  int index_of(const Map* m) const { return (int)(m - map); }
};

// carry_out of liodom_hip.hip, on the mirror of the device words; the text names what it did in its order
static std::string carry_out(World& w, Handle& h, int s, const AttachEffects<Map>& e) {
  std::string t;
  char buf[64];
  if (e.move_in) { std::snprintf(buf, sizeof(buf), " move=%d", w.index_of(e.move_in)); t += buf; }
  if (e.sel_cleared) { for (int k = 0; k < 3; k++) h.sel[3 * (size_t)s + k] = 0; t += " clr=1"; }
  if (e.own_again) { std::snprintf(buf, sizeof(buf), " own=%d", w.index_of(e.own_again)); t += buf; }
  if (e.sel_written) {
    for (int k = 0; k < 3; k++) h.sel[3 * (size_t)s + k] = e.sel[k];
    std::snprintf(buf, sizeof(buf), " sel=%d,%d,%d", e.sel[0], e.sel[1], e.sel[2]); t += buf;
  }
  if (e.lag_on >= 0) h.lag_on[(size_t)s] = e.lag_on;
  std::snprintf(buf, sizeof(buf), " lag=%d", e.lag_on); t += buf;
  return t;
}

static std::string run(World& w, const std::string& o) {
  const int hi = o.size() > 1 ? o[1] - 'A' : -1;
  if (hi < 0 || hi > 1) { std::fprintf(stderr, "unknown operation '%s'\n", o.c_str()); std::exit(2); }
  Handle& h = *w.h[hi];
  if (o[0] == 'X') {
    std::string t;
    while (Map* m = h.maps.release_next()) t += " own=" + std::to_string(w.index_of(m));
    w.h[hi] = std::make_unique<Handle>(hi == 0 ? 2 : 1);
    return "ok" + (t.empty() ? std::string(" -") : t);
  }
  const int s = o[2] - '0';
  if (o[0] == 'h') {
    const int radius = o[3] == '+' ? 0 : -1;
    const bool occ = radius >= 0 && h.maps.reader(s);
    h.maps.set_hits(s, radius);
    return occ ? "ok occ=1" : "ok -";
  }
  if (o[0] == 'd' || o[0] == 'e') return "ok" + carry_out(w, h, s, h.maps.detach(s));
  Map* m = &w.map[o[4] - '0'];
  Options opt{2, 1, o[0] == 'l' ? 1 : 0};
  if (o.size() > 5) std::sscanf(o.c_str() + 5, "/%d/%d", &opt.cells_xy, &opt.cells_z);
  if (o[0] == 'r') {
    switch (h.maps.reader_check(s, m)) {
      case kAttachMapIsWritten: return "is_written -";
      case kAttachOtherHandle: return "other_handle -";
      default: break;
    }
    const bool occ = h.maps.hits_on(s);
    opt.lag = 0;
    return std::string("ok") + (occ ? " occ=1" : "") + carry_out(w, h, s, h.maps.attach(s, m, true, opt));
  }
  if (o[0] != 'w' && o[0] != 'l') { std::fprintf(stderr, "unknown operation '%s'\n", o.c_str()); std::exit(2); }
  if (h.maps.writer_check(s, m) == kAttachMapIsRead) return "is_read -";
  return "ok" + carry_out(w, h, s, h.maps.attach(s, m, false, opt));
}

static void print_state(const World& w, const std::string& answer) {
  std::printf("%s |", answer.c_str());
  for (int hi = 0; hi < 2; hi++) {
    const Handle& h = *w.h[hi];
    for (int s = 0; s < (int)h.maps.at.size(); s++) {
      std::printf(" %c%d=", 'A' + hi, s);
      const Options& op = h.maps.opts(s);
      if (const Map* m = h.maps.writer(s)) std::printf("w%d/%d/%d/%d", w.index_of(m), op.cells_xy, op.cells_z, op.lag);
      else if (const Map* r = h.maps.reader(s)) std::printf("r%d/%d/%d", w.index_of(r), op.cells_xy, op.cells_z);
      else std::printf("-");
      if (h.maps.map_of(s) != (h.maps.writer(s) ? h.maps.writer(s) : h.maps.reader(s))) { std::fprintf(stderr, "map_of disagrees\n"); std::exit(3); }
      if (h.maps.lagged(s) != (h.maps.writer(s) && op.lag == 1)) { std::fprintf(stderr, "lagged disagrees\n"); std::exit(3); }
      std::printf(":h%d:t%d,%d,%d:g%d", h.maps.at[(size_t)s].hit_radius, h.sel[3 * (size_t)s], h.sel[3 * (size_t)s + 1], h.sel[3 * (size_t)s + 2], h.lag_on[(size_t)s]);
    }
  }
  for (int hi = 0; hi < 2; hi++) {
    const Maps& ms = w.h[hi]->maps;
    std::printf(" tags%c=", 'A' + hi);
    if (ms.tags.empty()) std::printf("-");
    for (size_t t = 0; t < ms.tags.size(); t++) {
      if (t) std::printf(",");
      if (ms.tags[t]) std::printf("%d", w.index_of(ms.tags[t])); else std::printf(".");
    }
    std::printf(" cnt%c=%d,%d,%d", 'A' + hi, ms.n_lagged, ms.n_readers, ms.n_hits);
    if (ms.any_lagged() != (ms.n_lagged > 0)) { std::fprintf(stderr, "any_lagged disagrees\n"); std::exit(3); }
  }
  for (int k = 0; k < 2; k++) {
    const MapLink& l = w.map[k].link;
    const char holder = l.holder == nullptr ? '-' : l.holder == w.h[0].get() ? 'A' : l.holder == w.h[1].get() ? 'B' : '?';
    std::printf(" m%d=%d/%d/%c", k, l.n_attached, l.n_readers, holder);
  }
  std::printf("\n");
}

int main() {
  auto w = std::make_unique<World>();
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    if (line == "new") { w = std::make_unique<World>(); print_state(*w, "new -"); }
    else print_state(*w, run(*w, line));
  }
  return 0;
}
