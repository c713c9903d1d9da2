// Driver of tests/test_edge_pipe.py: the bookkeeping of the pipeline edge buffers and the cursor of a staging ring
// (liodom_amd/csrc/edge_pipe.h) without a device.  Standard input is a sequence of lines:
//   new flags=0|1           a fresh EdgePipe; flags: the handle orders its HIP streams by sequence numbers, else by events
//   set ext=N odo=N         (driver only) the two sequence counters
//   x | s k | c | r | ra | y | z | p      the operations of tests/edge_pipe_cases.py
//   ahead slot S [list]     EdgePipe::ahead_set;  match slot S [list]  prints ahead_matches;  unahead  ahead_clear
//   ring stride             a StagingRing bound to a buffer of 3 slots of `stride` bytes
//   owns offset             the slot that owns base + offset (offset may be negative)
//   src own k | reg | page  the cursor's part of an upload from slot k of the ring / a registered buffer / pageable memory
//   hand                    liodom_scan_buffer*: the slot handed out (its upload has been waited for);  left  uploads_left
// The driver models only what the entry points of liodom_hip.hip add around EdgePipe: which function they call in which order.
// Output: one line per operation, "<verdict> | <state>" (Model.state of edge_pipe_cases.py), for ring lines "<answer> | next valid".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "edge_pipe.h"

using namespace liodom_dev;

struct Driver {
  EdgePipe pipe;
  bool flags = true;
  std::vector<EdgeTicketDraft> tickets;      // the script's: every ticket it was given
  int cur = 0;                               // the resident slot of the replay's next step
};

static void extract(Driver& d, int eb) { if (d.flags) d.pipe.extract_numbered(eb); }
static void odometry(Driver& d, int eb) {
  if (d.flags) d.pipe.odometry_reads(eb, d.pipe.odometry_numbered());
  else d.pipe.odometry_recorded(eb);
}

static void print_state(const EdgePipe& p, const std::string& verdict) {
  std::printf("%s | tk=%u,%u,%u x_next=%d fifo=", verdict.c_str(), p.tk_seq[0].load(), p.tk_seq[1].load(), p.tk_seq[2].load(), p.x_next);
  if (p.odo_pending == 0) std::printf("-");
  for (int i = 0; i < p.odo_pending; i++) std::printf(i ? ",%d" : "%d", p.odo_fifo[i]);
  std::printf(" ext=%u odo=%u ebs=%u,%u,%u ebr=%u,%u,%u free=%d,%d,%d parity=%d pf=%d active=%d live=%d\n", p.ext_seq, p.odo_seq, p.eb_seq[0],
              p.eb_seq[1], p.eb_seq[2], p.eb_reader[0].load(), p.eb_reader[1].load(), p.eb_reader[2].load(), (int)p.ev_free_valid[0].load(),
              (int)p.ev_free_valid[1].load(), (int)p.ev_free_valid[2].load(), p.parity, p.pf_slot, (int)p.pipe_active.load(), (int)p.replay_live.load());
}

static std::string run(Driver& d, const std::string& op, int k) {
  EdgePipe& p = d.pipe;
  char buf[64];
  if (op == "x") {
    switch (p.ticket_slot()) {
      case kSlotExtractionAhead: return "ahead";
      case kSlotReplayLive: return "replay_live";
      case kSlotsFull: return "full";
      case kSlotFree: break;
    }
    const EdgeTicketDraft t = p.ticket_draft();
    p.ticket_issued(t);
    d.tickets.push_back(t);
    std::snprintf(buf, sizeof(buf), "ok %d %u", t.slot, t.seq);
    return buf;
  }
  if (op == "s") {
    const EdgeTicketDraft t = (k >= 0 && (size_t)k < d.tickets.size()) ? d.tickets[(size_t)k] : EdgeTicketDraft{0, 0u};
    switch (p.submit_check(t.seq, t.slot)) {
      case kSubmitStale: return "stale";
      case kSubmitAlready: return "submitted";
      case kSubmitTwoInFlight: return "two_in_flight";
      case kSubmitOk: break;
    }
    odometry(d, t.slot);
    p.submitted(t.slot);
    return "ok";
  }
  if (op == "c") {
    const int lag = p.collect_lag();
    if (lag < 0) return "none";
    std::snprintf(buf, sizeof(buf), "ok %d %d", p.collected(), lag);
    return buf;
  }
  if ((op == "r" || op == "ra" || op == "p") && !p.tickets_idle()) return "tickets_out";
  if (op == "r" || op == "ra") {
    const int eb = p.replay_buffer();
    if (!p.ahead_matches(d.cur, nullptr, 1, 1)) extract(d, eb);
    p.ahead_clear();
    odometry(d, eb);
    p.replay_advance();
    d.cur++;
    if (op == "ra") { extract(d, p.parity); p.ahead_set(d.cur, nullptr, 1, 1); }
  } else if (op == "p" || (op == "y" && p.pf_slot < 0)) {
    if (p.needs_drain()) p.drained();
  } else if (op == "z") {
    p.reset();
  } else if (op != "y") {
    std::fprintf(stderr, "unknown operation '%s'\n", op.c_str());
    std::exit(2);
  }
  return "ok";
}

static std::vector<int32_t> int_list(std::istringstream& in) {
  std::vector<int32_t> v;
  std::string w;
  if (in >> w) { std::istringstream ls(w); std::string e; while (std::getline(ls, e, ',')) v.push_back(std::atoi(e.c_str())); }
  return v;
}

int main() {
  Driver* d = new Driver();
  StagingRing ring;
  std::vector<unsigned char> mem;
  constexpr int kPad = 64;      // the ring starts this far into its buffer: addresses below its base exist
  auto ring_state = [&](long long answer) { std::printf("%lld | next=%d valid=%d,%d,%d\n", answer, ring.next, (int)ring.valid[0], (int)ring.valid[1], (int)ring.valid[2]); };
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, w;
    if (!(in >> op)) continue;
    if (op == "new") {
      delete d;
      d = new Driver();
      if (in >> w) d->flags = w != "flags=0";
      print_state(d->pipe, "new");
    } else if (op == "set") {
      while (in >> w) {
        const unsigned int v = (unsigned int)std::strtoul(w.c_str() + w.find('=') + 1, nullptr, 10);
        if (w.compare(0, 4, "ext=") == 0) d->pipe.ext_seq = v; else d->pipe.odo_seq = v;
      }
    } else if (op == "ahead" || op == "match") {
      int slot = 0, S = 0;
      in >> slot >> S;
      const std::vector<int32_t> l = int_list(in);
      const int n = l.empty() ? S : (int)l.size();
      if (op == "ahead") { d->pipe.ahead_set(slot, l.data(), n, S); print_state(d->pipe, "ok"); }
      else std::printf("%d\n", d->pipe.ahead_matches(slot, l.data(), n, S) ? 1 : 0);
    } else if (op == "unahead") {
      d->pipe.ahead_clear();
      print_state(d->pipe, "ok");
    } else if (op == "ring") {
      size_t stride = 0;
      in >> stride;
      mem.assign(2 * kPad + (size_t)kEdgePipeBufs * stride, 0);
      ring.bind(mem.data() + kPad, stride);
      ring_state(0);
    } else if (op == "owns") {
      long long off = 0;
      in >> off;
      ring_state(ring.owns(ring.base + off));
    } else if (op == "src") {
      int k = 0;
      in >> w;
      if (w == "own") in >> k;
      const unsigned char outside = 0;
      const int own = ring.owns(w == "own" ? ring.slot(k) + ring.stride / 2 : &outside);
      const int used = ring.source_slot(own, w == "reg");
      if (used >= 0) ring.upload_recorded(used);
      ring_state(used);
    } else if (op == "hand") {
      ring.valid[ring.next] = false;
      ring_state(ring.next);
    } else if (op == "left") {
      ring.uploads_left();
      ring_state(0);
    } else {
      int k = -1;
      in >> k;
      print_state(d->pipe, run(*d, op, k));
    }
  }
  delete d;
  return 0;
}
