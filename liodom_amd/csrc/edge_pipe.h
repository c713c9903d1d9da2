// edge_pipe.h — the bookkeeping of the three pipeline edge buffers, which two clients share: the pipelined replay
// (liodom_process_resident*, liodom_replay_*) and the two-thread ticket hand-off (liodom_extract_edges_device,
// liodom_odometry_submit_device, liodom_odometry_collect and their polar forms); and the cursor of a page-locked staging ring
// (StagingRing).  Plain C++17 without a HIP include: what decides between LIODOM_ERR_BUSY ("keep the cloud, retry") and
// LIODOM_ERR_NEEDS_SYNC ("a retry would spin for ever"), and whether an extraction may rewrite an edge buffer, runs under g++ and
// host sanitizers (tests/edge_pipe_main.cc, tests/test_edge_pipe.py).  liodom_hip.hip maps each verdict to its code and message,
// and owns the HIP events, streams and buffers that go with the words here.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "liodom_sizes.h"

namespace liodom_dev {

enum TicketSlotVerdict { kSlotFree, kSlotExtractionAhead, kSlotReplayLive, kSlotsFull };
enum SubmitVerdict { kSubmitOk, kSubmitStale, kSubmitAlready, kSubmitTwoInFlight };

// The one place that skips 0: a sequence number 0 means "nothing to wait for".
inline unsigned int next_seq(unsigned int& counter) {
  if (++counter == 0u) ++counter;
  return counter;
}

struct EdgeTicketDraft { int slot; unsigned int seq; };

struct EdgePipe {
  // ---- extraction side (under mx_x) ----
  unsigned int ext_seq;                 // extractions issued into the pipeline buffers (flags: the number a buffer's flag is set to)
  unsigned int eb_seq[kEdgePipeBufs];   // sequence number of the extraction last issued into buffer b
  int x_next;                           // hand-off slot of the next liodom_extract_edges_device
  bool xdone_valid[3];                  // host-fed replay: ev_xdone[r] has been recorded (upload_slot_async)
  // ---- odometry side (under mx_o) ----
  unsigned int odo_seq;                 // odometries enqueued behind a pipeline buffer (flags)
  int parity;                           // edge buffer of the replay's next scan to enter odometry
  int odo_fifo[2], odo_pending;         // slots of the submitted, not yet collected scans (oldest first)
  // ---- the replay's extraction issued ahead: written by a replay step, with both sides held (read by the extraction side) ----
  int pf_slot;                          // resident slot whose extraction has been issued ahead, -1: none
  bool pf_subset;                       // ... for the streams of pf_list only; false: for every stream
  std::vector<int32_t> pf_list;
  // ---- words the other side reads (sequentially consistent, as they always were) ----
  std::atomic<bool> ev_free_valid[kEdgePipeBufs];      // events: ev_free[b] has been recorded.  Written by the odometry side, read by the extraction side
  std::atomic<unsigned int> eb_reader[kEdgePipeBufs];  // flags: number of the odometry that last read buffer b (0: none).  Written by the odometry side, read by the extraction side
  std::atomic<unsigned int> tk_seq[kEdgePipeBufs];     // 0: slot free, else the number of the extraction it holds.  Set by the extraction side (ticket_issued), cleared by
                                                       // the odometry side when that scan's pose has been collected (collected), read by both
  std::atomic<bool> pipe_active;        // scans went through the buffers by ticket since the last drain.  Set by either side, cleared by drained()
  std::atomic<bool> replay_live;        // ... by the replay (their odometries may not have been collected).  Set by a replay step, read by the extraction side, cleared by drained()

  EdgePipe() { reset(); }

  // ---- the two ways back to idle ----
  // Everything in flight has completed (the caller has synchronised the extraction stream and the odometry streams): no buffer has a
  // reader or a writer to wait for, the replay starts over at buffer 0, nothing is issued ahead.  The sequence counters go on, and
  // tickets stay good: tk_seq, x_next, the FIFO and eb_seq are left alone — liodom_sync() may run between an extraction by ticket
  // and its submission, and liodom_odometry_step drains holding the odometry side only, so nothing here may be a word the
  // extraction side writes outside a replay step.  (ev_free_valid and eb_reader are the odometry side's; pf_slot / pf_subset are
  // cleared as drain_pipeline always did: a replay step, their other writer, holds both sides.)
  // Against the four lists this replaces: pipe_active used to survive a drain that found parity != 0 (the || in front of its
  // exchange) — dead, it only made the next drain synchronise idle streams; replay_live and pipe_active used to be cleared before
  // the synchronisation, and stayed cleared if it failed — now they are cleared once it has succeeded.
  void drained() {
    pf_slot = -1; pf_subset = false; parity = 0;
    for (int b = 0; b < kEdgePipeBufs; b++) { ev_free_valid[b] = false; eb_reader[b] = 0u; }
    pipe_active.store(false); replay_live.store(false);
  }
  // liodom_reset (both sides held, every stream synchronised): drained(), and the counters start over, outstanding tickets are void.
  // Also the constructor's state.  Against reset_state's old list: pipe_active was left set (dead: as above), and xdone_valid, the FIFO's
  // entries and pf_list kept their values (dead: every event has completed; odo_pending == 0 and pf_subset == false hide the others).
  // What a reset keeps on purpose lives outside this struct: a StagingRing's `next` (below).
  void reset() {
    drained();
    ext_seq = odo_seq = 0u; x_next = 0; odo_pending = 0; odo_fifo[0] = odo_fifo[1] = 0; pf_list.clear();
    for (int b = 0; b < kEdgePipeBufs; b++) { eb_seq[b] = 0u; tk_seq[b] = 0u; xdone_valid[b] = false; }
  }
  bool needs_drain() const { return pf_slot >= 0 || parity != 0 || pipe_active.load() || replay_live.load(); }

  // ---- tickets ----
  bool tickets_idle() const {      // the plain entry points and the replay use the pipeline buffers themselves
    for (int b = 0; b < kEdgePipeBufs; b++) if (tk_seq[b].load() != 0u) return false;
    return true;
  }
  // Is the hand-off slot of the next extraction by ticket free?  Extraction side.  The replay uses the same three buffers (parity)
  // and may have odometries in flight that nobody has collected: an extraction by ticket waits for no reader on the device (a slot
  // is refilled only after its pose has been collected), so it would rewrite a buffer under them.
  TicketSlotVerdict ticket_slot() const {
    if (pf_slot >= 0) return kSlotExtractionAhead;
    if (replay_live.load()) return kSlotReplayLive;
    if (tk_seq[x_next].load() != 0u) return kSlotsFull;
    return kSlotFree;
  }
  // The slot and the number of the extraction about to be launched (the number is a kernel argument) ...
  EdgeTicketDraft ticket_draft() { return EdgeTicketDraft{x_next, next_seq(ext_seq)}; }
  // ... and, once it has been launched, the ticket is out.  (A launch that failed leaves the slot free.)
  void ticket_issued(const EdgeTicketDraft& t) {
    eb_seq[t.slot] = t.seq;
    pipe_active.store(true);
    tk_seq[t.slot].store(t.seq);
    x_next = (t.slot + 1) % kEdgePipeBufs;
  }
  // Odometry side.  slot is within [0, kEdgePipeBufs).
  SubmitVerdict submit_check(unsigned int seq, int slot) const {
    if (seq == 0u || tk_seq[slot].load() != seq) return kSubmitStale;
    for (int i = 0; i < odo_pending; i++) if (odo_fifo[i] == slot) return kSubmitAlready;
    if (odo_pending >= 2) return kSubmitTwoInFlight;
    return kSubmitOk;
  }
  void submitted(int slot) {
    pipe_active.store(true);
    odo_fifo[odo_pending++] = slot;
  }
  // The lag wait_pose is given for the oldest scan in flight (its scan count is that many behind the enqueue count); < 0: none.
  int collect_lag() const { return odo_pending - 1; }
  // The oldest scan's pose has been waited for — its odometry has completed: its slot may be refilled.  Returns the slot.
  int collected() {
    const int slot = odo_fifo[0];
    odo_fifo[0] = odo_fifo[1];
    odo_pending--;
    tk_seq[slot].store(0u);
    return slot;
  }

  // ---- what an enqueue leaves behind (flags: sequence numbers; events: that the event has been recorded) ----
  unsigned int extract_numbered(int eb) { return eb_seq[eb] = next_seq(ext_seq); }      // extraction side
  unsigned int odometry_numbered() { return next_seq(odo_seq); }                        // odometry side: the number of the next odometry ...
  void odometry_reads(int eb, unsigned int m) { eb_reader[eb] = m; }                    // ... which has been enqueued behind buffer eb
  void odometry_recorded(int eb) { ev_free_valid[eb] = true; }

  // ---- the replay (both sides held) ----
  int replay_buffer() { replay_live.store(true); return parity; }      // the buffer of the step's scan; from here on scans of the replay are in the buffers
  void replay_advance() { parity = (parity + 1) % kEdgePipeBufs; }
  // Has the extraction of `slot` been issued ahead for exactly these streams (all S of them: no list)?
  bool ahead_matches(int slot, const int32_t* streams, int n_active, int S) const {
    if (pf_slot != slot) return false;
    if (n_active == S) return !pf_subset;
    return pf_subset && (int)pf_list.size() == n_active && std::equal(streams, streams + n_active, pf_list.begin());
  }
  void ahead_set(int slot, const int32_t* streams, int n, int S) {
    pf_slot = slot; pf_subset = n != S;
    if (pf_subset) pf_list.assign(streams, streams + n);
  }
  void ahead_clear() { pf_slot = -1; pf_subset = false; }
};

// The cursor of a page-locked staging ring of kEdgePipeBufs slots: liodom_scan_buffer* hands slot `next` out, a pageable source is
// copied through it, and valid[r] says that the event "the upload has left slot r" has been recorded.  Extraction side.  The events,
// the waiting and the recording are liodom_hip.hip's (ring_*).  liodom_reset clears valid (uploads_left) and keeps `next`, as it
// always did: the buffer liodom_scan_buffer handed out before the reset is still the one the next upload is expected from.
struct StagingRing {
  unsigned char* base = nullptr;
  size_t stride = 0;                    // bytes per slot
  int next = 0;
  bool valid[kEdgePipeBufs] = {false, false, false};
  void bind(void* mem, size_t slot_bytes) { base = static_cast<unsigned char*>(mem); stride = slot_bytes; next = 0; uploads_left(); }
  unsigned char* slot(int r) const { return base + (size_t)r * stride; }
  int owns(const void* p) const {      // the slot p lies in, or -1
    const unsigned char* q = static_cast<const unsigned char*>(p);
    if (!base || q < base || q >= base + (size_t)kEdgePipeBufs * stride) return -1;
    return (int)((size_t)(q - base) / stride);
  }
  // The slot an upload reads: the source's own slot (own = owns(source) >= 0), none (-1) for a buffer the caller registered, and for
  // pageable memory slot `next`, which the source is copied into first.
  int source_slot(int own, bool registered) const { return own >= 0 ? own : (registered ? -1 : next); }
  void upload_recorded(int r) { valid[r] = true; next = (r + 1) % kEdgePipeBufs; }
  void uploads_left() { for (int b = 0; b < kEdgePipeBufs; b++) valid[b] = false; }      // every upload has completed
};

}  // namespace liodom_dev
