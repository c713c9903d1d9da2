// map_attach.h — which map is attached to which stream of a handle, as what: the bookkeeping behind liodom_attach_mapper*,
// liodom_attach_map_reader, liodom_set_map_hits and the map's side of liodom_destroy.  Plain C++17 without a HIP include: the
// rules run under g++ and host sanitizers (tests/map_attach_main.cc, tests/test_map_attach.py).  The checks return verdicts, which
// liodom_hip.hip maps to codes and messages; the transitions change the words here and return what the HIP half has to do
// (AttachEffects), which liodom_hip.hip carries out (carry_out): stream sync / destroy / create and the small copies to the
// device words reader_sel[s], lag_on[s].  The lazily allocated device buffers stay liodom_hip.hip's.
//
// What holds (DESIGN.md "Map attachments" has the same list):
//  1. A reader refuses a map another handle holds (kAttachOtherHandle); a writer moves it here without a word.  The handle that
//     lost it keeps naming it, and its steps keep enqueueing to it, until its stream detaches; that detach leaves the map's link alone.
//  2. Attach first, detach second: a stream that re-attaches the map it holds keeps the map on the handle's stream throughout.
//  3. A destroyed handle releases only the maps whose holder it still is (release_next).
//  4. detach() takes the stream's attachment away whichever kind it is, and either entry point with m = NULL ends up there.
//  5. n_lagged goes down by what the stream's options say when the writer leaves (they are written on attach only).
//  6. A read map's tag is the lowest free place of the tag table + 1; the place is freed when the last stream reading it leaves.
//  7. Hits on a stream (hits_on) are asked about BEFORE a reader is attached: the caller sizes the map's kept occupancy first.
#pragma once
#include <cstddef>
#include <vector>

namespace liodom_dev {

enum AttachVerdict { kAttachOk, kAttachMapIsRead, kAttachMapIsWritten, kAttachOtherHandle };

// The map's side: how many streams of `holder` hold it, how many of them reading.  holder is null exactly while n_attached == 0.
struct MapLink {
  int n_attached = 0, n_readers = 0;
  const void* holder = nullptr;
};

// What the HIP half does after a transition, in this order.
template <class Map>
struct AttachEffects {
  Map* move_in = nullptr;       // this map moves onto the handle's stream now (first attachment here, or a move from another handle)
  bool sel_cleared = false;     // a reader left the stream: reader_sel[s] = {0, 0, 0, 0}
  Map* own_again = nullptr;     // this map's last attachment has gone: it gets a stream of its own again
  bool sel_written = false;     // a reader came: reader_sel[s] = sel
  int sel[4] = {0, 0, 0, 0};    // {tag, cells_xy, cells_z, 0}
  int lag_on = -1;              // lag_on[s], where the handle has the word; -1: left as it is (a reader's attach never wrote it)
};

// The handle's side.  Map has a member `MapLink link`; Options is liodom_mapper_options_t (cells_xy, cells_z, lag are read here).
// A stream holds one map or none, writing or reading: no stream does both, and a map is read or written, never both.
template <class Map, class Options>
struct StreamMaps {
  struct Entry {
    Map* map = nullptr;
    bool reads = false;
    Options opts{};             // a writer's options; of a reader, cells_xy and cells_z
    int hit_radius = -1;        // liodom_set_map_hits: -1 off
  };
  const void* self = nullptr;   // the holder's identity in a MapLink
  std::vector<Entry> at;        // per stream
  std::vector<Map*> tags;       // distinct maps with readers; a map's tag is its index + 1 (freed places are null and taken again)
  int n_lagged = 0, n_readers = 0, n_hits = 0;      // streams with a lagged writer / a reader / hits on

  void bind(const void* holder, int S) { self = holder; at.assign((size_t)S, Entry{}); }

  // ---- queries ----
  Map* writer(int s) const { const Entry& e = at[(size_t)s]; return e.reads ? nullptr : e.map; }
  Map* reader(int s) const { const Entry& e = at[(size_t)s]; return e.reads ? e.map : nullptr; }
  Map* map_of(int s) const { return at[(size_t)s].map; }      // whichever kind; its extents are opts(s).cells_xy / cells_z
  const Options& opts(int s) const { return at[(size_t)s].opts; }
  bool any_lagged() const { return n_lagged > 0; }
  bool lagged(int s) const { const Entry& e = at[(size_t)s]; return e.map && !e.reads && e.opts.lag == 1; }
  bool hits_on(int s) const { return at[(size_t)s].hit_radius >= 0; }

  // ---- checks: may `m` become the writer / the reader of stream s?  The attachment s holds now does not count: the call replaces it ----
  AttachVerdict writer_check(int s, const Map* m) const {
    int writers = 0, readers = 0;
    others(s, m, &writers, &readers);
    return readers > 0 ? kAttachMapIsRead : kAttachOk;      // (a map another handle writes moves here: 1 above)
  }
  AttachVerdict reader_check(int s, const Map* m) const {
    int writers = 0, readers = 0;
    others(s, m, &writers, &readers);
    if (writers > 0) return kAttachMapIsWritten;
    if (m->link.n_attached > 0 && m->link.holder != self) return kAttachOtherHandle;
    return kAttachOk;
  }

  // ---- transitions ----
  // m becomes the stream's writer (reads = false, with its options) or its reader (reads = true; o carries the extents).  The
  // new attachment is counted before the old one goes (2 above).
  AttachEffects<Map> attach(int s, Map* m, bool reads, const Options& o) {
    AttachEffects<Map> e;
    MapLink& l = m->link;
    if (l.n_attached == 0 || l.holder != self) { e.move_in = m; l.holder = self; l.n_attached = 0; l.n_readers = 0; }
    l.n_attached++;
    if (reads) l.n_readers++;
    release(s, &e);
    Entry& en = at[(size_t)s];
    en.map = m; en.reads = reads; en.opts = o;
    if (reads) {
      size_t t = 0;
      for (; t < tags.size() && tags[t] != m; t++) {}
      if (t == tags.size()) {
        for (t = 0; t < tags.size() && tags[t]; t++) {}
        if (t == tags.size()) tags.push_back(m); else tags[t] = m;
      }
      n_readers++;
      e.sel_written = true; e.sel[0] = (int)t + 1; e.sel[1] = o.cells_xy; e.sel[2] = o.cells_z;
    } else {
      if (o.lag == 1) n_lagged++;
      e.lag_on = o.lag == 1 ? 1 : 0;
    }
    return e;
  }
  AttachEffects<Map> detach(int s) {
    AttachEffects<Map> e;
    release(s, &e);
    e.lag_on = 0;
    return e;
  }
  // liodom_destroy: the next map this handle still holds, let go of at once however many streams held it — writers' maps first,
  // then readers', each in stream order; null when there is none left.  Every map it returns gets a stream of its own again.  The
  // per-stream entries are left as they are: the handle is going.
  Map* release_next() {
    for (int kind = 0; kind < 2; kind++) {
      for (const Entry& en : at) {
        if (!en.map || en.reads != (kind == 1)) continue;
        MapLink& l = en.map->link;
        if (l.n_attached == 0 || l.holder != self) continue;      // (done already, or moved to another handle: 3 above)
        l = MapLink{};
        return en.map;
      }
    }
    return nullptr;
  }
  void set_hits(int s, int radius) {
    int& cur = at[(size_t)s].hit_radius;
    n_hits += (radius >= 0 ? 1 : 0) - (cur >= 0 ? 1 : 0);
    cur = radius;
  }

 private:
  // Attachments of m other than the one stream s holds now: writers, readers.  Of a map another handle holds, all of them.
  void others(int s, const Map* m, int* writers, int* readers) const {
    const Entry& en = at[(size_t)s];
    const int own = (en.map == m && m->link.holder == self) ? 1 : 0;
    *readers = m->link.n_readers - (en.reads ? own : 0);
    *writers = (m->link.n_attached - m->link.n_readers) - (en.reads ? 0 : own);
  }
  // The stream's attachment goes, whichever kind.  A map that has moved to another handle since is not this handle's to count.
  void release(int s, AttachEffects<Map>* e) {
    Entry& en = at[(size_t)s];
    Map* old = en.map;
    if (!old) return;
    en.map = nullptr;
    if (!en.reads) {
      if (en.opts.lag == 1) n_lagged--;
    } else {
      n_readers--;
      e->sel_cleared = true;
      bool still = false;
      for (const Entry& q : at) still = still || (q.reads && q.map == old);
      if (!still) for (Map*& q : tags) if (q == old) q = nullptr;
    }
    MapLink& l = old->link;
    if (l.holder != self) return;
    if (en.reads && l.n_readers > 0) l.n_readers--;
    if (l.n_attached > 0) l.n_attached--;
    if (l.n_attached == 0) { l.n_readers = 0; l.holder = nullptr; e->own_again = old; }
  }
};

}  // namespace liodom_dev
