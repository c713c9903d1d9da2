// liodom_replay — replays a directory of KITTI-style Velodyne scans (NNNNNN.bin, float32 x y z i)
// through the GPU path with the reference's parameters and writes the reference's result files
// (poses.txt in KITTI format, *_times.txt, nfeats.txt; src/stats.cc:73-132).
//
//   liodom_replay <scan_dir> <out_dir/> [name=value ...]     e.g. scan_lines=64 prev_frames=20
// With mapping=true the liodom_mapping node (launch/liodom.launch:41-56) is replayed on the device
// with its launch-file parameters (voxel_xysize= voxel_zsize= resolution= cells_xy= cells_z=); the
// final map is written to <out_dir>map.bin (float32 x y z i) and its cell count printed.  mapper_lag=1 inserts a frame when it
// leaves the sliding window instead of right after its scan (liodom_attach_mapper_ex: the mode that solves; the default 0 is the
// reference's loop, whose poses are the prediction); map_prune_period=N map_keep_xy= map_keep_z= prune the map to that box of
// cells around the pose every N-th scan.  map_state_in=FILE starts the mapper from a saved map state
// (liodom::Map::importState, before it is attached); map_state_out=FILE writes the mapper's state at the end, before map.bin.
// map_pager=KEEP_XY,KEEP_Z,LOAD_XY,LOAD_Z runs a liodom::MapPager after every scan: the device map is a window onto a map kept on
// the host (cells outside the keep box are paged out, stored cells inside the load box paged in); map_state_out= then writes the
// whole map (MapPager::exportAll) and the run prints the pager's counters.  Fused per-scan path only.
// localize=1 (with mapping=true map_state_in=FILE) runs the traversal AGAINST the saved map instead of building one: the map is
// attached read-only (LaserOdometer::attachMapReader: it is never written), seed_pose=qx,qy,qz,qw,tx,ty,tz places the first scan
// in it (LaserOdometer::seed; default: the identity) and every scan solves against window ++ local map.  Not with mapper_lag,
// map_prune_period or map_pager, which write.
// map_hits=FILE (with localize=1) switches the per-scan hit records on (LaserOdometer::setMapHits, hit_radius=0|1, default 1) and
// writes one line per scan: scan_index hits_r hits_0 n_edges.  relocalize_below=FRACTION adds the recovery (track_policy.h with
// lost_after=N, default 3): when the policy answers LOST, the scan's edges (FeatureExtractor::lastEdges) are searched in the map around the pose of the last scan
// whose fraction was >= FRACTION (this scan's pose if there was none) — one branch-and-bound level of +-reloc_window=METRES
// (default 10) at 0.4 m and +-pi at 0.02 rad, then the fine level (0.1 m, 0.005 rad, +-4 steps) — and, if the best pose's fraction
// is >= FRACTION, the odometer is seeded there and the SAME scan processed again: the result files and FILE keep one row per scan,
// the last processing's, and the run prints "relocalized at scan K".  Fused per-scan path only.
// threads=true runs the reference's own structure instead of the fused per-scan call: the clouds are
// pushed into SharedData (lidarClb), a FeatureExtractor thread and a LaserOdometer thread work side by
// side on the same handle (src/liodom_node.cc:89-91) and hand edge clouds over through the queue — the clouds stay on the
// device (tickets; handoff=host restores host clouds).  poll_us= sets the worker loops' sleep (2000 as the reference; 0 = yield);
// the run prints its scans/s.
// save_state=FILE save_at=K writes the odometer's state (LaserOdometer::saveState) after scan K and goes on; load_state=FILE
// first=K+1 starts from such a file at scan K+1: the result files of the two runs, one behind the other, are those of one run
// (last=K stops after scan K).  Fused per-scan path only (not with threads=true).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <dirent.h>
#include <fstream>
#include <iostream>
#include <memory>
#include <thread>

#include "liodom_host.h"
#include "../csrc/track_policy.h"

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s <scan_dir> <out_dir/> [name=value ...]\n", argv[0]); return 2; }
  const std::string dir = argv[1], out = argv[2];
  std::vector<std::string> kv(argv + 3, argv + argc);
  kv.push_back("save_results=true");
  liodom::Params* params = liodom::Params::getInstance();
  params->readParams(kv);

  std::vector<std::string> files;
  if (DIR* d = opendir(dir.c_str())) {
    while (dirent* e = readdir(d)) {
      const std::string n = e->d_name;
      if (n.size() > 4 && n.substr(n.size() - 4) == ".bin") files.push_back(dir + "/" + n);
    }
    closedir(d);
  }
  std::sort(files.begin(), files.end());
  if (files.empty()) { std::fprintf(stderr, "no .bin scans in %s\n", dir.c_str()); return 1; }

  size_t max_pts = 0;
  std::vector<liodom::PointCloud> clouds(files.size());
  for (size_t i = 0; i < files.size(); i++) {
    std::ifstream f(files[i], std::ios::binary | std::ios::ate);
    const size_t bytes = (size_t)f.tellg();
    f.seekg(0);
    clouds[i].points.resize(bytes / sizeof(liodom::Point));
    f.read(reinterpret_cast<char*>(clouds[i].points.data()), (std::streamsize)(clouds[i].points.size() * sizeof(liodom::Point)));
    clouds[i].width = (uint32_t)clouds[i].points.size(); clouds[i].height = 1;
    if (params->lidar_type_ == 1) {   // organised: rows = scan_lines
      clouds[i].height = (uint32_t)params->scan_lines_;
      clouds[i].width = (uint32_t)(clouds[i].points.size() / (size_t)params->scan_lines_);
    }
    max_pts = std::max(max_pts, clouds[i].points.size());
  }
  try {
    bool covariance = false;      // covariance=1: per-scan pose covariance, written to covariances.txt
    for (const std::string& a : kv) if (a == "covariance=1" || a == "covariance=true") covariance = true;
    auto eng = std::make_shared<liodom::Engine>(*params, 0, (int)max_pts, (int)(max_pts / (size_t)params->scan_lines_ + 1), 1, covariance ? 1 : 0);
    liodom::LaserOdometer odometer(eng);
    std::unique_ptr<liodom::Map> mapper;
    std::unique_ptr<liodom::MapPager> pager;
    std::string map_state_in, map_state_out, map_pager, seed_pose;
    bool localize = false;
    std::string map_hits;
    int hit_radius = 1;
    liodom_dev::TrackPolicy policy{-1.0, 3};      // relocalize_below < 0: no recovery
    double reloc_window = 10.0;
    for (const std::string& a : kv) {
      if (a == "localize=1" || a == "localize=true") localize = true;
      if (a.rfind("map_hits=", 0) == 0) map_hits = a.substr(9);
      if (a.rfind("hit_radius=", 0) == 0) hit_radius = std::stoi(a.substr(11));
      if (a.rfind("relocalize_below=", 0) == 0) policy.min_fraction = std::stod(a.substr(17));
      if (a.rfind("lost_after=", 0) == 0) policy.lost_after = std::stoi(a.substr(11));
      if (a.rfind("reloc_window=", 0) == 0) reloc_window = std::stod(a.substr(13));
      if (a.rfind("seed_pose=", 0) == 0) seed_pose = a.substr(10);
      if (a.rfind("map_state_in=", 0) == 0) map_state_in = a.substr(13);
      if (a.rfind("map_state_out=", 0) == 0) map_state_out = a.substr(14);
      if (a.rfind("map_pager=", 0) == 0) map_pager = a.substr(10);
    }
    if (!map_pager.empty() && !params->mapping_) { std::fprintf(stderr, "liodom_replay: map_pager needs mapping=true\n"); return 2; }
    if ((!map_state_in.empty() || !map_state_out.empty()) && !params->mapping_) {
      std::fprintf(stderr, "liodom_replay: map_state_in / map_state_out need mapping=true\n"); return 2;
    }
    if (localize && (!params->mapping_ || map_state_in.empty())) { std::fprintf(stderr, "liodom_replay: localize=1 needs mapping=true map_state_in=FILE\n"); return 2; }
    if (!seed_pose.empty() && !localize) { std::fprintf(stderr, "liodom_replay: seed_pose needs localize=1\n"); return 2; }
    const bool recover = policy.min_fraction >= 0.0;
    if ((!map_hits.empty() || recover) && !localize) { std::fprintf(stderr, "liodom_replay: map_hits / relocalize_below need localize=1 (a map that is read)\n"); return 2; }
    if (recover && map_hits.empty()) { std::fprintf(stderr, "liodom_replay: relocalize_below needs map_hits=FILE\n"); return 2; }
    if ((hit_radius != 0 && hit_radius != 1) || !(reloc_window >= 0.0) || (recover && !(policy.min_fraction <= 1.0))) {
      std::fprintf(stderr, "liodom_replay: hit_radius is 0 or 1, reloc_window >= 0, relocalize_below in 0 .. 1\n"); return 2;
    }
    if (params->mapping_) {
      double xy = 40.0, z = 50.0, res = 0.4;      // liodom_mapping_node.cc:115-134
      liodom_mapper_options_t mo;
      liodom_mapper_options_default(&mo);
      for (const std::string& a : kv) {
        const size_t eq = a.find('=');
        if (eq == std::string::npos) continue;
        const std::string k = a.substr(0, eq), v = a.substr(eq + 1);
        if (k == "voxel_xysize") xy = std::stod(v); else if (k == "voxel_zsize") z = std::stod(v);
        else if (k == "resolution") res = std::stod(v); else if (k == "cells_xy") mo.cells_xy = std::stoi(v);
        else if (k == "cells_z") mo.cells_z = std::stoi(v); else if (k == "mapper_lag") mo.lag = std::stoi(v);
        else if (k == "map_prune_period") mo.prune_period = std::stoi(v); else if (k == "map_keep_xy") mo.keep_cells_xy = std::stoi(v);
        else if (k == "map_keep_z") mo.keep_cells_z = std::stoi(v);
      }
      mapper.reset(new liodom::Map(xy, z, res));
      if (!map_state_in.empty()) {
        std::ifstream f(map_state_in, std::ios::binary | std::ios::ate);
        if (!f) { std::fprintf(stderr, "liodom_replay: cannot read %s\n", map_state_in.c_str()); return 1; }
        std::vector<uint8_t> st((size_t)f.tellg());
        f.seekg(0);
        f.read(reinterpret_cast<char*>(st.data()), (std::streamsize)st.size());
        mapper->importState(st);
      }
      if (localize) {
        if (mo.lag != 0 || mo.prune_period != 0 || !map_pager.empty()) { std::fprintf(stderr, "liodom_replay: localize=1 reads the map: not with mapper_lag, map_prune_period or map_pager\n"); return 2; }
        liodom::Pose sp;
        if (!seed_pose.empty() && std::sscanf(seed_pose.c_str(), "%lf,%lf,%lf,%lf,%lf,%lf,%lf", &sp.q[0], &sp.q[1], &sp.q[2], &sp.q[3], &sp.t[0], &sp.t[1], &sp.t[2]) != 7) {
          std::fprintf(stderr, "liodom_replay: seed_pose=qx,qy,qz,qw,tx,ty,tz\n"); return 2;
        }
        odometer.attachMapReader(mapper.get(), mo.cells_xy, mo.cells_z);
        odometer.seed(sp);
        if (!map_hits.empty()) odometer.setMapHits(hit_radius);
      } else {
        odometer.attachMapper(mapper.get(), mo);
      }
      if (!map_pager.empty()) {
        int b[4] = {0, 0, 0, 0};
        if (std::sscanf(map_pager.c_str(), "%d,%d,%d,%d", &b[0], &b[1], &b[2], &b[3]) != 4) {
          std::fprintf(stderr, "liodom_replay: map_pager=KEEP_XY,KEEP_Z,LOAD_XY,LOAD_Z\n"); return 2;
        }
        pager.reset(new liodom::MapPager(mapper.get(), b[0], b[1], b[2], b[3]));
      }
    }
    std::ofstream odom_log(out + "odom.txt");      // stamp, orientation xyzw, position, twist linear, twist angular
    odom_log.precision(17);
    std::ofstream cov_log;                          // covariance=1: scan index, flags, the 36 values of OdometryMsg::pose_covariance
    if (covariance) { cov_log.open(out + "covariances.txt"); cov_log.precision(17); }
    size_t cov_rows = 0;
    auto write_cov = [&](const liodom::OdometryMsg& msg) {
      if (!covariance) return;
      cov_log << cov_rows++ << ' ' << msg.covariance_flags;
      for (double v : msg.pose_covariance) cov_log << ' ' << v;
      cov_log << '\n';
    };
    bool threads = false, host_handoff = false;
    int poll_us = 2000;
    std::string save_state, load_state;
    long save_at = -1, first = 0, last = (long)clouds.size() - 1;
    for (const std::string& a : kv) {
      if (a.rfind("save_state=", 0) == 0) save_state = a.substr(11);
      if (a.rfind("load_state=", 0) == 0) load_state = a.substr(11);
      if (a.rfind("save_at=", 0) == 0) save_at = std::stol(a.substr(8));
      if (a.rfind("first=", 0) == 0) first = std::stol(a.substr(6));
      if (a.rfind("last=", 0) == 0) last = std::min(last, std::stol(a.substr(5)));
    }
    if ((!save_state.empty() || !load_state.empty()) && mapper) { std::fprintf(stderr, "liodom_replay: save_state / load_state do not carry an attached map\n"); return 2; }
    {
      // option combinations that would silently do something else than asked
      bool want_threads = false, has_first = false, has_last = false;
      for (const std::string& a : kv) {
        if (a == "threads=true" || a == "threads=1") want_threads = true;
        if (a.rfind("first=", 0) == 0) has_first = true;
        if (a.rfind("last=", 0) == 0) has_last = true;
      }
      const char* bad = nullptr;
      if (want_threads && !map_hits.empty()) bad = "map_hits / relocalize_below work on the fused per-scan path only, not with threads=true";
      else if (want_threads && pager) bad = "map_pager works on the fused per-scan path only, not with threads=true";
      else if (want_threads && (!save_state.empty() || !load_state.empty() || save_at >= 0 || has_first || has_last))
        bad = "save_state / load_state / save_at / first / last work on the fused per-scan path only, not with threads=true";
      else if (save_state.empty() != (save_at < 0)) bad = "save_state=FILE and save_at=K go together";
      else if (save_at >= (long)clouds.size()) bad = "save_at names a scan behind the last one";
      else if (has_first && load_state.empty()) bad = "first=K needs load_state=FILE (the state after scan K - 1)";
      else if (!load_state.empty() && !has_first) bad = "load_state=FILE needs first=K, the scan the state continues with";
      else if (first < 0 || first > last + 1) bad = "first / last out of range";
      else if (save_at >= 0 && (save_at < first || save_at > last)) bad = "save_at lies outside first .. last: the state would never be written";
      if (bad) { std::fprintf(stderr, "liodom_replay: %s\n", bad); return 2; }
    }
    if (!load_state.empty()) {
      std::ifstream f(load_state, std::ios::binary | std::ios::ate);
      if (!f) { std::fprintf(stderr, "liodom_replay: cannot read %s\n", load_state.c_str()); return 1; }
      std::vector<uint8_t> st((size_t)f.tellg());
      f.seekg(0);
      f.read(reinterpret_cast<char*>(st.data()), (std::streamsize)st.size());
      odometer.loadState(st);
    }
    for (const std::string& a : kv) {
      if (a == "threads=true" || a == "threads=1") threads = true;
      if (a == "handoff=host") host_handoff = true;
      if (a.rfind("poll_us=", 0) == 0) poll_us = std::stoi(a.substr(8));
    }
    if (threads) {
      liodom::FeatureExtractor extractor(eng);
      extractor.setDeviceHandoff(!host_handoff);
      liodom::SharedData* sdata = liodom::SharedData::getInstance();
      sdata->poll_us = poll_us;
      const auto t_begin = std::chrono::steady_clock::now();
      std::vector<liodom::OdometryMsg> msgs;
      std::atomic<bool> running{true};
      std::thread feat_thread([&] { extractor(running); });                 // liodom_node.cc:89
      std::thread odom_thread([&] { odometer(running, &msgs, nullptr); });   // liodom_node.cc:90-91
      for (size_t i = 0; i < clouds.size(); i++) {
        if (params->save_results_) liodom::Stats::getInstance()->startFrame(liodom::Clock::now());   // lidarClb :49-52
        sdata->pushPointCloud(clouds[i], 0.1 * (double)i);                 // lidarClb :54
      }
      // (msgs is appended by the odometer thread only; its size is polled until every scan is through)
      for (int spin = 0; spin < 3000000; spin++) {
        std::this_thread::sleep_for(std::chrono::microseconds(100));
        if (liodom::Stats::getInstance()->numPoses() >= clouds.size()) break;
      }
      const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
      running = false;
      feat_thread.join();
      odom_thread.join();
      for (const liodom::OdometryMsg& msg : msgs) {
        odom_log << msg.stamp;
        for (double v : msg.orientation) odom_log << ' ' << v;
        for (double v : msg.position) odom_log << ' ' << v;
        for (double v : msg.linear) odom_log << ' ' << v;
        for (double v : msg.angular) odom_log << ' ' << v;
        odom_log << '\n';
        write_cov(msg);
      }
      std::printf("threads: %zu scans through the extractor / odometer threads in %.3f s = %.1f scans/s (handoff=%s, poll_us=%d)\n",
                  msgs.size(), secs, (double)msgs.size() / secs, host_handoff ? "host" : "device", poll_us);
      if (msgs.size() != clouds.size()) { std::fprintf(stderr, "liodom_replay: %zu of %zu scans processed\n", msgs.size(), clouds.size()); return 1; }
    }
    std::ofstream hits_log;
    if (!map_hits.empty()) hits_log.open(map_hits);
    liodom_dev::TrackState track;
    liodom::Pose last_good;
    bool have_good = false;
    liodom::FeatureExtractor reloc_extractor(eng);
    for (size_t i = (size_t)std::max(0l, first); (long)i <= last && !threads; i++) {
      liodom_step_info_t info;
      liodom::Pose p = odometer.processScan(clouds[i], 0.1 * (double)i, &info);
      if (!map_hits.empty()) {
        liodom_map_hit_t hit = odometer.mapHit(info.scan_index);
        if (recover && liodom_dev::track_feed(policy, &track, hit.hits_r, hit.hits_0, hit.n_edges, hit.flags) == liodom_dev::TRACK_LOST) {
          liodom::PointCloud edges;
          reloc_extractor.lastEdges(edges);      // (the scan's edges as they lie in the handle: what the record was counted on)
          const liodom::Pose& c = have_good ? last_good : p;
          liodom_pose_search_t s;
          liodom_pose_search_default(&s);
          for (int j = 0; j < 4; j++) s.centre[j] = c.q[j];
          for (int j = 0; j < 3; j++) s.centre[4 + j] = c.t[j];
          s.step_xy = 0.4; s.step_yaw = 0.02; s.nx = s.ny = (int)std::ceil(reloc_window / 0.4); s.nyaw = (int)std::ceil(M_PI / 0.02); s.radius = 1;
          liodom_pose_search_result_t found = mapper->searchPoseBnb(edges, s);
          for (int j = 0; j < 7; j++) s.centre[j] = found.pose[j];
          s.step_xy = 0.1; s.step_yaw = 0.005; s.nx = s.ny = s.nyaw = 4;
          found = mapper->searchPose(edges, s);
          if (!liodom_dev::track_below(policy, found.hits_r, found.hits_0, (int32_t)edges.size())) {
            liodom::Pose sp;
            for (int j = 0; j < 4; j++) sp.q[j] = found.pose[j];
            for (int j = 0; j < 3; j++) sp.t[j] = found.pose[4 + j];
            odometer.seed(sp);
            liodom::Stats::getInstance()->dropLastScan();
            p = odometer.processScan(clouds[i], 0.1 * (double)i, &info);
            hit = odometer.mapHit(info.scan_index);
            std::printf("relocalized at scan %zu: fraction %.3f at %.3f %.3f %.3f\n", i, liodom_dev::track_fraction(found.hits_r, found.hits_0, (int32_t)edges.size()),
                        found.pose[4], found.pose[5], found.pose[6]);
          } else {
            std::printf("lost at scan %zu: nothing good enough within the window (best fraction %.3f)\n", i,
                        liodom_dev::track_fraction(found.hits_r, found.hits_0, (int32_t)edges.size()));
          }
        }
        if ((hit.flags & LIODOM_HIT_VALID) && !liodom_dev::track_below(policy, hit.hits_r, hit.hits_0, hit.n_edges)) { last_good = p; have_good = true; }
        hits_log << hit.scan_index << ' ' << hit.hits_r << ' ' << hit.hits_0 << ' ' << hit.n_edges << '\n';
      }
      const liodom::OdometryMsg msg = odometer.publishOdom(0.1 * (double)i, p);      // ~odom / ~twist numbers
      odom_log << msg.stamp;
      for (double v : msg.orientation) odom_log << ' ' << v;
      for (double v : msg.position) odom_log << ' ' << v;
      for (double v : msg.linear) odom_log << ' ' << v;
      for (double v : msg.angular) odom_log << ' ' << v;
      odom_log << '\n';
      write_cov(msg);
      if (pager) pager->step(p.matrix34());
      if (i % 50 == 0) std::printf("scan %zu: %d edges, %d matches, t = %.3f %.3f %.3f\n", i, info.n_edges, info.matches[1], p.t[0], p.t[1], p.t[2]);
      if ((long)i == save_at && !save_state.empty()) {
        const std::vector<uint8_t> st = odometer.saveState();
        std::ofstream f(save_state, std::ios::binary);
        f.write(reinterpret_cast<const char*>(st.data()), (std::streamsize)st.size());
        std::printf("state after scan %zu: %zu bytes -> %s\n", i, st.size(), save_state.c_str());
      }
    }
    liodom::Stats::getInstance()->writeResults(out);
    if (mapper) {
      odometer.attachMapper(nullptr);
      if (pager) std::printf("pager: %lld evicted, %lld loaded, %lld conflicts, %zu cells stored\n", pager->evicted, pager->loaded, pager->conflicts, pager->stored());
      if (!map_state_out.empty()) {
        const std::vector<uint8_t> st = pager ? pager->exportAll() : mapper->exportState();
        std::ofstream f(map_state_out, std::ios::binary);
        f.write(reinterpret_cast<const char*>(st.data()), (std::streamsize)st.size());
        std::printf("map state: %zu bytes -> %s\n", st.size(), map_state_out.c_str());
      }
      const liodom::PointCloud m = mapper->getMap();
      std::ofstream f(out + "map.bin", std::ios::binary);
      f.write(reinterpret_cast<const char*>(m.points.data()), (std::streamsize)(m.points.size() * sizeof(liodom::Point)));
      std::printf("map: %zu points in %d cells\n", m.size(), mapper->numCells());
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "liodom_replay: %s\n", e.what());
    return 1;
  }
  return 0;
}
