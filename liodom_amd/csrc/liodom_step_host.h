// liodom_step_host.h — part of liodom_hip.hip (included there, inside its unnamed namespace, behind ProfScope; not a standalone
// header): the launch sequences of a scan.  What a step launches, with which grids and in which order, is decided by the pure
// functions of step_plan.h; the code here fills their request, and issue_plan walks the list: it supplies the data arguments and
// holds the one launch expression of every kernel instance.

// What the launches of one plan read besides the plan: the rows, the edge buffer, and the scan of an extraction.
struct StepData {
  int s0 = 0, count = 0, eb = 0;
  const int32_t* list = nullptr;     // host copy of the stream list (s0 < 0)
  hipStream_t qx = nullptr;          // SQ_X
  const float4* in = nullptr; size_t in_stride = 0; int n = 0, height = 0, width = 0;
  unsigned int wait_odo = 0; int mirror = 0; unsigned int* pub_flag = nullptr; unsigned int* pub_host = nullptr; unsigned int pub_value = 0u;
};

// every kernel with rows comes in two instances (stream_of): rows = streams s0 + row, rows = entries of a stream list.
// TA: the template arguments in front of that flag, in parentheses, with their trailing comma.
#define LIODOM_UNPAREN(...) __VA_ARGS__
#define LAUNCH_ROWS(K, TA, ...)                                                                               \
  do {                                                                                                        \
    if (l.list) hipLaunchKernelGGL((K<LIODOM_UNPAREN TA true>), grid, block, l.lds, q, __VA_ARGS__);           \
    else hipLaunchKernelGGL((K<LIODOM_UNPAREN TA false>), grid, block, l.lds, q, __VA_ARGS__);                 \
  } while (0)
#define LAUNCH_ONE(K, ...) hipLaunchKernelGGL(K, grid, block, l.lds, q, __VA_ARGS__)

int issue_plan(liodom_handle* h, const StepPlan& plan, const StepData& d) {
  const DevView& v = h->v;
  const int s0 = d.s0, eb = d.eb;
  std::optional<ProfScope> ps;
  for (int i = 0; i < plan.n; i++) {
    const StepLaunch& l = plan.e[i];
    const hipStream_t q = l.q == SQ_ODO ? h->stream : (l.q == SQ_K ? h->stream_k : d.qx);
    const dim3 grid(l.gx, l.gy), block(l.block);
    if (l.scope != SS_SAME) { ps.reset(); if (l.scope == SS_OPEN) ps.emplace(h, (int)l.bucket, q); }
    switch (l.k) {
      // (the cases stand in the order in which the library has always first named its kernels: the code object lists them in that order, and a
      //  build stays comparable with its predecessors byte for byte.  k_chain_redo0 first: the chain flush; with_pass 0 names no scan's rows or buffer)
      case SK_CHAIN_REDO0: LAUNCH_ONE(k_chain_redo0<256>, v, l.with_pass ? s0 : 0, l.with_pass ? eb : 0, l.wait_edges, l.signal_odo, l.seq_k, l.scan_no, l.nA, l.with_pass, l.with_fix); break;
      // ---- extraction ----
      case SK_ROW_COMPACT: LAUNCH_ROWS(k_row_compact, (), v, s0, d.in, d.in_stride, d.n, d.height, d.width); break;
      case SK_RING_SPLIT_LB: LAUNCH_ROWS(k_ring_split_lb, (), v, s0, d.in, d.in_stride, d.n, d.height, d.width, l.tiles, l.lb_tag); break;
      case SK_RING_SPLIT_FIX: LAUNCH_ROWS(k_ring_split_fix, (), v, s0, d.in, d.in_stride, d.n, d.height, d.width, l.tiles); break;
      case SK_RING_SPLIT: LAUNCH_ROWS(k_ring_split, (), v, s0, d.in, d.in_stride, d.n, d.height, d.width); break;
      case SK_CLASSIFY: LAUNCH_ROWS(k_classify, (), v, s0, d.in, d.in_stride, d.n, d.height, d.width); break;
      case SK_RING_SCATTER: LAUNCH_ROWS(k_ring_scatter, (), v, s0, d.in, d.in_stride, d.n); break;
      case SK_RING_EXTRACT_256_BIG: LAUNCH_ROWS(k_ring_extract, (256, kExIPLBig,), v, s0); break;
      case SK_RING_EXTRACT_256: LAUNCH_ROWS(k_ring_extract, (256, kExIPL,), v, s0); break;
      case SK_RING_EXTRACT_1024_BIG: LAUNCH_ROWS(k_ring_extract, (1024, kExIPLBig,), v, s0); break;
      case SK_RING_EXTRACT_1024: LAUNCH_ROWS(k_ring_extract, (1024, kExIPL,), v, s0); break;
      case SK_COMPACT_EDGES: LAUNCH_ROWS(k_compact_edges, (), v, s0, eb, d.wait_odo, d.mirror, d.pub_flag, d.pub_host, d.pub_value); break;
      // ---- odometry ----
      case SK_IMU_OVERRIDE: LAUNCH_ROWS(k_imu_override, (), v, s0, d.count); break;
      case SK_WINDOW_STASH: LAUNCH_ROWS(k_window_stash, (), v, s0, h->lag_on, h->lag_stash, h->lag_stash_n); break;
      case SK_KNN_CHAIN_FIRST: LAUNCH_ONE((k_knn<256, false, true>), v, s0, 0, eb, l.wait_edges, l.signal_odo, l.seq_k, l.scan_no); break;
      case SK_LM0_CHAIN: LAUNCH_ONE((k_lm_solve<0, true>), v, s0, eb, l.seq_k, l.done_target); break;
      case SK_OV_GATE: LAUNCH_ONE(k_ov_gate, v, s0, l.seq_k); break;
      case SK_KNN_OV: LAUNCH_ONE((k_knn<256, true>), v, s0, l.pass, eb, 0u, 0u, l.seq_k, l.scan_no); break;
      case SK_KNN_REDO: LAUNCH_ONE(k_knn_redo<256>, v, s0, eb, l.seq_k, l.scan_no, l.alloc); break;
      case SK_LM1_CHAIN: LAUNCH_ONE((k_lm_solve<1, true>), v, s0, eb, l.seq_k, l.done_target); break;
      case SK_POSE_COV_CHAIN: LAUNCH_ONE(k_pose_cov<>, v, s0); break;
      case SK_REBUILD_ALLOC: LAUNCH_ONE(k_rebuild_alloc<>, v, s0); break;
      case SK_REBUILD_FIN: LAUNCH_ONE(k_rebuild_fin, v, s0, eb); break;
      case SK_KNN8_0: LAUNCH_ROWS(k_knn8, (0,), v, s0, eb); break;
      case SK_KNN8_1: LAUNCH_ROWS(k_knn8, (1,), v, s0, eb); break;
      case SK_KNN8_EXACT: LAUNCH_ROWS(k_knn8_exact, (), v, s0, l.pass, eb); break;
      case SK_LINE_GATE: LAUNCH_ROWS(k_line_gate, (), v, s0, l.pass, eb); break;
      case SK_KNN128: LAUNCH_ROWS(k_knn, (128, false, false,), v, s0, l.pass, eb, l.wait_edges, l.signal_odo, 0u, 0); break;
      case SK_KNN256: LAUNCH_ROWS(k_knn, (256, false, false,), v, s0, l.pass, eb, l.wait_edges, l.signal_odo, 0u, 0); break;
      case SK_LM0: LAUNCH_ROWS(k_lm_solve, (0, false,), v, s0, eb, l.seq_k, 0u); break;
      case SK_LM1: LAUNCH_ROWS(k_lm_solve, (1, false,), v, s0, eb, l.seq_k, 0u); break;
      case SK_POSE_COV: LAUNCH_ROWS(k_pose_cov, (), v, s0); break;
      case SO_MAP_BLOCK: {      // the mapper / map-reader block of a mapping handle, where it has always stood: behind the solves, in front of the hash step
        const int count = d.count;
        // synchronous replay of the mapping node for the streams with an attached map: updateMap(edges_k,
        // pose_k), then getLocalMap(pose_k) straight into the stream's received-map buffer.
        // lag = 1: the map takes the frame that left the window instead (stashed above; world frame already: no transform), then the
        // optional prune around pose_k, then the same getLocalMap.
        for (int i = 0; i < count; i++) {
          const int s = d.list ? (int)d.list[i] : s0 + i;
          liodom_map* mp = h->maps.writer(s);
          if (!mp) continue;
          ProfScope ps(h, KID_OTHER);
          StreamState* st = v.state + s;
          const liodom_mapper_options_t& mo = h->maps.opts(s);
          int rc = mo.lag == 1 ? map_enqueue_update(mp, h->lag_stash + (size_t)s * v.edge_cap, h->lag_stash_n + s, nullptr, h->stream)
                               : map_enqueue_update(mp, v.edges + ((size_t)eb * v.n_streams + s) * v.edge_cap, &st->n_edges_buf[eb], st->final_odom, h->stream);
          if (rc) return rc;
          // (scans_enqueued[s] is this scan's index: launch_odometry counts it when the step has been enqueued)
          if (mo.prune_period > 0 && (h->scans_enqueued[s] + 1) % mo.prune_period == 0) {
            rc = map_enqueue_prune(mp, st->final_odom, mo.keep_cells_xy, mo.keep_cells_z, h->stream);
            if (rc) return rc;
          }
          rc = map_enqueue_local(mp, st->final_odom, mo.cells_xy, mo.cells_z, v.recv_pts + (size_t)s * v.recv_cap,
                                 v.recv_cap, &st->n_recv, h->stream, 1);
          if (rc) return rc;
        }
        // map readers: getLocalMap(pose_k) of the step's reader rows, one launch per distinct map (k_map_local_rows plans in LDS and
        // writes nothing of the map, so the rows share it); nothing else — no stash, no update, no prune.  A reader whose extents
        // the LDS plan cannot hold takes the two old launches.
        if (h->maps.n_readers > 0) {
          ProfScope ps(h, KID_OTHER);
          const std::vector<liodom_map*>& tags = h->maps.tags;
          for (size_t t = 0; t < tags.size(); t++) {
            liodom_map* mp = tags[t];
            if (!mp) continue;
            bool rows = false;
            for (int i = 0; i < count; i++) {
              const int s = d.list ? (int)d.list[i] : s0 + i;
              if (h->maps.reader(s) != mp) continue;
              const liodom_mapper_options_t& ro = h->maps.opts(s);
              if (h->plan.map_rows && map_rows_fit(mp, ro.cells_xy, ro.cells_z)) { rows = true; continue; }
              StreamState* st = v.state + s;
              const int rc = map_enqueue_local(mp, st->final_odom, ro.cells_xy, ro.cells_z, v.recv_pts + (size_t)s * v.recv_cap, v.recv_cap, &st->n_recv, h->stream, 1);
              if (rc) return rc;
            }
            if (!rows) continue;
            MapRows r{};
            r.T = v.state[0].final_odom; r.T_stride = (long long)(sizeof(StreamState) / sizeof(double));
            r.out = v.recv_pts; r.out_stride = v.recv_cap;
            r.n_out = &v.state[0].n_recv; r.n_stride = (long long)(sizeof(StreamState) / sizeof(int));
            r.total = nullptr; r.sel = h->reader_sel; r.tag = (int)t + 1; r.cap = v.recv_cap; r.sticky = 1;
            r.s0 = s0; r.list = s0 < 0 ? reinterpret_cast<const int*>(v.pipe_flags) + kStreamListBase + (size_t)(-s0 - 1) * (size_t)v.n_streams : nullptr;
            const dim3 grid(map_rows_grid_x(count, v.recv_cap), count);
            if (s0 < 0) hipLaunchKernelGGL((k_map_local_rows<true>), grid, dim3(kMapRowsThreads), 0, h->stream, mp->m, r);
            else hipLaunchKernelGGL((k_map_local_rows<false>), grid, dim3(kMapRowsThreads), 0, h->stream, mp->m, r);
          }
        }
        // per-scan hit records (liodom_set_map_hits): the step's rows with hits on, counted at final_odom against the occupancy
        // of the map they read — one k_map_hit_rows launch per distinct map, in front of it the occupancy's two launches only if
        // the map may have changed since it was built — and one launch for the rows without a reader (NO_READER records).
        if (h->maps.n_hits > 0) {
          ProfScope ps(h, KID_OTHER);
          MapHitRows r{};
          r.edges = v.edges + (size_t)eb * v.n_streams * v.edge_cap; r.edge_stride = v.edge_cap;
          r.n_edges = &v.state[0].n_edges_buf[eb]; r.n_stride = (long long)(sizeof(StreamState) / sizeof(int));
          r.T = v.state[0].final_odom; r.T_stride = (long long)(sizeof(StreamState) / sizeof(double));
          r.edge_cap = v.edge_cap; r.log = reinterpret_cast<uint4*>(h->hit_log); r.log_cap = v.pose_log_cap;
          r.scan_no = &v.state[0].scan_counter; r.raw = &v.state[0].append_raw;
          r.radius_of = h->hit_radius; r.sel = h->reader_sel; r.s0 = s0;
          r.list = s0 < 0 ? reinterpret_cast<const int*>(v.pipe_flags) + kStreamListBase + (size_t)(-s0 - 1) * (size_t)v.n_streams : nullptr;
          const std::vector<liodom_map*>& tags = h->maps.tags;
          for (size_t t = 0; t <= tags.size(); t++) {      // (the last turn: tag 0, the rows without a reader)
            liodom_map* mp = t < tags.size() ? tags[t] : nullptr;
            if (t < tags.size() && !mp) continue;
            bool any = false;
            for (int i = 0; i < count && !any; i++) {
              const int s = d.list ? (int)d.list[i] : s0 + i;
              any = h->maps.hits_on(s) && h->maps.reader(s) == mp;
            }
            if (!any) continue;
            if (mp) { const int rc = map_refresh_occ(mp, h->stream); if (rc) return rc; }
            r.tag = mp ? (int)t + 1 : 0;
            const MapView none{};
            if (s0 < 0) hipLaunchKernelGGL((k_map_hit_rows<true>), dim3(count), dim3(kMapHitThreads), 0, h->stream, mp ? mp->m : none, mp ? mp->d_occ : nullptr,
                                           mp ? mp->occ_cells : 0, mp ? (float)mp->cfg.resolution : 0.f, r);
            else hipLaunchKernelGGL((k_map_hit_rows<false>), dim3(count), dim3(kMapHitThreads), 0, h->stream, mp ? mp->m : none, mp ? mp->d_occ : nullptr,
                                    mp ? mp->occ_cells : 0, mp ? (float)mp->cfg.resolution : 0.f, r);
          }
        }
        break;
      }
      case SK_HASH_APPEND: LAUNCH_ROWS(k_hash_append, (), v, s0, eb); break;
      case SK_HASH_BUILD: LAUNCH_ROWS(k_hash_build, (), v, s0, eb); break;
      case SK_WINDOW_INSERT: LAUNCH_ROWS(k_window_insert, (), v, s0, eb); break;
      case SK_HASH_ALLOC: LAUNCH_ROWS(k_hash_alloc, (), v, s0); break;
      case SK_HASH_SCATTER: LAUNCH_ROWS(k_hash_scatter, (), v, s0); break;
      case SK_VOXEL_BBOX: LAUNCH_ROWS(k_voxel_bbox, (), v, s0); break;
      case SK_VOXEL_INSERT: LAUNCH_ROWS(k_voxel_insert, (), v, s0); break;
      case SK_VOXEL_ALLOC: LAUNCH_ROWS(k_voxel_alloc, (), v, s0); break;
      case SK_VOXEL_SCATTER: LAUNCH_ROWS(k_voxel_scatter, (), v, s0); break;
      case SK_VOXEL_CENTROID: LAUNCH_ROWS(k_voxel_centroid, (), v, s0); break;
      case SK_FILT_INSERT: LAUNCH_ROWS(k_filt_insert, (), v, s0); break;
      case SK_FILT_ALLOC: LAUNCH_ROWS(k_filt_alloc, (), v, s0); break;
      case SK_FILT_SCATTER: LAUNCH_ROWS(k_filt_scatter, (), v, s0); break;
      // ---- host-side operations ----
      case SO_EV_OV:
        HIP_TRY(hipEventRecord(h->ev_ov, h->stream));
        HIP_TRY(hipStreamWaitEvent(h->stream_k, h->ev_ov, 0));
        break;
      case SO_EV_CH:
        HIP_TRY(hipEventRecord(h->ev_ch, h->stream_k));
        HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_ch, 0));
        break;
    }
  }
  ps.reset();
  HIP_TRY(hipGetLastError());
  return LIODOM_OK;
}
#undef LAUNCH_ROWS
#undef LAUNCH_ONE
#undef LIODOM_UNPAREN

// The odometry side's device results (window, correspondences, pose log, state) are complete when its streams have drained: in
// chain mode the kNN passes and the rebuild run on stream_k.
// Speculative hand-over of a chain-mode scan's result (kernels_sync.h): the repair of an APPEND that started from a pose the solve
// did not end with rides behind the NEXT scan's first pass (k_chain_redo0).  When no such pass follows — the handle leaves chain
// mode, or the host is about to read the odometry side's results — the repair is enqueued on its own (it waits for the scan's
// verdict; normally it finds nothing to do).
void chain_flush(liodom_handle* h) {
  StepPlan plan;
  plan_chain_flush(h->plan, &h->step, h->scans_enqueued[0], &plan);
  if (plan.n) (void)issue_plan(h, plan, StepData{});
}
hipError_t sync_odometry(liodom_handle* h) {
  chain_flush(h);
  hipError_t e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess && h->step.chain_used && h->stream_k) e = hipStreamSynchronize(h->stream_k);
  return e;
}

// Feature extraction of `count` streams starting at s0; input scan for stream s0+i at in + i*stride.
// s0 < 0: of the `count` streams of device-side stream list -s0 - 1 (put_stream_list); input scan of stream s at in + s*stride.
int launch_extract(liodom_handle* h, hipStream_t q, int eb, int s0, int count, const float4* in, size_t in_stride,
                   int n, int height, int width, unsigned int wait_odo = 0, int mirror = 0, unsigned int* pub_flag = nullptr, unsigned int* pub_host = nullptr, unsigned int pub_value = 0u) {
  ExtractRequest rq;
  rq.count = count; rq.list = s0 < 0; rq.n = n; rq.width = width; rq.max_width = h->config.max_width;
  StepPlan plan;
  plan_extract_step(h->plan, &h->xstep, rq, &plan);
  StepData d;
  d.s0 = s0; d.count = count; d.eb = eb; d.qx = q; d.in = in; d.in_stride = in_stride; d.n = n; d.height = height; d.width = width;
  d.wait_odo = wait_odo; d.mirror = mirror; d.pub_flag = pub_flag; d.pub_host = pub_host; d.pub_value = pub_value;
  return issue_plan(h, plan, d);
}

// The handle's part of the decision to overlap the second kNN pass (ov) and to run a scan in chain mode (chain): the streamed
// rebuild, flags between the streams, and the GPU to this handle alone — its waiting workgroups and those of a second handle of
// the process could end up behind each other in a shared hardware queue.  plan_odometry_step adds the scan's own conditions.
OverlapModes overlap_modes(const liodom_handle* h) { return plan_overlap_modes(h->plan, g_live_handles.load() <= 1); }

// Odometry on the dense edges already on the device; the poses are published by k_lm_solve into host-mapped memory (HostOut).
// s0 < 0: the `count` streams of device-side stream list -s0 - 1, whose entries the host loops read from `list`.
int enqueue_odometry(liodom_handle* h, int eb, int s0, int count, unsigned int wait_edges, unsigned int signal_odo, const int32_t* list = nullptr) {
  StepRequest rq;
  rq.s0 = s0; rq.count = count; rq.list = list; rq.wait_edges = wait_edges; rq.signal_odo = signal_odo;
  rq.profiling = h->profiling; rq.ov_suppress = h->ov_suppress; rq.alone = g_live_handles.load() <= 1;
  rq.scans_enqueued = count > 0 ? h->scans_enqueued[rq.stream_at(0)] : 0;
  if (h->maps.any_lagged()) for (int i = 0; i < count; i++) rq.lagged = rq.lagged || h->maps.lagged(rq.stream_at(i));
  StepPlan plan;
  plan_odometry_step(h->plan, &h->step, rq, &plan);
  StepData d;
  d.s0 = s0; d.count = count; d.eb = eb; d.list = list;
  return issue_plan(h, plan, d);
}

int launch_odometry(liodom_handle* h, int eb, int s0, int count, unsigned int wait_edges = 0, unsigned int signal_odo = 0, const int32_t* list = nullptr) {
  // (a hipGraph replay of this launch sequence was measured slower than the eager launches in rounds 1-2 — the chain is
  //  bound by its kernels, the host enqueue is hidden behind them, hipGraphLaunch adds start latency — and removed in round 3)
  const int rc = enqueue_odometry(h, eb, s0, count, wait_edges, signal_odo, list);
  if (rc) return rc;
  for (int i = 0; i < count; i++) { const int s = list ? list[i] : s0 + i; h->last_eb[s] = eb; h->scans_enqueued[s]++; }
  return LIODOM_OK;
}
