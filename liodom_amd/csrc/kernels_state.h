// kernels_state.h — a stream's odometry state as one contiguous blob (layout in stream_state_format.h): k_state_pack /
// k_state_unpack, and the per-stream clear behind liodom_reset_stream / liodom_import_stream_state.
// Part of liodom_kernels.h (included there, inside namespace liodom_dev, behind kernels_cov.h; not a standalone header).
// None of this is on the per-scan path: a handle that never calls the four stream-state entry points launches none of these
// kernels and allocates nothing for them.
constexpr int kStateThreads = 256;

// Gathers stream s into `blob` (device memory, 16-byte aligned, state_blob_bytes(P, P * edge_cap, recv_cap) bytes): the record and
// the frame counts by workgroup 0, the window frames oldest first and the received map by all — one 16-byte load and one 16-byte
// store per point, consecutive threads on consecutive points.  The header is the host's.  Grid: ceil((map_cap) / 256) workgroups
// cover any window; workgroups behind the last point return.
__global__ __launch_bounds__(kStateThreads) void k_state_pack(DevView v, int s, unsigned char* blob) {
  __shared__ WinIndex w;
  const StreamState& st = v.state[s];
  const int P = v.prev_frames, nf = st.n_frames, Mw = st.n_map;
  const int nr = v.mapping ? st.n_recv : 0;
  const int tid = threadIdx.x;
  win_index_load(v, s, nf, w, tid, kStateThreads);
  __syncthreads();
  if (blockIdx.x == 0) {
    StateBlobRecord* r = reinterpret_cast<StateBlobRecord*>(blob + kStateHeaderBytes);
    if (tid < 12) { r->odom[tid] = st.odom[tid]; r->prev_odom[tid] = st.prev_odom[tid]; r->final_odom[tid] = st.final_odom[tid]; }
    if (tid < 4) { r->param_q[tid] = st.param_q[tid]; r->imu_q[tid] = v.imu_q[(size_t)s * 4 + tid]; }
    if (tid < 3) r->param_t[tid] = st.param_t[tid];
    if (tid == 0) {
      r->initialized = st.initialized; r->append_raw = st.append_raw; r->frame_count = st.frame_count; r->n_frames = nf;
      r->scan_counter = st.scan_counter; r->status = st.status; r->n_points = Mw; r->n_recv = nr;
      r->has_imu = v.use_imu ? 1 : 0; r->pad = 0;
    }
    int* cnt = reinterpret_cast<int*>(blob + kStateCountsOffset);
    for (int j = tid; j < state_counts_bytes(P) / 4; j += kStateThreads) cnt[j] = j < nf ? w.sbase[j + 1] - w.sbase[j] : 0;
  }
  float4* out = reinterpret_cast<float4*>(blob + state_points_offset(P));
  const int m = blockIdx.x * kStateThreads + tid;
  if (m < Mw) out[m] = win_point(v, s, nf, w, m);
  else if (m < Mw + nr) out[m] = v.recv_pts[(size_t)s * v.recv_cap + (m - Mw)];
}

// The reverse: the record into a fresh StreamState of stream s, the frames into the ring slots the stream's frame_count implies
// (frame j of n_frames, oldest first, lives in slot (frame_count - n_frames + j) % P: finalize_scan's rule), win_n / win_base /
// win_slot, the received map, the IMU orientation.  blob == nullptr: the state of a stream that never ran (liodom_reset_stream).
// The host has checked the blob against the handle's capacities; the counts are clamped here all the same.
// Kept of the old state: n_edges_buf — the edge buffers belong to the handle's pipeline, and an extraction issued ahead for the
// stream's next scan stays valid.  The kernel reads nothing else of the old state (k_stream_clear, launched in front, does).
__global__ __launch_bounds__(kStateThreads) void k_state_unpack(DevView v, int s, const unsigned char* blob) {
  __shared__ int sbase[kMaxFrames + 1];
  __shared__ int sslot[kMaxFrames];
  __shared__ int sh_nf, sh_fc, sh_nr;
  StreamState& st = v.state[s];
  const int P = v.prev_frames, tid = threadIdx.x;
  const StateBlobRecord* r = blob ? reinterpret_cast<const StateBlobRecord*>(blob + kStateHeaderBytes) : nullptr;
  const int* cnt = blob ? reinterpret_cast<const int*>(blob + kStateCountsOffset) : nullptr;
  if (tid == 0) {
    int nf = r ? r->n_frames : 0;
    nf = nf < 0 ? 0 : (nf > P ? P : nf);
    const int fc = r ? (r->frame_count < nf ? nf : r->frame_count) : 0;
    int acc = 0;
    for (int j = 0; j < nf; j++) {
      int c = cnt[j];
      c = c < 0 ? 0 : (c > v.edge_cap ? v.edge_cap : c);
      sbase[j] = acc; acc += c;
      sslot[j] = (fc - nf + j) % P;
    }
    sbase[nf] = acc;
    int nr = (r && v.mapping) ? r->n_recv : 0;
    sh_nf = nf; sh_fc = fc; sh_nr = nr < 0 ? 0 : (nr > v.recv_cap ? v.recv_cap : nr);
  }
  __syncthreads();
  const int nf = sh_nf, fc = sh_fc, nr = sh_nr, Mw = sbase[nf];
  if (blockIdx.x == 0) {
    // a fresh state, word by word (reset_state's initial value), around the edge counts
    int* words = reinterpret_cast<int*>(&st);
    const int e0 = (int)(offsetof(StreamState, n_edges_buf) / 4), e1 = e0 + 4;
    for (int i = tid; i < (int)(sizeof(StreamState) / 4); i += kStateThreads) if (i < e0 || i >= e1) words[i] = 0;
    for (int j = tid; j < P; j += kStateThreads) v.win_n[(size_t)s * P + j] = 0;
    __syncthreads();
    if (tid < 12) {
      const double id = (tid == 0 || tid == 5 || tid == 10) ? 1.0 : 0.0;
      st.odom[tid] = r ? r->odom[tid] : id; st.prev_odom[tid] = r ? r->prev_odom[tid] : id; st.final_odom[tid] = r ? r->final_odom[tid] : id;
      st.pred_odom[0][tid] = id; st.pred_odom[1][tid] = id;
    }
    if (tid < 4) {
      st.param_q[tid] = r ? r->param_q[tid] : (tid == 3 ? 1.0 : 0.0);
      v.imu_q[(size_t)s * 4 + tid] = (r && r->has_imu) ? r->imu_q[tid] : (tid == 3 ? 1.0 : 0.0);
    }
    if (tid < 3) st.param_t[tid] = r ? r->param_t[tid] : 0.0;
    if (tid == 0) {
      st.table_mask = (uint32_t)v.table_size - 1u;
      st.n_recv = nr;
      if (r) {
        st.initialized = r->initialized; st.append_raw = r->append_raw; st.frame_count = fc; st.n_frames = nf;
        st.scan_counter = r->scan_counter; st.status = r->status; st.n_map = Mw;
        st.n_search = Mw + nr;
      }
    }
    for (int j = tid; j < nf; j += kStateThreads) {
      v.win_n[(size_t)s * P + sslot[j]] = sbase[j + 1] - sbase[j];
      v.win_slot[(size_t)s * P + j] = sslot[j];
    }
    for (int j = tid; j <= P; j += kStateThreads) v.win_base[(size_t)s * (P + 1) + j] = j <= nf ? sbase[j] : 0;
  }
  if (!blob) return;
  const float4* in = reinterpret_cast<const float4*>(blob + state_points_offset(P));
  const int m = blockIdx.x * kStateThreads + tid;
  if (m < Mw) {
    int lo = 0, hi = nf;             // largest j with sbase[j] <= m
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (sbase[mid] <= m) lo = mid; else hi = mid; }
    v.win_pts[((size_t)s * P + sslot[lo]) * v.edge_cap + (m - sbase[lo])] = in[m];
  } else if (m < Mw + nr) {
    v.recv_pts[(size_t)s * v.recv_cap + (m - Mw)] = in[m];
  }
}

// Empties everything stream s has built, through the lists of what is occupied (a table holds up to a few thousand cells of
// 2^17 and more slots): the cell hash — both tables of an early_rebuild handle, with their padding and overflow lists —, an
// LDS-built table (slots [0, kLdsSlots), which no list names: k_hash_reset's rule) and the voxel table of a filtered local map.
// Reads the OLD state: launched in front of k_state_unpack.  Any grid of kStateThreads-thread workgroups.
__global__ __launch_bounds__(kStateThreads) void k_stream_clear(DevView v, int s) {
  StreamState& st = v.state[s];
  const int t = blockIdx.x * kStateThreads + threadIdx.x, nt = gridDim.x * kStateThreads;
  const int ntab = v.early_rebuild ? 2 : 1;
  for (int par = 0; par < ntab; par++) hash_clear_used(v, s + par * v.n_streams, st.n_used_tab[par], t, nt);
  if (st.table_mask != (unsigned int)v.table_size - 1u || st.hb_main_fc != 0) {
    CellSlot empty; empty.key = kEmptyKey; empty.start = 0; empty.cnt = 0;
    const int nl = kLdsSlots < v.table_size ? kLdsSlots : v.table_size;
    for (int i = t; i < nl; i += nt) {
      v.cells[(size_t)s * v.table_size + i] = empty;
      if (i < nl / 32) v.cell_bits[(size_t)s * (v.table_size >> 5) + i] = 0u;
    }
  }
  if (v.vox_cells) {
    CellSlot empty; empty.key = kEmptyKey; empty.start = 0; empty.cnt = 0;
    const int nup = st.vox_used < v.map_cap ? st.vox_used : v.map_cap;
    for (int u = t; u < nup; u += nt) {
      const int h = v.vox_used_list[(size_t)s * v.map_cap + u];
      v.vox_cells[(size_t)s * v.table_size + h] = empty;
      v.vox_fill[(size_t)s * v.table_size + h] = 0;
    }
  }
}
