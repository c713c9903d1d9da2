// kernels_mapper.h — the lagged mapper of liodom_attach_mapper_ex (lag = 1; no counterpart in the reference): a frame enters the
// attached map when it LEAVES the sliding window, so the map and the window never share a point ("Lagged mapper").
// Included by liodom_kernels.h.  A handle without a lagged mapper launches none of this.
#pragma once

// First launch of a step, in front of the scan's first kNN pass on the odometry stream: for every stream of the step that has a
// lagged mapper (lag[s] != 0) and a full window, the frame this scan's append will overwrite — slot frame_count % P, the oldest
// frame liodom_get_window shows before the step (finalize_scan's rule) — is copied aside with its count; stash_n = 0 while the
// window is not full.  Plain stream order does the rest: the previous scan's append has completed, this scan's has not begun.
// grid (chunk, row); 16-byte loads and stores, consecutive lanes on consecutive points.
template <bool kList = false>
__global__ __launch_bounds__(256) void k_window_stash(DevView v, int s0, const int* lag, float4* stash, int* stash_n) {
  const int s = stream_of<kList>(v, s0, blockIdx.y);
  if (!lag[s]) return;
  const StreamState& st = v.state[s];
  const int P = v.prev_frames;
  int n = 0;
  if (st.n_frames == P) {
    const int slot = st.frame_count % P;
    n = max(0, min(v.win_n[(size_t)s * P + slot], v.edge_cap));
    const float4* src = v.win_pts + ((size_t)s * P + slot) * v.edge_cap;
    float4* dst = stash + (size_t)s * v.edge_cap;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) dst[i] = src[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) stash_n[s] = n;
}
