// kernels_cov.h — k_pose_cov: per-scan pose covariance and eigen-decomposition (config.pose_covariance = 1).
// Part of liodom_kernels.h (included there, inside namespace liodom_dev, after kernels_lm.h; not a standalone header).
// =============================================================================================
// k_pose_cov: one 64-thread workgroup per stream, grid (count), launched on the odometry HIP stream straight behind every
//   finalising solve (k_lm_solve<1, ...>).  It reads what that solve's controller left in v.cov_raw[s] (pose_cov_store:
//   H at the returned pose, cost, residual blocks, termination) and forms the record of liodom_pose_cov_t on one lane
//   (pose_cov_compute, liodom_math.h: sigma^2, Cholesky inverse, cyclic Jacobi — FP64, ~a thousand instructions, once per scan);
//   the wave then stores it into the device log (entry [s][k], skipped for k >= pose_log_cap like finalize_scan's pose log) and
//   into the host-mapped record k & 1 of the stream, whose sequence word is written last with a system-scope release (as HostOut).
//   Why the raw record cannot be overwritten before this launch reads it: the next writer is the NEXT scan's finalising solve,
//   which is enqueued on the same HIP stream behind this launch.  In chain mode the next scan's first solve is enqueued there too —
//   it follows this launch in stream order, and the next second kNN pass (and so the next finalising solve) waits for that solve.
//   The host-mapped slot k & 1 is rewritten by scan k + 2 only, whose launches follow this one on the same stream.
// =============================================================================================
template <bool kList = false>
__global__ __launch_bounds__(64) void k_pose_cov(DevView v, int s0) {
  const int s = stream_of<kList>(v, s0, (int)blockIdx.x);
  const int lane = (int)threadIdx.x;
  __shared__ liodom_pose_cov_t rec;
  __shared__ double sh_H[21];
  const PoseCovRaw* r = v.cov_raw + s;
  if (lane < 21) sh_H[lane] = r->H[lane];
  __syncthreads();
  if (lane == 0) {
    rec.scan_index = r->scan_index;
    rec.n_residuals = r->n_res;
    rec.termination = r->termination;
    rec.final_cost = r->cost;
    rec.flags = pose_cov_compute(sh_H, r->cost, r->n_res, r->termination, r->has_solve, &rec.sigma2, rec.information, rec.covariance,
                                 rec.eigenvalues, rec.eigenvectors);
  }
  __syncthreads();
  const int k = rec.scan_index;
  if (k < 0) return;
  constexpr int kWords = (int)(sizeof(liodom_pose_cov_t) / 8);
  static_assert(sizeof(liodom_pose_cov_t) % 8 == 0, "record is copied as 8-byte words");
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&rec);
  if (k < v.pose_log_cap) {
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(v.cov_log + (size_t)s * v.pose_log_cap + k);
    for (int i = lane; i < kWords; i += 64) dst[i] = src[i];
  }
  HostCov* ho = v.cov_host + (size_t)s * 2 + (k & 1);      // two records per stream: the host may read scan k while scan k + 1 publishes
  unsigned long long* hdst = reinterpret_cast<unsigned long long*>(&ho->rec);
  for (int i = lane; i < kWords; i += 64) hdst[i] = src[i];
  // every lane's payload stores before the sequence word the host polls
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  __syncthreads();
  if (lane == 0) __hip_atomic_store(&ho->seq, k + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
