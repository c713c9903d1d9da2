// kernels_polar.h — projection of a polar scan (range counts + encoder ticks, liodom_polar_geometry_t) to the packed XYZI cloud
// every later stage reads.  It stands where the sensor driver's projection and pcl::fromROSMsg stand in front of lidarClb
// (src/liodom_node.cc:40-55): the host uploads 3-6 bytes per point instead of 16 and the device writes the 16.
//
// The arithmetic is polar_project_point (liodom_math.h), bit for bit.
// Part of liodom_kernels.h (included there, inside namespace liodom_dev, behind kernels_state.h; not a standalone header).
#pragma once

constexpr int kPolarThreads = 256;
constexpr int kPolarPerThread = 4;
constexpr int kPolarTile = kPolarThreads * kPolarPerThread;      // points per workgroup
constexpr int kPolarMaxHeight = 2048;                            // rows whose beam table fits the LDS beside the tile

struct PolarView {
  const float4* beam;        // [H] (cos_alt, sin_alt, cos_baz, sin_baz)
  const float2* enc;         // [T] (cos_enc, sin_enc)
  int H, W, T, n;            // n = H W
  int range_bytes;           // per count: 2 or 4
  int inten_bytes;           // per intensity: 0, 1 or 2
  int order;                 // the handle's lidar_type: 0: point i = col H + row, 1: i = row W + col
  float range_unit, beam_origin;
  long long range_off, inten_off, blob_bytes;      // polar_sections
};

inline size_t polar_lds_bytes(int H) { return sizeof(float4) * (size_t)H; }

// One workgroup projects kPolarTile consecutive points of one scan (one launch per upload).  The tile's counts and intensities are narrow
// (1-4 bytes): they come in as 16-byte vectors per lane, raw, into the LDS, and each lane then picks the elements of its points —
// lane l of a pass takes point base + l, so a wave stores 1 KB of contiguous float4 per pass.  The beam tables sit in the LDS; the
// tick of a column and its encoder entry come through the cache (type 0: H consecutive points share a column; type 1:
// consecutive points read consecutive ticks).
// Every 16-byte vector read starts inside its section and ends at or before the section's padded end (sections start and end
// on 16-byte boundaries, polar_sections); out[p] is written for p < n only, n <= max_points (liodom_set_polar_geometry).
__global__ __launch_bounds__(kPolarThreads) void k_polar_project(PolarView g, const unsigned char* __restrict__ blob, float4* __restrict__ out) {
  extern __shared__ float4 s_beam[];
  __shared__ uint4 s_rng[kPolarTile * 4 / 16];
  __shared__ uint4 s_int[kPolarTile * 2 / 16];
  const int tid = threadIdx.x;
  const long long base = (long long)blockIdx.x * kPolarTile;
  for (int r = tid; r < g.H; r += kPolarThreads) s_beam[r] = g.beam[r];
  {
    const long long sec = polar_align16((long long)g.n * g.range_bytes), at = base * g.range_bytes + 16LL * tid;
    if (tid < kPolarTile * g.range_bytes / 16 && at < sec) s_rng[tid] = *reinterpret_cast<const uint4*>(blob + g.range_off + at);
  }
  if (g.inten_bytes) {
    const long long sec = polar_align16((long long)g.n * g.inten_bytes), at = base * g.inten_bytes + 16LL * tid;
    if (tid < kPolarTile * g.inten_bytes / 16 && at < sec) s_int[tid] = *reinterpret_cast<const uint4*>(blob + g.inten_off + at);
  }
  __syncthreads();
  const uint32_t* ticks = reinterpret_cast<const uint32_t*>(blob);
  LD_UNROLL
  for (int k = 0; k < kPolarPerThread; k++) {
    const int e = k * kPolarThreads + tid;
    const long long p = base + e;
    if (p >= g.n) break;
    const uint32_t c = g.range_bytes == 2 ? (uint32_t)reinterpret_cast<const unsigned short*>(s_rng)[e]
                                          : reinterpret_cast<const uint32_t*>(s_rng)[e];
    uint32_t iv = 0u;
    if (g.inten_bytes == 1) iv = reinterpret_cast<const unsigned char*>(s_int)[e];
    else if (g.inten_bytes == 2) iv = reinterpret_cast<const unsigned short*>(s_int)[e];
    const uint32_t pi = (uint32_t)p;
    uint32_t row, col;
    if (g.order == 0) { col = pi / (uint32_t)g.H; row = pi - col * (uint32_t)g.H; }
    else { row = pi / (uint32_t)g.W; col = pi - row * (uint32_t)g.W; }
    const uint32_t t = ticks[col];
    const bool tick_ok = t < (uint32_t)g.T;
    float2 en = make_float2(0.f, 0.f);
    if (tick_ok) en = g.enc[t];
    const float4 b = s_beam[row];
    float o[4];
    polar_project_point(c, (float)iv, tick_ok, en.x, en.y, b.x, b.y, b.z, b.w, g.range_unit, g.beam_origin, o);
    out[p] = make_float4(o[0], o[1], o[2], o[3]);
  }
}
