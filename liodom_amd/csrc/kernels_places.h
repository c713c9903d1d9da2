// Finding the place (liodom_places_*; no counterpart in the reference): binary polar descriptors of edge clouds in the sensor frame,
// their Hamming distance under every yaw shift, and the K nearest places of a query.  Included by liodom_hip.hip.
//
// The contract (include/liodom_hip.h; tests/place_model.py restates it in NumPy and every output is held equal):
//   point      (x, y, z) with a non-finite coordinate sets nothing
//   sector     j = #{i = 1..15 : |y| * C_i >= |x| * S_i} (float multiplies); by quadrant (x < 0, y < 0 as written: -0 is not
//              below 0): j, 31 - j, 32 + j, 63 - j
//   ring       r2 = x * x + y * y (two multiplies, one add); ring = #{i : r2 >= R2_i}; ring == n_rings sets nothing
//   layer      z < Z_0 sets nothing; layer = #{i >= 1 : z >= Z_i}; layer == n_layers sets nothing
//   bit        `sector` of word ring * n_layers + layer
//   distance   d(s) = sum over w of popcount(rotl64(q[w], s) ^ k[w]); a place's distance is the smallest d(s), its shift the lowest
//              such s; places rank by (distance, index)
// The tables are the database's (place_state_format.h: PlaceTables), read from global memory with wave-uniform indices.
#pragma once

#include "place_state_format.h"
#include "wave_ops.h"

namespace liodom_dev {

constexpr int kPlaceDescThreads = 256;
constexpr int kPlaceMatchThreads = 256;
constexpr int kPlaceMatchWaves = kPlaceMatchThreads / 64;      // places of one workgroup and round: one wave each
constexpr int kPlaceTopkThreads = 1024;
constexpr int kPlaceTopkWaves = kPlaceTopkThreads / 64;

// One 256-thread workgroup per row.
//   words      W 64-bit words in the LDS, zeroed by the first W threads
//   edges      one 16-byte load per lane and edge through the cache, consecutive lanes on consecutive edges
//   bit        the comparisons of the contract against tables read with uniform indices (scalar loads), then one 64-bit LDS
//              atomicOr per surviving point
//   output     one barrier; the first W lanes of wave 0 store the words (one coalesced store) and the wave sums their popcounts
__global__ __launch_bounds__(kPlaceDescThreads) void k_place_describe(const PlaceTables* __restrict__ tab, int n_rings, int n_layers,
                                                                      const float4* __restrict__ edges, long long edge_stride,
                                                                      const int* __restrict__ n_edges, int edge_cap,
                                                                      unsigned long long* __restrict__ desc, int* __restrict__ bits) {
  __shared__ unsigned long long sh_w[kPlaceWordsMax];
  const int tid = threadIdx.x;
  const int row = blockIdx.x;
  const int W = n_rings * n_layers;               // <= kPlaceWordsMax (checked on the host)
  if (tid < kPlaceWordsMax) sh_w[tid] = 0ull;
  __syncthreads();
  const int n = max(0, min(n_edges[row], edge_cap));
  const float4* src = edges + (long long)row * edge_stride;
  for (int i = tid; i < n; i += kPlaceDescThreads) {
    const float4 p = src[i];
    if (!(ld_isfinite((double)p.x) && ld_isfinite((double)p.y) && ld_isfinite((double)p.z))) continue;
    const float ax = fabsf(p.x), ay = fabsf(p.y);
    int j = 0;
#pragma unroll
    for (int k = 0; k < 15; k++) j += (ay * tab->cs[k] >= ax * tab->cs[16 + k]) ? 1 : 0;
    const bool xn = p.x < 0.0f, yn = p.y < 0.0f;
    const int sector = yn ? (xn ? 32 + j : 63 - j) : (xn ? 31 - j : j);
    const float r2 = p.x * p.x + p.y * p.y;
    int ring = 0;
    for (int k = 0; k < n_rings; k++) ring += (r2 >= tab->r2[k]) ? 1 : 0;
    if (ring >= n_rings) continue;
    if (p.z < tab->z[0]) continue;
    int layer = 0;
    for (int k = 1; k <= n_layers; k++) layer += (p.z >= tab->z[k]) ? 1 : 0;
    if (layer >= n_layers) continue;
    atomicOr(&sh_w[ring * n_layers + layer], 1ull << sector);
  }
  __syncthreads();
  if (tid >= 64) return;
  unsigned long long w = 0ull;
  if (tid < W) { w = sh_w[tid]; desc[(size_t)row * (size_t)W + tid] = w; }
  const int total = wave_incl_scan_i32(__popcll(w));      // lane 63 holds the sum
  if (tid == 63 && bits) bits[row] = total;
}

// One wave per (place, query); lane s is yaw shift s.  Grid x strides the places in groups of kPlaceMatchWaves, y is the query.
//   query      the workgroup builds rot[w][s] = rotl64(q[w], s) once in the LDS (W x 64 x 8 bytes, dynamic: 32 KiB at W = 64) and
//              keeps it for every place it visits; lane s reads rot[w][s]: consecutive lanes, consecutive 8-byte words
//   place      the lanes < W load its words with one coalesced load; word w reaches all lanes as a wave-uniform value (readlane)
//   distance   popcount(rot ^ k) summed over w per lane; the wave minimum of (distance << 6) | shift by DPP / permlane steps
//   output     lane 0 stores one 32-bit key per (query, place).  No atomics.
__global__ __launch_bounds__(kPlaceMatchThreads) void k_place_match(const unsigned long long* __restrict__ places, int n_places, int W,
                                                                    const unsigned long long* __restrict__ queries,
                                                                    unsigned int* __restrict__ keys) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sh_rot[];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int query = blockIdx.y;
  const unsigned long long* q = queries + (size_t)query * (size_t)W;
  for (int w = wave; w < W; w += kPlaceMatchWaves) {
    const unsigned long long v = q[w];
    sh_rot[w * 64 + lane] = (v << lane) | (v >> ((64 - lane) & 63));      // lane 0: v | v
  }
  __syncthreads();
  unsigned int* out = keys + (size_t)query * (size_t)n_places;
  for (int p = (int)blockIdx.x * kPlaceMatchWaves + wave; p < n_places; p += (int)gridDim.x * kPlaceMatchWaves) {
    const unsigned long long mine = lane < W ? places[(size_t)p * (size_t)W + lane] : 0ull;
    const int lo = (int)(unsigned int)mine, hi = (int)(unsigned int)(mine >> 32);
    int d = 0;
    for (int w = 0; w < W; w++) {
      const unsigned long long k = ((unsigned long long)(unsigned int)readlane_i32(hi, w) << 32) | (unsigned int)readlane_i32(lo, w);
      d += __popcll(sh_rot[w * 64 + lane] ^ k);
    }
    const int best = wave_min_i32((d << 6) | lane);      // d <= 64 * 64: the key is below 2^19
    if (lane == 0) out[p] = (unsigned int)best;
  }
}

// the minimum over a wave, uniform over it
__device__ __forceinline__ unsigned long long place_wave_min_u64(unsigned long long v) {
  v = half_min_u64(v);
  const unsigned long long o = xor32_u64(v);
  return o < v ? o : v;
}

// One workgroup of 1024 per query: k rounds of "smallest (distance << 32 | index) + 1 strictly above the previous pick" over the
// query's row of match keys, waves by DPP / permlane steps, the workgroup through one LDS word per wave (two sets, taken in turn:
// one barrier per round).  Writes {index, distance, shift, 0} per rank; ranks beyond the number of places get {-1, 0, 0, 0}.
__global__ __launch_bounds__(kPlaceTopkThreads) void k_place_topk(const unsigned int* __restrict__ keys, int n_places, int k,
                                                                  int4* __restrict__ out) {
  __shared__ unsigned long long sh_min[2][kPlaceTopkWaves];
  const int tid = threadIdx.x;
  const int query = blockIdx.x;
  const unsigned int* row = keys + (size_t)query * (size_t)n_places;
  unsigned long long prev = 0ull;                 // below every candidate: a candidate is its key + 1
  for (int r = 0; r < k; r++) {
    unsigned long long best = ~0ull;
    for (int i = tid; i < n_places; i += kPlaceTopkThreads) {
      const unsigned long long c = (((unsigned long long)(row[i] >> 6) << 32) | (unsigned long long)(unsigned int)i) + 1ull;
      if (c > prev && c < best) best = c;
    }
    best = place_wave_min_u64(best);
    if ((tid & 63) == 0) sh_min[r & 1][tid >> 6] = best;
    __syncthreads();
    best = sh_min[r & 1][0];
#pragma unroll
    for (int w = 1; w < kPlaceTopkWaves; w++) { const unsigned long long o = sh_min[r & 1][w]; best = o < best ? o : best; }
    if (tid == 0) {
      int4 res = make_int4(-1, 0, 0, 0);
      if (best != ~0ull) {
        const int idx = (int)(unsigned int)(best - 1ull);
        res = make_int4(idx, (int)((best - 1ull) >> 32), (int)(row[idx] & 63u), 0);
      }
      out[(size_t)query * (size_t)k + r] = res;
    }
    prev = best;                                  // ~0: nothing is above it, every later rank is -1 too
  }
}

}  // namespace liodom_dev
